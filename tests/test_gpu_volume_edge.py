"""Edge sharpness on the device (GPU): every kernel of csrc/volume_edge.hip against the numpy specification of
mri_superresolution_amd/volume_sharpness.py at the smallest shapes at which a kernel can go wrong - one voxel, a run shorter than a
wave and one that is no multiple of it, more than one workgroup, more slots than the last pass adds in one step - and
``evaluate_volume(tissue_edges=True)`` end to end."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edgeutil as E                                                         # noqa: E402
from mri_superresolution_amd import volume_sharpness as V                    # noqa: E402

pytestmark = pytest.mark.gpu

SIDES_SHAPES = [(1, 1, 1), (1, 1, 70), (33, 17, 65), (300, 2, 3)]
SPACINGS = [(1.0, 1.0, 1.0), (0.8, 1.0, 2.5)]
# (70, 64, 64): 286720 voxels are 70 workgroups of 4096, more than the 64 slots the last pass adds in one step
PROFILE_SHAPES = [(1, 1, 1), (3, 5, 67), (33, 17, 65), (70, 64, 64)]
RTOL = 1e-12


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def label_cases(shape, seed):
    """Random labels 0..3 in blocks (so that distances exceed 1), and the volumes in which a side is empty."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 4, tuple((d + 3) // 4 for d in shape), dtype=np.uint8)
    blocks = np.repeat(np.repeat(np.repeat(coarse, 4, 0), 4, 1), 4, 2)[:shape[0], :shape[1], :shape[2]].copy()
    return {"blocks": blocks, "random": rng.integers(0, 4, shape, dtype=np.uint8), "dark only": np.minimum(blocks, 1),
            "bright only": np.where(blocks != 0, 3, 0).astype(np.uint8), "empty": np.zeros(shape, dtype=np.uint8)}


@pytest.mark.parametrize("shape", SIDES_SHAPES)
def test_sides_and_signed_distance_equal_the_specification_bit_for_bit(shape):
    for name, labels in label_cases(shape, sum(shape)).items():
        d = dev(labels)
        for k in (1, 2):                                               # K = 3: k = 1 and k = K - 1
            sides = V.interface_sides(d, k)
            assert sides.dtype == torch.uint8 and np.array_equal(host(sides), V.interface_sides_np(labels, k)), (name, k)
            for spacing in SPACINGS:
                want = V.signed_distance_np(labels, k, spacing)
                got = host(V.signed_distance(d, k, spacing))
                assert got.dtype == np.float32
                assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isnan(want), labels == 0), (name, k, spacing)
                ok = ~np.isnan(want)
                assert np.array_equal(bits(got[ok]), bits(want[ok])), (name, k, spacing)      # infinities and signs included
        if name == "dark only":
            assert np.isneginf(got[labels != 0]).all()
        if name == "bright only":
            assert np.isposinf(got[labels != 0]).all()
    labels = label_cases(shape, 1)["blocks"]
    stacked = host(V.signed_distances(dev(labels), 3, SPACINGS[1]))
    assert stacked.shape == (2,) + shape
    for k in (1, 2):
        assert np.array_equal(stacked[k - 1], V.signed_distance_np(labels, k, SPACINGS[1]), equal_nan=True)


def test_signed_distance_checks_its_arguments():
    d = dev(np.ones((2, 3, 4), np.uint8))
    with pytest.raises(ValueError, match="k must be"):
        V.interface_sides(d, 0)
    with pytest.raises(ValueError, match="k must be"):
        V.signed_distance(d, 255)
    with pytest.raises(ValueError, match="voxel sizes"):
        V.signed_distance(d, 1, (1, -1, 1))
    with pytest.raises(ValueError, match="limit of 1024"):
        V.signed_distance(torch.ones((1, 1, 1025), dtype=torch.uint8, device="cuda"), 1)
    with pytest.raises(ValueError, match="uint8"):
        V.signed_distance(d.float(), 1)
    with pytest.raises(ValueError, match="volume \\(X, Y, Z\\)"):
        V.interface_sides(d[0], 1)
    with pytest.raises(ValueError, match="out must be"):
        V.signed_distance(d, 1, out=torch.empty((2, 3, 5), device="cuda"))
    with pytest.raises(ValueError, match="classes must be"):
        V.signed_distances(d, 1)


def profile_case(shape, J, seed, kind="mixed"):
    """-> (vol, sdist): signed distances that vary slowly along z, as real ones do, so that lanes of a wave share bins, with NaN and
    both infinities among them; a volume with NaN and inf."""
    rng = np.random.default_rng(seed)
    z = np.arange(shape[2], dtype=np.float64)
    sdist = np.empty((J,) + shape, dtype=np.float32)
    for j in range(J):
        sdist[j] = (0.37 * (z - shape[2] * (j + 1) / (J + 1.0)) + rng.normal(0.0, 0.8, shape)).astype(np.float32)
    vol = rng.normal(500.0, 200.0, shape).astype(np.float32)
    if kind == "one bin":
        sdist[:] = rng.uniform(0.51, 0.99, sdist.shape).astype(np.float32)
    elif kind == "none":
        sdist[:] = np.where(rng.random(sdist.shape) < 0.5, np.float32(-7.5), np.float32(4.0))      # 4.0: the first value past the range
    if kind != "one bin":
        flat = sdist.reshape(-1)
        flat[::13] = np.nan
        flat[5::17] = np.inf
        flat[7::19] = -np.inf
        vol.reshape(-1)[::11] = np.nan
        vol.reshape(-1)[3::23] = np.inf
        vol.reshape(-1)[4::29] = -np.inf
    return vol, sdist


def same_profile(got, want):
    assert got.count.dtype == np.int64 and np.array_equal(got.count, want.count)
    # another order of a float64 sum: the cases keep the terms of a bin at one sign (v > 0; no bin straddles s = 0), so the bound
    # is relative to the sum itself
    for a, b in ((got.sum_v, want.sum_v), (got.sum_s, want.sum_s), (got.sum_vv, want.sum_vv)):
        assert a.dtype == np.float64 and a.shape == b.shape
        scale = np.maximum(np.abs(b), 1e-300)
        assert (np.abs(a - b) <= RTOL * scale).all(), float((np.abs(a - b) / scale).max())


@pytest.mark.parametrize("J,radius,width", [(1, 4.0, 0.5), (5, 1.0, 1.0), (5, 4.0, 0.125), (2, 4.0, 0.5)])
@pytest.mark.parametrize("shape", PROFILE_SHAPES)
def test_edge_profile_equals_the_specification(shape, J, radius, width):
    vol, sdist = profile_case(shape, J, 3 * sum(shape) + J)
    # the terms of a sum share a sign: v > 0 where it is finite, and with these radii and widths no bin straddles s = 0
    vol = np.where(np.isfinite(vol), np.abs(vol) + np.float32(1.0), vol).astype(np.float32)
    want = V.edge_profile_np(vol, sdist, radius, width)
    nb = want.count.shape[1]
    assert nb == {0.5: 16, 1.0: 2, 0.125: 64}[width]
    ws = V.EdgeWorkspace(J, nb, "cuda")
    words = V.edge_profile(dev(vol), dev(sdist), radius, width, ws)
    assert words.dtype == torch.int64 and tuple(words.shape) == (J, nb, 4)
    first = host(words).copy()
    same_profile(V.profile_of(first), want)
    ws.slots.fill_(-1)                                                 # the workspace needs no initialisation
    words.fill_(-1)
    second = host(V.edge_profile(dev(vol), dev(sdist), radius, width, ws))
    assert np.array_equal(first, second)                               # the same bits on every run
    alone = host(V.edge_profile(dev(vol), dev(sdist), radius, width))
    assert np.array_equal(first, alone)
    if np.prod(shape) > 1000:
        assert want.count.sum() > 0


@pytest.mark.parametrize("shape", [(3, 5, 67), (70, 64, 64)])
def test_edge_profile_with_every_voxel_in_one_bin_and_with_none_in_range(shape):
    vol, sdist = profile_case(shape, 2, 5, "one bin")                  # the worst case of the reduction inside a wave
    vol = np.abs(vol) + np.float32(1.0)
    got = V.profile_of(host(V.edge_profile(dev(vol), dev(sdist), 4.0, 0.5)))
    want = V.edge_profile_np(vol, sdist, 4.0, 0.5)
    same_profile(got, want)
    assert (got.count[:, 9] == vol.size).all() and got.count.sum() == 2 * vol.size      # s in [0.5, 1): bin 9 of 16
    vol, sdist = profile_case(shape, 2, 6, "none")
    got = V.profile_of(host(V.edge_profile(dev(vol), dev(sdist), 4.0, 0.5)))
    for a in got:
        assert not a.any()
    assert np.array_equal(got.sum_v, np.zeros((2, 16)))


def test_edge_profile_checks_its_arguments():
    vol, sdist = torch.zeros((2, 3, 4), device="cuda"), torch.zeros((2, 2, 3, 4), device="cuda")
    with pytest.raises(ValueError, match="65 bins"):
        V.edge_profile(vol, sdist, 4.0625, 0.125)
    with pytest.raises(ValueError, match="finite positive"):
        V.edge_profile(vol, sdist, 4.0, 0.0)
    with pytest.raises(ValueError, match="sdist must be"):
        V.edge_profile(vol, sdist[:, :, :, :3].contiguous())
    with pytest.raises(ValueError, match="J in 1..5"):
        V.edge_profile(vol, torch.zeros((6, 2, 3, 4), device="cuda"))
    with pytest.raises(ValueError, match="vol must be"):
        V.edge_profile(vol.double(), sdist)
    with pytest.raises(ValueError, match="EdgeWorkspace\\(2, 16"):
        V.edge_profile(vol, sdist, workspace=V.EdgeWorkspace(1, 16, "cuda"))
    with pytest.raises(ValueError, match="EdgeWorkspace\\(2, 16"):
        V.edge_profile(vol, sdist, workspace=V.EdgeWorkspace(2, 8, "cuda"))
    with pytest.raises(ValueError, match="no CPU fallback"):
        V.edge_profile(vol.cpu(), sdist)


def test_edge_profile_in_a_graph_replayed_on_new_data():
    """edge_profile with an EdgeWorkspace captured in a torch.cuda.graph and replayed on new data: no host read, no allocation."""
    shape = (9, 20, 70)
    (v1, s1), (v2, s2) = profile_case(shape, 2, 1), profile_case(shape, 2, 2)
    vol, sdist = dev(v1), dev(s1)
    ws = V.EdgeWorkspace(2, 16, "cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        V.edge_profile(vol, sdist, 4.0, 0.5, ws)                       # warm-up outside the capture: the code objects are loaded
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        words = V.edge_profile(vol, sdist, 4.0, 0.5, ws)
    for v, s in ((v2, s2), (v1, s1)):
        vol.copy_(torch.from_numpy(v))
        sdist.copy_(torch.from_numpy(s))
        words.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        replayed = host(words).copy()
        eager = host(V.edge_profile(dev(v), dev(s), 4.0, 0.5))
        assert np.array_equal(replayed, eager)
        assert np.array_equal(V.profile_of(replayed).count, V.edge_profile_np(v, s, 4.0, 0.5).count)


def test_edge_sharpness_on_the_phantom_equals_the_specification():
    labels = np.array(E.truth())
    d = dev(labels)
    sdist = V.signed_distances(d, 3)
    ws = V.EdgeWorkspace(2, 16, "cuda")
    widths = []
    for sigma in (0.0, 1.0, 2.0):
        vol = np.array(E.phantom(sigma, E.PHANTOM_NOISE))
        want = V.edge_sharpness_np(vol, labels, 3)
        got = V.edge_sharpness(dev(vol), sdist=sdist, workspace=ws)
        same_profile(got.profile, want.profile)
        assert got.width == pytest.approx(want.width, rel=1e-9) and got.contrast == pytest.approx(want.contrast, rel=1e-9)
        direct = V.edge_sharpness(dev(vol), d, 3)
        assert np.array_equal(direct.width, got.width) and np.array_equal(direct.profile.sum_vv, got.profile.sum_vv)
        widths.append(got.width)
    assert (np.diff(np.array(widths), axis=0) > 0).all()               # sharper is narrower, on the device as in the specification
    aniso = V.edge_sharpness(dev(np.array(E.phantom(1.0))), d, 3, (0.8, 1.0, 2.5), 4.0, 0.5)
    want = V.edge_sharpness_np(np.array(E.phantom(1.0)), labels, 3, (0.8, 1.0, 2.5), 4.0, 0.5)
    same_profile(aniso.profile, want.profile)
    assert aniso.width == pytest.approx(want.width, rel=1e-9, nan_ok=True)


def test_evaluate_volume_tissue_edges(monkeypatch):
    from mri_superresolution_amd.models.unet_model import UNetSuperRes
    from mri_superresolution_amd.volume_eval import evaluate_volume
    torch.manual_seed(1234)
    model = UNetSuperRes(1, 1, base_filters=16).cuda().eval()
    ref = dev(np.array(E.phantom(1.0, E.PHANTOM_NOISE)))
    seen = []
    real = V.signed_distances

    def recording(labels, classes, spacing):
        seen.append((labels.clone(), classes, tuple(spacing)))
        return real(labels, classes, spacing)

    monkeypatch.setattr(V, "signed_distances", recording)
    spacing = (1.0, 1.25, 2.0)
    common = dict(batch_size=4, use_graph=False, mask="otsu", tissue_dice=3)
    res = evaluate_volume(model, ref, tissue_edges=True, spacing=spacing, **common)
    monkeypatch.undo()
    assert list(res.tissue_edges) == ["unet", "linear", "cubic", "reference"] and len(seen) == 1 and res.tissue_surface is None
    labels, classes, used = seen[0]
    assert classes == 3 and used == spacing
    own = res.tissue_edges["reference"]
    want = V.edge_sharpness(ref, labels, 3, spacing, 4.0, 0.5)
    for a, b in zip(own[:2] + tuple(own.profile), want[:2] + tuple(want.profile)):
        assert np.array_equal(a, b, equal_nan=True)
    with np.errstate(invalid="ignore"):
        assert (own.contrast / own.contrast).tolist() == [1.0, 1.0]    # the reference row's econ
    spec = V.edge_sharpness_np(host(ref), host(labels), 3, spacing, 4.0, 0.5)
    same_profile(own.profile, spec.profile)
    assert own.width == pytest.approx(spec.width, rel=1e-9) and np.isfinite(own.width).all()
    for method in ("linear", "cubic"):                                 # the same voxels in every bin: the signed distances are shared
        assert res.tissue_edges[method].profile.count.tolist() == own.profile.count.tolist()
    # linear interpolation of the mean over pairs is a low-pass with a kernel that is nowhere negative: wider than the reference
    assert (res.tissue_edges["linear"].width > own.width).all()
    # other bins, and the rules
    fine = evaluate_volume(model, ref, tissue_edges=True, edge_radius=3.0, edge_bin=0.25, **common)
    assert fine.tissue_edges["reference"].profile.count.shape == (2, 24)
    plain = evaluate_volume(model, ref, **common)
    assert plain.tissue_edges is None
    for method in plain:                                               # the metrics come from float64 atomics: equal to their rounding
        assert host(plain[method]) == pytest.approx(host(res[method]), rel=1e-9, abs=1e-12)
        assert np.array_equal(plain.tissue_dice[method], res.tissue_dice[method])
    with pytest.raises(ValueError, match="tissue_edges needs tissue_dice"):
        evaluate_volume(model, ref, mask="otsu", tissue_edges=True)
