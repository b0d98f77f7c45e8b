"""Surface distances on the device (GPU): every kernel of csrc/volume_surface.hip against the numpy specification of
mri_superresolution_amd/volume_surface.py, bit for bit, at the smallest shapes at which a kernel can go wrong - extents of 1, lines
longer than a wave and longer than 256 on every axis, fewer lines than a tile, every tile width, more than one workgroup - and the
three distances end to end."""
import math

import numpy as np
import pytest
import torch

from mri_superresolution_amd import volume_surface as S

pytestmark = pytest.mark.gpu

# (33, 17, 65): tiles of 64 columns along axis 1 and 0, partial ones; (300, 2, 3): 16 columns, a line of 300 along axis 0;
# (3, 300, 2): 16 columns, fewer than a tile; (2, 3, 300): rows longer than 256 for the wave pass, 64 columns for axis 0;
# (9, 40, 20): 32 columns along axis 1
EDT_SHAPES = [(1, 1, 1), (1, 1, 70), (33, 17, 65), (300, 2, 3), (3, 300, 2), (2, 3, 300), (9, 40, 20)]
WEIGHTS = [(1.0, 1.0, 1.0), (0.64, 1.0, 6.25)]
DENSITIES = {"none": 0.0, "one": None, "sparse": 0.01, "dense": 0.5}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def labels_volume(shape, seed, top=3):
    return np.random.default_rng(seed).integers(0, top + 1, shape, dtype=np.uint8)


def sites_volume(shape, kind, seed):
    rng = np.random.default_rng(seed)
    kinds = rng.integers(1, 4, shape, dtype=np.uint8)                  # the bytes 1..3: value 2 picks a third of the sites
    if DENSITIES[kind] is None:
        on = np.zeros(shape, dtype=bool)
        on.reshape(-1)[rng.integers(0, on.size)] = True
        kinds[on] = 2
    else:
        on = rng.random(shape) < DENSITIES[kind]
    return np.where(on, kinds, 0).astype(np.uint8)


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 3, 2), (33, 17, 65)])
def test_label_boundary_equals_the_specification(shape):
    labels = labels_volume(shape, sum(shape))
    for background in (True, False):
        got = S.label_boundary(dev(labels), background)
        assert got.dtype == torch.uint8 and np.array_equal(host(got), S.boundary_np(labels, background))
    blocks = np.repeat(np.repeat(np.repeat(labels_volume((2, 2, 2), 5), 3, 0), 3, 1), 3, 2)[:shape[0], :shape[1], :shape[2]]
    for background in (True, False):                                   # interiors that are not boundary
        assert np.array_equal(host(S.label_boundary(dev(blocks), background)), S.boundary_np(blocks, background))


@pytest.mark.parametrize("shape", EDT_SHAPES)
def test_distance_transform_equals_the_specification_bit_for_bit(shape):
    for kind in DENSITIES:
        sites = sites_volume(shape, kind, 7 * sum(shape) + len(kind))
        d = dev(sites)
        for weights in WEIGHTS:
            for value in (0, 2):
                want = S.edt_sq_np(sites, value, weights)
                got = S.distance_transform_sq(d, value, weights)
                assert got.dtype == torch.float32 and np.array_equal(bits(host(got)), bits(want)), (kind, weights, value)
                full = torch.empty_like(got)
                S._edt_launch(d, d.shape, value, S._check_weights(weights), full, full_scan=True)
                assert torch.equal(full.view(torch.int32), got.view(torch.int32)), (kind, weights, value)
        if kind == "none":
            assert np.isposinf(host(got)).all()
    again = S.distance_transform_sq(d, 0, WEIGHTS[1], out=torch.empty(shape, dtype=torch.float32, device="cuda"))
    assert np.array_equal(bits(host(again)), bits(S.edt_sq_np(sites, 0, WEIGHTS[1])))


def test_distance_transform_checks_its_arguments():
    d = dev(np.zeros((2, 3, 4), np.uint8))
    with pytest.raises(ValueError, match="limit of 1024"):
        S.distance_transform_sq(torch.zeros((1, 1, 1025), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="weights"):
        S.distance_transform_sq(d, 0, (1, 0, 1))
    with pytest.raises(ValueError, match="value"):
        S.distance_transform_sq(d, 256)
    with pytest.raises(ValueError, match="out must be"):
        S.distance_transform_sq(d, 0, (1, 1, 1), out=torch.empty((2, 3, 5), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="uint8"):
        S.distance_transform_sq(d.float())


@pytest.mark.parametrize("n", [1, 4097, 20 * 22 * 24])
def test_gather_equals_its_definition_and_repeats_its_bits(n):
    rng = np.random.default_rng(n)
    d2 = (rng.random(n) * 500.0).astype(np.float32)
    d2[rng.random(n) < 0.1] = np.inf
    query = rng.integers(0, 4, n, dtype=np.uint8)
    if n == 1:
        query[0] = 2
    d2_d, query_d = dev(d2), dev(query)
    slots = torch.empty(int(S.L.load().mrisr_f32_volume_surface_workspace_bytes()) // 8, dtype=torch.int64, device="cuda")
    runs = []
    for _ in range(2):
        dist, sel = torch.full((n,), -1.0, device="cuda"), torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        result = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        S._gather(d2_d, query_d, 2, dist, sel, slots, result, 0)
        runs.append((host(dist), host(sel), host(result)))
    on = query == 2
    want = np.where(on, np.sqrt(d2), np.float32(0)).astype(np.float32)
    dist, sel, result = runs[0]
    assert np.array_equal(bits(dist), bits(want)) and np.array_equal(sel, on.astype(np.uint8))
    assert int(result[0]) == int(on.sum())
    assert bits(np.array([want[on].max()], np.float32))[0] == int(result[2])
    total = math.fsum(float(x) for x in want[on] if np.isfinite(x))
    assert abs(float(result[1:2].view(np.float64)[0]) - total) <= n * 2.0 ** -52 * total
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _boxes(shift=3):
    a, b = np.zeros((16, 16, 16), dtype=np.uint8), np.zeros((16, 16, 16), dtype=np.uint8)
    a[2:10, 4:12, 4:12] = 1
    b[2 + shift:10 + shift, 4:12, 4:12] = 1
    return a, b


def _same(got, want):
    assert got.counts.dtype == np.int64 and np.array_equal(got.counts, want.counts)
    assert np.array_equal(got.hd, want.hd, equal_nan=True) and np.array_equal(got.hd95, want.hd95, equal_nan=True)
    assert np.array_equal(np.isnan(got.assd), np.isnan(want.assd))
    n = got.counts.sum(axis=1)
    ok = ~np.isnan(want.assd)
    assert (np.abs(got.assd[ok] - want.assd[ok]) <= n[ok] * 2.0 ** -52 * want.assd[ok]).all()


def test_surface_distances_on_shifted_boxes():
    a, b = _boxes()
    want = S.surface_distances_np(a, b)
    got = S.surface_distances(dev(a), dev(b))
    _same(got, want)
    assert got.hd[0] == 3.0 and np.isnan(got.hd[1:]).all() and got.counts[1:].sum() == 0
    got = S.surface_distances(dev(a), dev(b), 3, (2, 1, 1))
    _same(got, S.surface_distances_np(a, b, 3, (2, 1, 1)))
    assert got.hd[0] == 6.0
    zero = S.surface_distances(dev(a), dev(a), 2)
    assert zero.assd[0] == zero.hd95[0] == zero.hd[0] == 0.0 and np.isnan(zero.hd[1])


def test_surface_distances_on_random_labels_with_a_shared_workspace():
    shape = (20, 22, 24)
    a, b = labels_volume(shape, 1), labels_volume(shape, 2)
    # smooth blocks so that the surfaces are surfaces, with class 3 absent from d
    c = np.repeat(np.repeat(np.repeat(labels_volume((5, 6, 6), 3), 4, 0), 4, 1), 4, 2)[:20, :22, :24].copy()
    d = np.roll(np.where(c == 3, 2, c), 2, axis=1).astype(np.uint8)
    ws = S.SurfaceWorkspace(shape, 3, "cuda")
    first = S.surface_distances(dev(a), dev(b), 3, (0.8, 1.0, 2.5), True, ws)
    second = S.surface_distances(dev(c), dev(d), 3, (0.8, 1.0, 2.5), False, ws)
    third = S.surface_distances(dev(a), dev(b), 3, (0.8, 1.0, 2.5), True, ws)
    _same(first, S.surface_distances_np(a, b, 3, (0.8, 1.0, 2.5), True))
    want = S.surface_distances_np(c, d, 3, (0.8, 1.0, 2.5), False)
    _same(second, want)
    assert want.counts[2, 0] > 0 and want.counts[2, 1] == 0 and np.isnan(second.assd[2]) and np.isnan(second.hd95[2]) and np.isnan(second.hd[2])
    assert np.isfinite(second.assd[:2]).all() and second.hd[0] > 0
    for x, y in zip(first, third):                                     # every run gives the same bits
        assert np.array_equal(x, y, equal_nan=True)
    _same(S.surface_distances(dev(c), dev(d), 3, (0.8, 1.0, 2.5), True), S.surface_distances_np(c, d, 3, (0.8, 1.0, 2.5), True))
    high = a.copy()
    high[3, 3, 3] = 4
    with pytest.raises(ValueError, match="label above 3"):
        S.surface_distances(dev(high), dev(b), 3, workspace=ws)
    with pytest.raises(ValueError, match="SurfaceWorkspace"):
        S.surface_distances(dev(a), dev(b), 2, workspace=ws)
    with pytest.raises(ValueError, match="voxel sizes"):
        S.surface_distances(dev(a), dev(b), 3, (1, 0, 1), workspace=ws)
