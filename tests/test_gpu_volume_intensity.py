"""Intensity standardisation (GPU): csrc/volume_intensity.hip against the numpy specification of volume_intensity.py (itself pinned
to np.percentile in tests/test_volume_intensity_host.py) - the landmarks by value, the map and the whole operation bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import registerutil as U                                             # noqa: E402
from test_percentile_host import CLASSES, input_class                # noqa: E402
from mri_superresolution_amd import volume_intensity as I            # noqa: E402
from mri_superresolution_amd.volume_eval import foreground_mask, foreground_mask_np      # noqa: E402

SIXTEEN = (0, 0, 1, 5, 5, 10, 25, 50, 50, 50, 75, 90, 99, 99.5, 100, 100)
PERCENTILE_SETS = [I.LANDMARKS, (1, 99), (0, 100), (50,), SIXTEEN]
SMALL = [(1, 1, 1), (1, 1, 2), (1, 1, 3), (7, 5, 3), (1, 1, 201), (24, 40, 3)]
MANY_BLOCKS = (96, 80, 64)


def volume(name, shape, seed=0):
    return np.ascontiguousarray(input_class(name, (shape[0] * shape[1], shape[2]), seed).reshape(shape))


def mask_cases(shape, seed=0):
    rng = np.random.default_rng([seed, *shape])
    n = int(np.prod(shape))
    one, two = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    one[n // 2] = 1
    two[[0, n - 1]] = 1
    box = np.zeros(shape, dtype=np.uint8)
    box[shape[0] // 4:shape[0] // 4 + max(1, shape[0] // 2), shape[1] // 4:shape[1] // 4 + max(1, shape[1] // 2),
        shape[2] // 4:shape[2] // 4 + max(1, shape[2] // 2)] = 1
    odd = np.where(rng.random(n) < 0.5, rng.choice(np.array([2, 255], dtype=np.uint8), n), 0).astype(np.uint8)
    return {"none": None, "ones": np.ones(shape, dtype=np.uint8), "half": (rng.random(shape) < 0.5).astype(np.uint8),
            "one_voxel": one.reshape(shape), "two_voxels": two.reshape(shape), "box": box, "values_2_255": odd.reshape(shape)}


def device_landmarks(v, m, qs, workspace=None):
    out, count = I.masked_percentiles(torch.from_numpy(v).cuda(), None if m is None else torch.from_numpy(m).cuda(), qs, workspace)
    assert out.dtype == torch.float32 and out.shape == (len(qs),) and count.dtype == torch.int64 and count.shape == (1,)
    return out.cpu().numpy(), int(count.cpu()[0])


def check(v, m, qs, what, workspace=None):
    want, n = I.landmarks_np(v, m, qs if len(qs) > 1 else tuple(qs) * 2)      # the specification takes two or more
    want = want[:len(qs)]
    got, count = device_landmarks(v, m, qs, workspace)
    assert count == n, (what, count, n)
    assert np.array_equal(got, want, equal_nan=True), (what, got, want)       # by value: -0.0 == +0.0


@pytest.mark.parametrize("name", CLASSES)
def test_masked_percentiles_small(name):
    for shape in SMALL:
        v = volume(name, shape)
        for mname, m in mask_cases(shape).items():
            sets = PERCENTILE_SETS if mname in ("none", "half") else [I.LANDMARKS]
            for qs in sets:
                check(v, m, qs, (name, shape, mname, qs))


@pytest.mark.parametrize("name", ["mri", "normal", "last_digit"])
def test_masked_percentiles_many_workgroups(name):
    v = volume(name, MANY_BLOCKS)
    masks = mask_cases(MANY_BLOCKS)
    for mname in ("none", "half", "box", "values_2_255", "two_voxels"):
        check(v, masks[mname], I.LANDMARKS, (name, mname))
    check(v, masks["half"], SIXTEEN, (name, "half", "sixteen"))
    # an all-ones mask is no mask
    a, b = device_landmarks(v, masks["ones"], I.LANDMARKS), device_landmarks(v, None, I.LANDMARKS)
    assert a[1] == b[1] == v.size and np.array_equal(a[0].view(np.int32), b[0].view(np.int32))


def test_masked_percentiles_more_than_2_24_voxels():
    """257^3 > 2^24: counts and ranks beyond float32's integers - the virtual index float32(count - 1) * q32 is a rounded product,
    and the rule clamps its floor to count - 1."""
    shape = (257, 257, 257)
    v = volume("mri", shape)
    assert v.size > 2 ** 24
    check(v, None, (0, 1, 10, 50, 90, 99, 99.9999, 100), "257^3")


def test_volume_off_the_16_byte_boundary():
    shape = (7, 5, 3)
    for name in ("normal", "mri"):
        v = volume(name, shape)
        buf = torch.zeros(v.size + 8, dtype=torch.float32, device="cuda")
        assert buf.data_ptr() % 16 == 0
        view = buf[1:1 + v.size].view(shape)
        view.copy_(torch.from_numpy(v))
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        for m in (None, mask_cases(shape)["half"]):
            out, count = I.masked_percentiles(view, None if m is None else torch.from_numpy(m).cuda())
            want, n = I.landmarks_np(v, m)
            assert int(count.cpu()[0]) == n and np.array_equal(out.cpu().numpy(), want)
        # a mask that starts off a 4-byte boundary, under an aligned volume
        m = mask_cases(shape)["half"]
        mbuf = torch.zeros(v.size + 8, dtype=torch.uint8, device="cuda")
        mview = mbuf[1:1 + v.size].view(shape)
        mview.copy_(torch.from_numpy(m))
        out, count = I.masked_percentiles(torch.from_numpy(v).cuda(), mview)
        want, n = I.landmarks_np(v, m)
        assert int(count.cpu()[0]) == n and np.array_equal(out.cpu().numpy(), want)


def test_nan_voxels_lowest_byte_and_all_equal():
    shape = (24, 40, 3)
    v = volume("normal", shape).copy()
    rng = np.random.default_rng(11)
    v.reshape(-1)[rng.choice(v.size, 200, replace=False)] = np.nan
    for mname in ("none", "half", "box"):
        check(v, mask_cases(shape)[mname], I.LANDMARKS, ("nan", mname))
    check(np.full(shape, np.nan, dtype=np.float32), None, I.LANDMARKS, "all nan")
    # values that differ only in their lowest byte: all 32 targets share one histogram until the last pass
    low = (1.0 + rng.permutation(v.size)[:v.size] % 256 * 2.0 ** -23).astype(np.float32).reshape(shape)
    for qs in (I.LANDMARKS, SIXTEEN):
        check(low, None, qs, "lowest byte")
        check(low, mask_cases(shape)["half"], qs, "lowest byte, half")
    for value in (1234.5, 0.0, -7.25):
        check(np.full(shape, value, dtype=np.float32), mask_cases(shape)["half"], I.LANDMARKS, ("constant", value))
    zeros = np.zeros(shape, dtype=np.float32)
    zeros.reshape(-1)[::3] = -0.0
    check(zeros, None, I.LANDMARKS, "signed zeros")


def test_empty_mask_then_a_normal_call_on_the_same_workspace():
    shape = (24, 40, 3)
    v = volume("mri", shape)
    ws = I.percentiles_workspace(11, "cuda")
    got, count = device_landmarks(v, np.zeros(shape, dtype=np.uint8), I.LANDMARKS, ws)
    assert count == 0 and np.isnan(got).all()
    check(v, mask_cases(shape)["half"], I.LANDMARKS, "after an empty mask", ws)


def test_workspace_needs_no_initialisation():
    ws = I.percentiles_workspace(16, "cuda")
    ws.fill_(0x5A5A5A5A)
    check(volume("normal", MANY_BLOCKS), mask_cases(MANY_BLOCKS)["half"], SIXTEEN, "first call", ws)
    check(volume("mri", (24, 40, 3)), None, I.LANDMARKS, "second call", ws)


def same_bits(a, b):
    """Equal int32 views wherever there is a number, NaNs in the same places (a NaN's sign and payload are nobody's rule)."""
    if not (a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))):
        return False
    number = ~np.isnan(a)
    return np.array_equal(a.view(np.int32)[number], b.view(np.int32)[number])


def map_landmarks(L, kind, rng):
    s = np.sort(rng.uniform(0, 4000, L)).astype(np.float32)
    d = np.sort(rng.uniform(-50, 900, L)).astype(np.float32)
    if kind == "zero_first":
        s[1] = s[0]
    elif kind == "zero_interior" and L > 3:
        s[L // 2] = s[L // 2 - 1]
    elif kind == "zero_last":
        s[-1] = s[-2]
    elif kind == "nan_source":
        s[:] = np.nan
    elif kind == "nan_target":
        d[:] = np.nan
    elif kind == "nan_both":
        s[:], d[:] = np.nan, np.nan
    return s, d


def map_voxels(n, s, rng):
    """Below, on, next to, between and above the landmarks; a NaN and both infinities."""
    finite = s[np.isfinite(s)] if np.isfinite(s).any() else np.array([0, 4000], dtype=np.float32)
    lo, hi = float(finite.min()), float(finite.max())
    x = rng.uniform(lo - 0.3 * (hi - lo) - 1, hi + 0.3 * (hi - lo) + 1, n).astype(np.float32)
    special = np.concatenate([finite, np.nextafter(finite, np.float32(-np.inf)), np.nextafter(finite, np.float32(np.inf)),
                              np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)]).astype(np.float32)
    k = min(n, special.size)
    x[rng.choice(n, k, replace=False)] = special[rng.permutation(special.size)[:k]]
    return x


@pytest.mark.parametrize("L", [2, 11, 16])
def test_piecewise_map_equals_the_specification_bit_for_bit(L):
    rng = np.random.default_rng(L)
    for n in (1, 3, 105, 201, 491520):
        kinds = ("plain", "zero_first", "zero_interior", "zero_last", "nan_source", "nan_target", "nan_both") if n <= 201 else ("plain", "zero_interior")
        for kind in kinds:
            s, d = map_landmarks(L, kind, rng)
            x = map_voxels(n, s, rng)
            want = I.piecewise_map_np(x, s, d)
            xs, sl, dl = torch.from_numpy(x).cuda(), torch.from_numpy(s).cuda(), torch.from_numpy(d).cuda()
            got = I.piecewise_map(xs, sl, dl).cpu().numpy()
            assert same_bits(got, want), (L, n, kind)
            if kind.startswith("nan"):
                assert np.isnan(got).all()
            # out aliasing the input, and an input off the 16-byte boundary
            assert I.piecewise_map(xs, sl, dl, out=xs) is xs and same_bits(xs.cpu().numpy(), want), (L, n, kind, "in place")
            buf = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
            buf[1:1 + n] = torch.from_numpy(x).cuda()
            assert same_bits(I.piecewise_map(buf[1:1 + n], sl, dl).cpu().numpy(), want), (L, n, kind, "unaligned")


def distorted_pair():
    fixed, _ = U.synthetic_pair()
    x = np.clip(fixed.astype(np.float64), 0.0, None)
    source = (700.0 * (x / float(fixed.max())) ** 0.7 + 0.05 * x + 40.0).astype(np.float32)
    return source, fixed.copy()      # writable copies: torch.from_numpy wants them so


def test_match_intensity_equals_the_specification_with_otsu_masks():
    source, target = distorted_pair()
    smask_np, tmask_np = foreground_mask_np(source), foreground_mask_np(target)
    want, found_np = I.match_intensity_np(source, target, smask_np, tmask_np)
    src, tgt = torch.from_numpy(source).cuda(), torch.from_numpy(target).cuda()
    smask, tmask = foreground_mask(src)[0], foreground_mask(tgt)[0]
    assert np.array_equal(smask.cpu().numpy(), smask_np) and np.array_equal(tmask.cpu().numpy(), tmask_np)
    got, found = I.match_intensity(src, tgt, smask, tmask)
    assert same_bits(got.cpu().numpy(), want)
    assert found.percentiles == found_np.percentiles and found.source_count == found_np.source_count and found.target_count == found_np.target_count
    assert same_bits(found.source_landmarks, found_np.source_landmarks) and same_bits(found.target_landmarks, found_np.target_landmarks)
    got2, found2 = I.match_intensity(src, tgt, None, None, I.RANGE)
    want2, found2_np = I.match_intensity_np(source, target, None, None, I.RANGE)
    assert same_bits(got2.cpu().numpy(), want2) and found2.source_count == source.size and same_bits(found2.source_landmarks, found2_np.source_landmarks)
    with pytest.raises(ValueError, match="no voxels"):
        I.match_intensity(src, tgt, torch.zeros_like(smask), tmask)
    with pytest.raises(ValueError, match="constant foreground"):
        I.match_intensity(torch.full_like(src, 2.5), tgt)


def test_landmarks_and_map_in_one_graph():
    """masked_percentiles + piecewise_map captured in one torch.cuda.graph - one stream, a linear chain, the workspace allocated
    before the capture - and replayed on new data: there is no host read in the chain."""
    shape = (24, 40, 3)
    first, second = volume("normal", shape), volume("mri", shape, seed=5)
    m1, m2 = mask_cases(shape)["half"], mask_cases(shape, seed=3)["box"]
    d = np.linspace(0, 1000, 11).astype(np.float32)
    vol, mask, dl = torch.from_numpy(first).cuda(), torch.from_numpy(m1).cuda(), torch.from_numpy(d).cuda()
    ws = I.percentiles_workspace(11, "cuda")
    out = torch.empty_like(vol)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        I.piecewise_map(vol, I.masked_percentiles(vol, mask, I.LANDMARKS, ws)[0], dl, out=out)      # warm-up: code objects loaded
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sl, count = I.masked_percentiles(vol, mask, I.LANDMARKS, ws)
        I.piecewise_map(vol, sl, dl, out=out)
    for v, m in ((first, m1), (second, m2)):
        vol.copy_(torch.from_numpy(v))
        mask.copy_(torch.from_numpy(m))
        graph.replay()
        torch.cuda.synchronize()
        want_sl, n = I.landmarks_np(v, m)
        assert int(count.cpu()[0]) == n and np.array_equal(sl.cpu().numpy(), want_sl)
        assert same_bits(out.cpu().numpy(), I.piecewise_map_np(v, want_sl, d))


def test_device_argument_errors():
    v = torch.zeros((4, 4, 4), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        I.masked_percentiles(v.double())
    with pytest.raises(ValueError):
        I.masked_percentiles(v[:, :, ::2])
    with pytest.raises(ValueError):
        I.masked_percentiles(v, torch.ones((4, 4, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        I.masked_percentiles(v, torch.ones((4, 4, 4), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        I.masked_percentiles(v, None, ())
    with pytest.raises(ValueError):
        I.masked_percentiles(v, None, tuple(range(17)))
    with pytest.raises(ValueError):
        I.masked_percentiles(v, None, (50,), torch.empty(8, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        I.piecewise_map(v, torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda"))
    with pytest.raises(ValueError):
        I.piecewise_map(v, torch.zeros(3, device="cuda"), torch.zeros(2, device="cuda"))
    with pytest.raises(ValueError):
        I.piecewise_map(v, torch.zeros(2, device="cuda"), torch.zeros(2, device="cuda"), out=torch.zeros(5, device="cuda"))
    # the C entry points refuse on their own
    from mri_superresolution_amd import _lib as L
    lib = L.load()
    assert lib.mrisr_f32_masked_percentiles_workspace_bytes(0) == 0 == lib.mrisr_f32_masked_percentiles_workspace_bytes(17)
    ws, out, count = I.percentiles_workspace(2, "cuda"), torch.empty(2, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda")
    q = (L.C.c_double * 2)(60.0, 40.0)
    assert lib.mrisr_f32_volume_masked_percentiles(v.data_ptr(), None, 64, q, 2, out.data_ptr(), count.data_ptr(), ws.data_ptr(), None) != 0
    q = (L.C.c_double * 2)(40.0, 60.0)
    assert lib.mrisr_f32_volume_masked_percentiles(v.data_ptr(), None, 0, q, 2, out.data_ptr(), count.data_ptr(), ws.data_ptr(), None) != 0
    assert lib.mrisr_f32_volume_masked_percentiles(v.data_ptr(), None, 2 ** 32, q, 2, out.data_ptr(), count.data_ptr(), ws.data_ptr(), None) != 0
    assert lib.mrisr_f32_volume_masked_percentiles(v.data_ptr(), None, 64, q, 2, None, count.data_ptr(), ws.data_ptr(), None) != 0
    assert lib.mrisr_f32_volume_piecewise_map(v.data_ptr(), 64, out.data_ptr(), out.data_ptr(), 17, v.data_ptr(), None) != 0
