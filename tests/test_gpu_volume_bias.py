"""Bias-field matching (GPU): csrc/volume_bias.hip against the numpy specification of volume_bias.py (itself checked in
tests/test_volume_bias_host.py) - the masked Gaussian sums, the pairwise and the single-scan form bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import biasutil as B                                             # noqa: E402
from mri_superresolution_amd import volume_bias as V             # noqa: E402

E_ARG, E_SHAPE = -1, -2      # MRISR_E_ARG, MRISR_E_SHAPE (include/mrisr.h)
R128 = 128 / 3               # ceil(3 sigma) = 128, the largest radius
# (shape, sigmas in voxels per axis).  Radii: larger than the axis (sigma 4 on the axis of 5), 0 on an axis, 128 on the axis of 64;
# 94 | 95 and 126 | 127, where the y / x passes change their outputs per thread (4 | 2 | 1); 128 on each axis in turn.
CASES = [
    ((19, 23, 37), (1.5, 2.0, 3.0)),
    ((19, 23, 37), (0.0, 0.4, 0.0)),
    ((8, 8, 8), (1.0, 1.0, 1.0)),
    ((8, 8, 8), (31.3, 31.6, 42.0)),
    ((8, 8, 8), (42.3, R128, R128)),
    ((8, 8, 8), (R128, 42.3, 31.6)),
    ((40, 48, 36), (4.0, 4.0, 4.0)),
    ((5, 64, 12), (4.0, R128, 0.0)),
    ((5, 64, 12), (0.3, 6.0, 2.0)),
    ((2, 3, 290), (0.5, 0.5, 5.0)),      # the one long axis: a row of more than one 256-voxel tile of the z pass
]


def volume(shape, seed):
    """Positive and negative values, a few NaNs."""
    rng = np.random.default_rng([seed, *shape])
    v = rng.normal(200.0, 300.0, shape).astype(np.float32)
    v.reshape(-1)[rng.choice(v.size, max(1, v.size // 97), replace=False)] = np.nan
    v.reshape(-1)[rng.choice(v.size, 3, replace=False)] = [0.0, -0.0, 1e-30]
    return v


def masks(shape, seed):
    rng = np.random.default_rng([seed, 7, *shape])
    dense = np.where(rng.random(shape) < 0.8, rng.choice(np.array([1, 2, 255], dtype=np.uint8), shape), 0).astype(np.uint8)
    return {"dense": dense, "sparse": (rng.random(shape) < 0.03).astype(np.uint8), "empty": np.zeros(shape, dtype=np.uint8),
            "bool": rng.random(shape) < 0.5}


def on_device(a, offset=0):
    """A CUDA copy of ``a``; ``offset``: its base pointer that many elements past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.cuda()
    buf = torch.zeros(a.size + 8, dtype=t.dtype, device="cuda")
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (offset * t.element_size()) % 16 and view.is_contiguous()
    return view


def equal_bits(got, want):
    got = got.cpu().numpy()
    return got.dtype == want.dtype == np.float32 and got.shape == want.shape and np.array_equal(B.bits(got), B.bits(want))


@pytest.mark.parametrize("shape,sigmas", CASES)
def test_smooth_masked_equals_the_specification_bit_for_bit(shape, sigmas):
    v = volume(shape, 1)
    for name, m in masks(shape, 1).items():
        want_num, want_den = V.smooth_masked_np(v, m, sigmas)
        num, den = V.smooth_masked(on_device(v), on_device(m), sigmas)
        assert equal_bits(num, want_num) and equal_bits(den, want_den), (shape, sigmas, name)
    # the volume one float, the mask one byte past a 16-byte boundary: no 16-byte accesses
    m = masks(shape, 1)["dense"]
    want_num, want_den = V.smooth_masked_np(v, m, sigmas)
    for vo, mo in ((1, 0), (0, 1), (1, 3)):
        num, den = V.smooth_masked(on_device(v, vo), on_device(m, mo), sigmas)
        assert equal_bits(num, want_num) and equal_bits(den, want_den), (shape, sigmas, vo, mo)


@pytest.mark.parametrize("shape,sigmas", [CASES[0], CASES[2], CASES[6], CASES[7]])
@pytest.mark.parametrize("want_field", [True, False])
def test_match_bias_and_correct_bias_equal_the_specification(shape, sigmas, want_field):
    src, ref = volume(shape, 2), np.abs(volume(shape, 3)) + np.float32(50)
    ms, mr = masks(shape, 2), masks(shape, 3)
    ws = V.BiasWorkspace(shape, sigmas, "cuda")
    for sname, rname, offset in (("dense", "dense", 0), ("dense", "bool", 1), ("sparse", "dense", 0), ("empty", "dense", 0)):
        want_out, want_field_np = V.match_bias_np(src, ref, ms[sname], mr[rname], sigmas)
        out, field = V.match_bias(on_device(src, offset), on_device(ref), on_device(ms[sname]), on_device(mr[rname]), sigmas,
                                  workspace=ws if offset == 0 else None, want_field=want_field)
        assert B.same_bits(out.cpu().numpy(), want_out), (shape, sname, rname)
        assert (field is None) if not want_field else equal_bits(field, want_field_np), (shape, sname, rname)
        if sname == "empty":
            assert B.same_bits(out.cpu().numpy(), src) and (want_field_np == 1).all()
    for name, limit in (("dense", 4.0), ("sparse", 1.25), ("empty", 4.0), ("bool", 4.0)):
        want_out, want_field_np = V.correct_bias_np(src, ms[name], sigmas, limit)
        out, field = V.correct_bias(on_device(src), on_device(ms[name]), sigmas, limit, workspace=ws, want_field=want_field)
        assert B.same_bits(out.cpu().numpy(), want_out), (shape, name)
        assert (field is None) if not want_field else equal_bits(field, want_field_np), (shape, name)


def test_phantom_on_the_device():
    src, ref, _, sm, rm = B.phantom()
    for sigma in (4.0, 8.0):
        want_out, want_field = V.match_bias_np(src, ref, sm, rm, (sigma,) * 3)
        out, field = V.match_bias(on_device(src), on_device(ref), on_device(sm), on_device(rm), (sigma,) * 3)
        assert equal_bits(out, want_out) and equal_bits(field, want_field)
    want_out, want_field = V.correct_bias_np(src, sm, (6.0,) * 3)
    out, field = V.correct_bias(on_device(src), on_device(sm), (6.0,) * 3)
    assert equal_bits(out, want_out) and equal_bits(field, want_field)


def test_match_bias_in_one_graph():
    """match_bias captured in one torch.cuda.graph - one stream, a linear chain, the workspace made before the capture - and
    replayed twice on new data: there is no host read in the chain."""
    shape, sigmas = (19, 23, 37), (1.5, 2.0, 3.0)
    first = (volume(shape, 4), np.abs(volume(shape, 5)) + np.float32(50), masks(shape, 4)["dense"], masks(shape, 5)["dense"])
    second = (volume(shape, 6), np.abs(volume(shape, 7)) + np.float32(50), masks(shape, 6)["sparse"], masks(shape, 7)["dense"])
    src, ref, sm, rm = (on_device(a) for a in first)
    ws = V.BiasWorkspace(shape, sigmas, "cuda")
    eager_out, eager_field = V.match_bias(src, ref, sm, rm, sigmas)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        V.match_bias(src, ref, sm, rm, sigmas, workspace=ws)      # warm-up: code objects loaded
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, field = V.match_bias(src, ref, sm, rm, sigmas, workspace=ws)
    for data in (first, second):
        for t, a in zip((src, ref, sm, rm), data):
            t.copy_(torch.from_numpy(a))
        graph.replay()
        torch.cuda.synchronize()
        want_out, want_field = V.match_bias_np(*data, sigmas)
        assert B.same_bits(out.cpu().numpy(), want_out) and equal_bits(field, want_field)
        if data is first:
            assert B.same_bits(out.cpu().numpy(), eager_out.cpu().numpy()) and torch.equal(field, eager_field)


def test_device_argument_errors():
    v = torch.zeros((4, 4, 4), dtype=torch.float32, device="cuda")
    m = torch.ones((4, 4, 4), dtype=torch.uint8, device="cuda")
    sig = (1.0, 1.0, 1.0)
    with pytest.raises(ValueError):
        V.smooth_masked(v.double(), m, sig)
    with pytest.raises(ValueError):
        V.smooth_masked(v[:, :, ::2], m[:, :, ::2], sig)
    with pytest.raises(ValueError):
        V.smooth_masked(v, m[:3], sig)
    with pytest.raises(ValueError):
        V.smooth_masked(v, m.int(), sig)
    with pytest.raises(ValueError):
        V.smooth_masked(v, m, (43.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        V.match_bias(v, torch.zeros((4, 4, 5), device="cuda"), m, torch.ones((4, 4, 5), dtype=torch.uint8, device="cuda"), sig)
    with pytest.raises(ValueError):
        V.correct_bias(v, m, sig, limit=0.0)
    with pytest.raises(ValueError):
        V.correct_bias(v, m, sig, workspace=V.BiasWorkspace((4, 4, 5), sig, "cuda"))
    with pytest.raises(ValueError):
        V.correct_bias(v, m, sig, workspace=V.BiasWorkspace((4, 4, 4), (1.0, 1.0, 2.0), "cuda"))
    # the C entry points refuse on their own and launch nothing: the outputs keep their sentinel
    from mri_superresolution_amd import _lib as L
    lib = L.load()
    ws = V.BiasWorkspace((4, 4, 4), sig, "cuda")
    num, den = torch.full_like(v, -7.0), torch.full_like(v, -7.0)
    t = [x.data_ptr() for x in ws.taps]
    tmp = ws.sums[0].data_ptr()

    def smooth(vol=v.data_ptr(), mask=m.data_ptr(), X=4, Y=4, Z=4, t0=t[0], r0=3, t1=t[1], r1=3, t2=t[2], r2=3, n=num.data_ptr(),
               d=den.data_ptr(), tmp=tmp):
        return lib.mrisr_f32_volume_smooth_masked(vol, mask, None, X, Y, Z, t0, r0, t1, r1, t2, r2, n, d, tmp, None)

    assert smooth(r0=129) == E_SHAPE and smooth(r1=129) == E_SHAPE and smooth(r2=129) == E_SHAPE and smooth(r2=-1) == E_SHAPE
    assert smooth(t0=None) == E_SHAPE and smooth(t1=None) == E_SHAPE and smooth(t2=None) == E_SHAPE
    assert smooth(X=0) == E_SHAPE and smooth(Z=32768) == E_SHAPE
    assert smooth(vol=None) == E_ARG and smooth(mask=None) == E_ARG and smooth(n=None) == E_ARG and smooth(tmp=None) == E_ARG
    assert smooth(d=num.data_ptr()) == E_ARG
    out = torch.full_like(v, -7.0)

    def apply(src=v.data_ptr(), n=64, nu=num.data_ptr(), de=den.data_ptr(), nr=num.data_ptr(), dr=den.data_ptr(), p50=None, count=None,
              limit=4.0, mode=V.MODE_PAIR, o=out.data_ptr()):
        return lib.mrisr_f32_volume_bias_apply(src, n, nu, de, nr, dr, p50, count, limit, mode, None, o, None)

    assert apply(src=None) == E_ARG and apply(nr=None) == E_ARG and apply(o=None) == E_ARG and apply(mode=3) == E_ARG
    assert apply(mode=V.MODE_HUM) == E_ARG and apply(limit=0.5) == E_ARG and apply(limit=float("nan")) == E_ARG
    assert apply(n=0) == E_SHAPE
    torch.cuda.synchronize()
    assert (num == -7).all() and (den == -7).all() and (out == -7).all()
    assert smooth() == 0 and apply() == 0
    torch.cuda.synchronize()
    assert ((den > 0) & (den <= 1)).all() and (num == 0).all() and (out == 0).all()
