"""csrc/conv_upadj.hip: the input gradient of bilinear x2 (align_corners=True) + 3x3 conv (final_up_bilinear,
unet_model.py:151-152) formed at low resolution in one launch, against a float64 CPU reference of conv-dgrad followed by
the x2 adjoint, and against the two-launch path it replaces (mrisr_conv_forward on the mirrored weights + mrisr_upsample2_adjoint)."""
from __future__ import annotations

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import hiputil as U
from mri_superresolution_amd import _lib as L

pytestmark = pytest.mark.gpu


def ref_f64(g, w, h, wd):
    """d/da of sum(g * conv2d(interpolate(a, x2, bilinear, align_corners=True), w, padding=1)) in float64."""
    a = torch.zeros((g.shape[0], w.shape[1], h, wd), dtype=torch.float64, requires_grad=True)
    up = F.interpolate(a, scale_factor=2, mode="bilinear", align_corners=True)
    y = F.conv2d(up, w.double(), padding=1)
    (da,) = torch.autograd.grad(y, a, g.double())
    return da


def upadj(g, w, dt, h, wd):
    n, cg = g.shape[0], g.shape[1]
    ca = w.shape[1]
    nbytes = L.load().mrisr_packed_weight_bytes_upadj(dt, cg, ca, 3)
    assert nbytes > 0
    wp = torch.empty(nbytes, dtype=torch.uint8, device=U.DEV)
    wd_ = U.w_cl(w)
    L.call("mrisr_pack_weights", dt, wd_.data_ptr(), cg, ca, 3, L.PACK_UPADJ, wp.data_ptr(), U.stream())
    gd = U.nhwc(g, dt)
    out = torch.full((n, h, wd, ca), float("nan"), dtype=U.tdt(dt), device=U.DEV)
    d = L.ConvDesc()
    d.dtype, d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.nsrc = dt, n, 2 * h, 2 * wd, ca, cg, 3, 1
    d.wpacked = wp.data_ptr()
    L.call("mrisr_conv_upadj", C.byref(d), gd.data_ptr(), out.data_ptr(), U.stream())
    torch.cuda.synchronize()
    buf = C.create_string_buffer(96)
    L.call("mrisr_conv_variant", C.byref(d), 2, buf, 96)
    assert buf.value.decode() == f"conv_upadj_kernel<{'bf16' if dt == L.BF16 else 'f16'},{cg},{ca}>"
    return U.nchw(out).double()


def two_launch(g, w, dt, h, wd):
    """The engine's previous path: dgrad conv at 2h x 2w (rounded to dt), then the x2 adjoint."""
    n, cg = g.shape[0], g.shape[1]
    ca = w.shape[1]
    keep = []
    d = U.make_desc(dt, [U.SrcSpec(g)], 2 * h, 2 * wd, cg, ca, 3, keep=keep)
    d.groups = 0
    wp = U.pack(w, dt, 1)
    d.wpacked = wp.data_ptr()
    dx = torch.empty((n, 2 * h, 2 * wd, ca), dtype=U.tdt(dt), device=U.DEV)
    d.out = dx.data_ptr()
    L.call("mrisr_conv_forward", C.byref(d), U.stream())
    out = torch.empty((n, h, wd, ca), dtype=U.tdt(dt), device=U.DEV)
    L.call("mrisr_upsample2_adjoint", dt, dx.data_ptr(), out.data_ptr(), n, h, wd, ca, U.stream())
    torch.cuda.synchronize()
    return U.nchw(out).double()


def errs(got, ref):
    e = got - ref
    return float(e.abs().max()), float(e.pow(2).mean().sqrt())


def check(g, w, dt, h, wd):
    g = U.rounded(g, dt)
    w = U.rounded(w, dt)          # both paths multiply with the weights rounded to dt
    ref = ref_f64(g, w, h, wd)
    new, old = upadj(g, w, dt, h, wd), two_launch(g, w, dt, h, wd)
    assert torch.isfinite(new).all() and torch.isfinite(old).all()
    (mn, rn), (mo, ro) = errs(new, ref), errs(old, ref)
    # both paths end with the same rounding of d_a to dt, worth up to half an ulp of max|d_a| in EITHER path's maximum: the
    # maximum gets that much slack on top of the 1.25x, the RMS (over every element) none
    half_ulp = 0.5 * float(torch.finfo(U.tdt(dt)).eps) * 2.0 ** torch.frexp(ref.abs().max()).exponent.item() / 2.0
    floor = 1e-6 * float(ref.abs().max())
    assert mn <= 1.25 * mo + half_ulp, (mn, mo, half_ulp)
    assert rn <= 1.25 * ro + floor, (rn, ro)
    assert U.relerr(new, ref) <= 2e-2


def rnd(*shape, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=gen) * scale


# (N, h, w) at low resolution: partial 8 x 16 tiles on both axes, image edges on every side, odd sizes, several tiles
SHAPES = [(1, 16, 24), (1, 20, 20), (2, 128, 128), (1, 13, 21), (2, 5, 7), (1, 9, 33)]


CASES = [(f, s) for f in (16, 32, 64) for s in SHAPES if f == 64 or s[1] < 128]   # the full-size case at the headline width


@pytest.mark.parametrize("dt", [L.BF16, L.F16])
@pytest.mark.parametrize("f,shape", CASES)
def test_upadj_vs_f64(dt, f, shape):
    n, h, wd = shape
    g = rnd(n, f // 2, 2 * h, 2 * wd, seed=11 + h)
    w = rnd(f // 2, f, 3, 3, seed=12 + f, scale=(2.0 / (9 * f)) ** 0.5)
    check(g, w, dt, h, wd)


def test_upadj_fp16_large_magnitude():
    """fp16 near the top of its range: g scaled so that the reference's high-resolution input gradient and d_a both reach
    half of the fp16 maximum.  h (bounded by 4 max|g|) must not overflow where the two-launch path does not."""
    n, h, wd, f = 1, 24, 40, 64
    g = rnd(n, f // 2, 2 * h, 2 * wd, seed=21)
    w = rnd(f // 2, f, 3, 3, seed=22, scale=(2.0 / (9 * f)) ** 0.5)
    wr = U.rounded(w, L.F16).double()
    dx = F.conv_transpose2d(g.double(), wr, padding=1)
    da = ref_f64(g, w, h, wd)
    s = 0.5 * 65504.0 / max(float(dx.abs().max()), float(da.abs().max()))
    check(g * s, w, L.F16, h, wd)


def test_upadj_declines_other_widths():
    """fp32, C5's 64 -> 128 and non-3x3 shapes have no W^T image: the engine keeps the two-launch path for them."""
    lib = L.load()
    assert lib.mrisr_packed_weight_bytes_upadj(L.F32, 32, 64, 3) == 0
    assert lib.mrisr_packed_weight_bytes_upadj(L.BF16, 64, 128, 3) == 0
    assert lib.mrisr_packed_weight_bytes_upadj(L.BF16, 32, 64, 1) == 0
    assert lib.mrisr_packed_weight_bytes_upadj(L.BF16, 32, 64, 3) > 0
