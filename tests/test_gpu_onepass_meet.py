"""csrc/norm_bwd_onepass.hip, onepass_meet: what crosses the image barrier of the one-pass GroupNorm + LeakyReLU backward.
Every block adds its gamma-weighted GROUP sums into the image's table behind the barrier words and reads only that table
after the barrier; the per-channel sums in red[] are turned into dgamma / dbeta by the block that completes the image's count.

Smallest shapes at which that meeting can go wrong: C = 8 with one group (one channel vector per pixel), C = 16, C = 64 and
C = 512 with the network's 8 groups; 1, 2, 16, 17 (uneven membership of the 16 block groups) and more than 32 blocks per
image; N = 1 and N = 3 (image tables and slots must not alias); one and two plain consumers, one of them a channel window of
a wider tensor; the window kernel with and without a plain consumer, with a tail block.  gamma of mixed sign with one exact
zero per group, x and upstream gradients of non-zero mean that follow xhat (normbwdutil.make_case's recipe), so that the mean
terms x B + C are as large as g A.

Reference: float64 on the host.  Bounds (tests/test_gpu_blend_bwd.py's convention): dx - RMS and maximum error within 1.25x
of the two-pass kernels' (mrisr_act_bwd_reduce + mrisr_act_bwd_apply_fused) on the same inputs, plus half an output ulp on
the maximum; dgamma / dbeta - within 1.5x of theirs plus the fp32 summation bound.  dgamma / dbeta start from non-zero values
and every case is launched twice on fresh red / arrive: the expected value is start + 2 x the share, so an image's share
added twice, or not at all, is off by the share itself.  Every test prints its margins."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hiputil as U
from mri_superresolution_amd import _lib as L

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
SLOPE = 0.2
WIDER = 16           # channels a windowed consumer's tensor has beyond the node's (the node sits at c_off = 8)

# (C, groups, N, H, W, consumers) - consumers: "p" plain of the node's own tensor shape, "P" plain channel window of a wider
# tensor, "w" the 2x2 pool.  Blocks per image: plain kernel (256 / (C / 8)) * 8 pixels, window kernel (256 / (C / 8)) * 2 windows.
CASES = [
    (8, 1, 1, 16, 16, "p"),        # 1 block of 2048 pixels, mostly empty: no partner
    (8, 1, 3, 64, 48, "pP"),       # 2 blocks
    (8, 1, 3, 20, 12, "w"),        # window kernel, one tail block
    (16, 8, 1, 32, 32, "pP"),      # 1 block, exactly full
    (16, 8, 3, 136, 128, "P"),     # 17 blocks
    (16, 8, 3, 48, 40, "wP"),      # window kernel, 480 windows of 256 per block: 2 blocks, the second a tail
    (64, 8, 1, 16, 16, "pP"),      # 1 block
    (64, 8, 3, 32, 16, "P"),       # 2 blocks
    (64, 8, 3, 64, 64, "pP"),      # 16 blocks: every block group has one member
    (64, 8, 3, 68, 64, "p"),       # 17 blocks: group 0 has two members
    (64, 8, 1, 96, 96, "Pp"),      # 36 blocks
    (64, 8, 3, 16, 16, "w"),       # window kernel, 1 block
    (64, 8, 1, 20, 12, "wP"),      # 60 windows of 64: one tail block
    (64, 8, 3, 36, 20, "Pw"),      # 180 windows: 3 blocks, the last a tail; the pool is the second consumer
    (64, 8, 1, 72, 64, "w"),       # 18 blocks
    (64, 8, 1, 96, 96, "wP"),      # 36 blocks
    (512, 8, 3, 8, 8, "p"),        # 64 vectors, 4 pixel lanes: 2 blocks
    (512, 8, 1, 24, 24, "pP"),     # 18 blocks
    (512, 8, 1, 16, 16, "wP"),     # 8 windows per block: 8 blocks
]
IDS = [f"C{c}g{g}_N{n}_{h}x{w}_{k}" for c, g, n, h, w, k in CASES]
DTS = [L.BF16, L.F16]


def _blocks(c, h, w, kinds):
    lanes = 256 // (c // 8)
    return -(-(h * w // 4) // (lanes * 2)) if "w" in kinds else -(-(h * w) // (lanes * 8))


def test_case_list_covers_the_block_counts():
    plain = {_blocks(c, h, w, k) for c, g, n, h, w, k in CASES if "w" not in k}
    window = {_blocks(c, h, w, k) for c, g, n, h, w, k in CASES if "w" in k}
    assert {1, 2, 16, 17} <= plain and max(plain) > 32 and {1, 2} <= window and max(window) > 32


class Case:
    """Inputs on the host (float64 tensors of storage-rounded values, NCHW) and on the device."""

    def __init__(self, dt, c, groups, n, h, w, kinds, seed):
        self.dt, self.shape, self.groups, self.kinds = dt, (n, c, h, w), groups, kinds
        gen = torch.Generator().manual_seed(seed)
        r = lambda v: U.rounded(v.float(), dt).double()                                  # noqa: E731
        randn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)           # noqa: E731
        gs = c // groups
        x = r(1.5 * randn(n, c, h, w) + 0.7)
        sign = torch.where(torch.rand(c, generator=gen) < 0.5, -1.0, 1.0).double()
        sign[0::2 * gs] = 1.0                       # both signs in the layer whatever the draw
        if c > gs:
            sign[gs::2 * gs] = -1.0
        elif gs > 2:
            sign[2] = -1.0
        gamma = (sign * (0.8 + 0.7 * torch.rand(c, generator=gen, dtype=torch.float64))).float()
        gamma[1 % gs::gs] = 0.0                     # one exact zero per group
        beta = (0.1 * randn(c)).float()
        xg = x.view(n, groups, -1)
        mean = xg.mean(2).float()
        rstd = (1.0 / torch.sqrt(xg.var(2, unbiased=False) + 1e-5)).float()
        pc = lambda v: v.repeat_interleave(gs, 1)                                         # noqa: E731  (N, G) -> (N, C)
        scale = gamma.view(1, c) * pc(rstd)                                               # float32, as mrisr_gn_finalize forms them
        shift = beta.view(1, c) - pc(mean) * scale
        self.x, self.gamma, self.mean, self.rstd, self.scale, self.shift = x, gamma.double(), mean.double(), rstd.double(), scale.double(), shift.double()
        self.count = float(gs * h * w)
        xhat = (x - pc(self.mean)[:, :, None, None]) * pc(self.rstd)[:, :, None, None]
        s = torch.where(gamma < 0, -1.0, 1.0).double().view(1, c, 1, 1)
        self.cons = []                              # (kind, da NCHW float64, c_off)
        for k in kinds:
            if k == "w":
                far = (s * (0.5 + 2.25 * torch.tanh(xhat)))
                self.cons.append(("w", r(4.0 * F.avg_pool2d(far, 2) + 0.5 * randn(n, c, h // 2, w // 2)), 0))
            else:
                coff, extra = (8, WIDER) if k == "P" else (0, 0)
                da = 0.5 * randn(n, c + extra, h, w)
                da[:, coff:coff + c] += s * (1.5 + 2.25 * torch.tanh(xhat))
                self.cons.append(("p", r(da), coff))
        # ---- device operands
        self.xd = U.nhwc(x.float(), dt)
        self.keep = [U.nhwc(da.float(), dt) for _, da, _ in self.cons]
        self.carr = (L.Consumer * 2)()
        for e, (kind, da, coff), dd in zip(self.carr, self.cons, self.keep):
            e.da, e.C_total, e.c_off, e.H, e.W = dd.data_ptr(), da.shape[1], coff, da.shape[2], da.shape[3]
            e.spatial, e.off_y, e.off_x, e.weight_mode = (L.SP_POOL2 if kind == "w" else L.SP_NONE), 0, 0, 0
        dev = lambda v: v.float().contiguous().to(U.DEV)                                  # noqa: E731
        self.scaled, self.shiftd, self.gammad = dev(scale.reshape(-1)), dev(shift.reshape(-1)), dev(gamma)
        self.mrd = dev(torch.stack([mean, rstd], -1).reshape(-1))
        self.start = [0.75 + 0.01 * torch.arange(c, dtype=torch.float32), -1.25 + 0.02 * torch.arange(c, dtype=torch.float32)]      # dgamma, dbeta


def reference(k: Case):
    """float64: dx, one launch's share of dgamma / dbeta, and the fp32 summation bound n_terms 2^-24 sum |terms| of either."""
    n, c, h, w = k.shape
    gs = c // k.groups
    b = lambda v: v.repeat_interleave(gs, 1)[:, :, None, None]                            # noqa: E731
    mean, rstd = b(k.mean), b(k.rstd)
    pre = k.x * k.scale[:, :, None, None] + k.shift[:, :, None, None]
    gact = torch.zeros_like(k.x)
    for kind, da, coff in k.cons:
        if kind == "w":
            act = torch.where(pre > 0, pre, SLOPE * pre)
            _, idx = F.max_pool2d(act, 2, return_indices=True)            # aten: the first maximum in scan order
            gact += torch.zeros(n, c, h * w, dtype=torch.float64).scatter_(2, idx.view(n, c, -1), da.reshape(n, c, -1)).view(n, c, h, w)
        else:
            gact += da[:, coff:coff + c]
    g = gact * torch.where(pre > 0, 1.0, SLOPE)
    xhat = (k.x - mean) * rstd
    gam = k.gamma.view(1, c, 1, 1)
    grp = lambda v: v.reshape(n, k.groups, -1).sum(2) / k.count                          # noqa: E731
    S1, S2 = b(grp(g * gam)), b(grp(g * gam * xhat))
    dx = g * (rstd * gam) + k.x * (-rstd * rstd * S2) + (mean * rstd * rstd * S2 - rstd * S1)
    nt = n * h * w
    return dict(dx=dx, dbeta=g.sum((0, 2, 3)), dgamma=(g * xhat).sum((0, 2, 3)),
                dbeta_b=nt * EPS32 * g.abs().sum((0, 2, 3)),
                dgamma_b=nt * EPS32 * (rstd * g.abs() * (k.x.abs() + mean.abs())).sum((0, 2, 3)))      # the kernels sum g x and mean g


def launch_twice(k: Case, onepass: bool):
    """Two launches of the node's backward on fresh red / arrive, accumulating into ONE pair of pre-filled dgamma / dbeta."""
    n, c, h, w = k.shape
    lib = L.load()
    kind = 2 if "w" in k.kinds else 1
    ncons = len(k.cons)
    dgamma, dbeta = k.start[0].to(U.DEV), k.start[1].to(U.DEV)
    dxs = []
    for _ in range(2):
        dx = torch.full_like(k.xd, float("nan"))
        if onepass:
            assert lib.mrisr_act_bwd_onepass_ok(k.dt, ncons, k.carr, n, h, w, c) == kind
            red = torch.zeros(n * c * 2 * lib.mrisr_act_bwd_onepass_slots(), device=U.DEV)
            arrive = torch.zeros(n * lib.mrisr_act_bwd_onepass_barrier_words(), dtype=torch.int32, device=U.DEV)
        else:
            red = torch.zeros(n * c * 2, device=U.DEV)
        fin = L.GnBwdFin(red.data_ptr(), k.gammad.data_ptr(), k.mrd.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), None, None, None,
                         k.count, 0.0, k.groups)
        if onepass:
            L.call("mrisr_act_bwd_onepass", k.dt, k.xd.data_ptr(), k.scaled.data_ptr(), k.shiftd.data_ptr(), k.mrd.data_ptr(), ncons, k.carr,
                   red.data_ptr(), arrive.data_ptr(), C.byref(fin), dx.data_ptr(), n, h, w, c, U.stream())
        else:
            L.call("mrisr_act_bwd_reduce", k.dt, k.xd.data_ptr(), k.scaled.data_ptr(), k.shiftd.data_ptr(), k.mrd.data_ptr(), ncons, k.carr,
                   None, None, red.data_ptr(), None, n, h, w, c, k.groups, U.stream())
            L.call("mrisr_act_bwd_apply_fused", k.dt, k.xd.data_ptr(), k.scaled.data_ptr(), k.shiftd.data_ptr(), ncons, k.carr, None,
                   None, C.byref(fin), dx.data_ptr(), n, h, w, c, U.stream())
        torch.cuda.synchronize()
        if onepass:       # everybody was counted, once
            words = arrive.cpu().view(n, -1)
            blocks = _blocks(c, h, w, k.kinds)
            assert (words[:, 0:256:16].sum(1) == blocks).all() and (words[:, 256] == min(blocks, 16)).all()
        dxs.append(U.nchw(dx).double())
    return dxs, dgamma.cpu().double(), dbeta.cpu().double()


def errs(got, ref):
    e = got - ref
    return float(e.abs().max()), float(e.pow(2).mean().sqrt())


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_onepass_meet_vs_f64_and_two_pass(case, dt):
    c, groups, n, h, w, kinds = case
    k = Case(dt, c, groups, n, h, w, kinds, seed=100 + CASES.index(case))
    ref = reference(k)
    (new1, new2), dg_new, db_new = launch_twice(k, True)
    (old1, _), dg_old, db_old = launch_twice(k, False)
    tag = f"{IDS[CASES.index(case)]} {'bf16' if dt == L.BF16 else 'fp16'} ({_blocks(c, h, w, kinds)} blocks per image)"
    eps = float(torch.finfo(U.tdt(dt)).eps)
    half_ulp = 0.5 * eps * 2.0 ** torch.frexp(ref["dx"].abs().max()).exponent.item() / 2.0
    (mo, ro) = errs(old1, ref["dx"])
    for i, dxn in enumerate((new1, new2)):
        assert torch.isfinite(dxn).all(), "a block gave up waiting at the image barrier"
        (mn, rn) = errs(dxn, ref["dx"])
        print(f"{tag} dx launch {i}: max err one-pass {mn:.3e} two-pass {mo:.3e} (+{half_ulp:.1e}), rms one-pass {rn:.3e} two-pass {ro:.3e}, "
              f"|ref| max {float(ref['dx'].abs().max()):.3e}")
        assert mn <= 1.25 * mo + half_ulp, (mn, mo, half_ulp)
        assert rn <= 1.25 * ro, (rn, ro)
    for name, vn, vo, start in (("dgamma", dg_new, dg_old, k.start[0].double()), ("dbeta", db_new, db_old, k.start[1].double())):
        want = start + 2.0 * ref[name]
        # two launches' sums, and the two float32 additions into the running value
        bound = 2.0 * ref[name + "_b"] + 2.0 * 2.0 ** -24 * (start.abs() + 2.0 * ref[name].abs())
        en, eo = (vn - want).abs(), (vo - want).abs()
        print(f"{tag} {name}: worst err one-pass {float(en.max()):.3e} two-pass {float(eo.max()):.3e}, fp32 summation bound "
              f"{float(bound.min()):.3e} .. {float(bound.max()):.3e}, smallest |share| {float(ref[name].abs().min()):.3e}")
        assert torch.isfinite(vn).all()
        assert bool((en <= 1.5 * eo + bound).all()), (name, en.max(), eo.max(), bound.max())
