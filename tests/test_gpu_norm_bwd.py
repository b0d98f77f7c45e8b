"""csrc/norm_bwd*.hip: every launch sequence of the GroupNorm + LeakyReLU backward against the float64 specification of normbwdutil
under its DERIVED bounds (store rounding, float32 evaluation, float32 summation - see that module's docstring), on inputs under
which the mean terms x B + C are as large as g A: upstream gradients of non-zero mean that follow xhat, gamma of mixed sign and
exactly zero, 2x2 windows with tied maxima, and pre exactly zero.  test_norm_bwd_host.py proves on the same inputs that a
kernel without B or C, with another group's sums, with the wrong tie or kink rule... lands outside these bounds.
Every test prints, per output, the worst ratio of error to bound."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hiputil as U
import normbwdutil as NB
from mri_superresolution_amd import _lib as L

pytestmark = pytest.mark.gpu

G = NB.G
DTS = [L.F32, L.BF16, L.F16]
DT16 = [L.BF16, L.F16]
IDS = lambda dts: [NB.DTNAME[d] for d in dts]       # noqa: E731
TAGS = ["", "ties_", "kink_"]
_CASES = {}


def get_case(dt, name):
    if dt not in _CASES:
        _CASES[dt] = {k.name: k for k in NB.case_list(dt)}
    return _CASES[dt][name]


def other_cases(dt, build):
    if (dt, build) not in _CASES:
        _CASES[(dt, build)] = build(dt)
    return _CASES[(dt, build)]


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def forward_state(k: NB.Case):
    """mrisr_gn_finalize on the device from exact float64 sums of x - or, for a kink case, from the handed statistics
    (sum 0, sum of squares = count).  Returns (scale, shift, meanrstd) on the device and (mean, rstd) as float64 arrays."""
    n, c, h, w = k.shape
    stats = torch.zeros(L.STAT_SLOTS, n, G, 2, dtype=torch.float64)
    if k.kink:
        stats[3, :, :, 1] = k.count
    else:
        xg = torch.from_numpy(k.x).view(n, G, -1)
        stats[3] = torch.stack([xg.sum(2), (xg * xg).sum(2)], -1)
    stats = stats.contiguous().to(U.DEV)
    scale, shift, mr = torch.empty(n * c, device=U.DEV), torch.empty(n * c, device=U.DEV), torch.empty(n * G * 2, device=U.DEV)
    gd, bd = t32(k.gamma).to(U.DEV), t32(k.beta).to(U.DEV)
    L.call("mrisr_gn_finalize", stats.data_ptr(), gd.data_ptr(), bd.data_ptr(), scale.data_ptr(), shift.data_ptr(), mr.data_ptr(),
           n, c, G, k.count, 1e-5, U.stream())
    torch.cuda.synchronize()
    got = mr.cpu().double().view(n, G, 2).numpy()
    want = k.stats32()
    for i in range(2):      # the statistics themselves are checked elsewhere; here: what the specification is handed is what they are
        assert np.abs(got[..., i] - want[i]).max() <= 2.0 ** -22 * max(np.abs(want[i]).max(), 1e-30) + (1e-30 if k.kink else 0)
    return scale, shift, mr, (got[..., 0].copy(), got[..., 1].copy())


class Launch:
    """Device operands of one case."""

    def __init__(self, k: NB.Case, ref0=None):
        self.k, dt = k, k.dt
        n, c, h, w = k.shape
        self.scale, self.shift, self.mr, self.meanrstd = forward_state(k)
        self.xd = U.nhwc(t32(k.x), dt)
        self.gammad = t32(k.gamma).to(U.DEV)
        self.ad = torch.tensor([k.alpha if k.alpha is not None else 0.0], device=U.DEV)
        self.keep, self.carr = [], (L.Consumer * 2)()
        self.head = None
        for i, q in enumerate(k.cons):
            e = self.carr[i]
            if q.kind == "head":
                dd = t32(q.da).to(U.DEV).contiguous()
                out = t32(ref0["head_out"]).to(U.DEV).contiguous()
                hw = t32(q.head_w).to(U.DEV)
                self.head = dict(part=torch.zeros(n * (c + 1), device=U.DEV), dw=torch.zeros(c, device=U.DEV), db=torch.zeros(1, device=U.DEV))
                e.da, e.C_total, e.c_off, e.H, e.W, e.spatial, e.weight_mode = dd.data_ptr(), c, 0, h, w, L.SP_HEAD, 0
                e.head_out, e.head_w, e.head_part = out.data_ptr(), hw.data_ptr(), self.head["part"].data_ptr()
                e.head_dw, e.head_db = self.head["dw"].data_ptr(), self.head["db"].data_ptr()
                self.keep += [dd, out, hw]
                continue
            dd = U.nhwc(t32(q.da), dt)
            self.keep.append(dd)
            e.da, e.C_total, e.c_off, e.H, e.W = dd.data_ptr(), q.da.shape[1], q.c_off, q.da.shape[2], q.da.shape[3]
            e.spatial = {"plain": L.SP_NONE, "pool": L.SP_POOL2, "up": L.SP_UP2}[q.kind]
            e.off_y, e.off_x, e.weight_mode = q.off[0], q.off[1], q.wm
        self.ncons = len(k.cons)
        self.blend = self.ad.data_ptr() if any(q.wm for q in k.cons) else None

    def buffers(self, slots=1):
        n, c, h, w = self.k.shape
        z = lambda m: torch.zeros(m, device=U.DEV)       # noqa: E731
        b = dict(red=z(n * c * 2 * slots + 256), dgamma=z(c), dbeta=z(c), dalpha=z(1), dbias=z(4 * c), coef=torch.empty(3 * n * c, device=U.DEV),
                 dx=torch.full_like(self.xd, float("nan")))
        b["slots"] = b["red"][n * c * 2 * slots:]
        return b

    def fin(self, b, with_alpha=False):
        sgn = {1: 1.0, 2: -1.0}.get(self.k.cons[0].wm, 0.0)
        return L.GnBwdFin(b["red"].data_ptr(), self.gammad.data_ptr(), self.mr.data_ptr(), b["dgamma"].data_ptr(), b["dbeta"].data_ptr(),
                          b["slots"].data_ptr() if with_alpha else None, self.ad.data_ptr() if with_alpha else None,
                          b["dalpha"].data_ptr() if with_alpha else None, self.k.count, sgn, G)

    def results(self, b, dx=None, **more):
        r = dict(dx=U.nchw(b["dx"] if dx is None else dx).double().numpy(), dgamma=b["dgamma"].cpu().double().numpy(),
                 dbeta=b["dbeta"].cpu().double().numpy())
        if self.head is not None:
            r["head_dw"], r["head_db"] = self.head["dw"].cpu().double().numpy(), self.head["db"].cpu().double().numpy()
        r.update(more)
        return r


def run_g_apply(la: Launch, shuffled=False):
    """mrisr_act_bwd_reduce with g stored + mrisr_act_bwd_finalize + mrisr_act_bwd_apply."""
    k, dt = la.k, la.k.dt
    n, c, h, w = k.shape
    b = la.buffers()
    g = torch.full_like(la.xd, float("nan"))
    L.call("mrisr_act_bwd_reduce", dt, la.xd.data_ptr(), la.scale.data_ptr(), la.shift.data_ptr(), la.mr.data_ptr(), la.ncons, la.carr,
           la.blend, g.data_ptr(), b["red"].data_ptr(), None, n, h, w, c, G, U.stream())
    L.call("mrisr_act_bwd_finalize", b["red"].data_ptr(), la.gammad.data_ptr(), la.mr.data_ptr(), b["dgamma"].data_ptr(), b["dbeta"].data_ptr(),
           b["coef"].data_ptr(), n, c, G, k.count, None, None, None, 0.0, U.stream())
    more = {}
    if shuffled:
        dxs = torch.full((n, h // 2, w // 2, 4 * c), float("nan"), dtype=U.tdt(dt), device=U.DEV)
        L.call("mrisr_act_bwd_apply", dt, la.xd.data_ptr(), g.data_ptr(), b["coef"].data_ptr(), dxs.data_ptr(), n, h, w, c,
               L.OUT_PIXEL_SHUFFLE2, b["dbias"].data_ptr(), U.stream())
        torch.cuda.synchronize()
        dx = F.pixel_shuffle(U.nchw(dxs), 2).double().numpy()
        more["dbias"] = b["dbias"].cpu().double().numpy()
    else:
        L.call("mrisr_act_bwd_apply", dt, la.xd.data_ptr(), g.data_ptr(), b["coef"].data_ptr(), b["dx"].data_ptr(), n, h, w, c,
               L.OUT_PLAIN, None, U.stream())
        torch.cuda.synchronize()
        dx = U.nchw(b["dx"]).double().numpy()
    r = la.results(b, g=U.nchw(g).double().numpy(), **more)
    r["dx"] = dx
    return r


def run_fused(la: Launch, in_kernel=True):
    """mrisr_act_bwd_reduce with g = NULL + mrisr_act_bwd_apply_fused, coefficients from mrisr_act_bwd_finalize or in the kernel."""
    k, dt = la.k, la.k.dt
    n, c, h, w = k.shape
    b = la.buffers()
    L.call("mrisr_act_bwd_reduce", dt, la.xd.data_ptr(), la.scale.data_ptr(), la.shift.data_ptr(), la.mr.data_ptr(), la.ncons, la.carr,
           la.blend, None, b["red"].data_ptr(), None, n, h, w, c, G, U.stream())
    if in_kernel:
        fin = la.fin(b)
        L.call("mrisr_act_bwd_apply_fused", dt, la.xd.data_ptr(), la.scale.data_ptr(), la.shift.data_ptr(), la.ncons, la.carr, la.blend,
               None, C.byref(fin), b["dx"].data_ptr(), n, h, w, c, U.stream())
    else:
        L.call("mrisr_act_bwd_finalize", b["red"].data_ptr(), la.gammad.data_ptr(), la.mr.data_ptr(), b["dgamma"].data_ptr(),
               b["dbeta"].data_ptr(), b["coef"].data_ptr(), n, c, G, k.count, None, None, None, 0.0, U.stream())
        L.call("mrisr_act_bwd_apply_fused", dt, la.xd.data_ptr(), la.scale.data_ptr(), la.shift.data_ptr(), la.ncons, la.carr, la.blend,
               b["coef"].data_ptr(), None, b["dx"].data_ptr(), n, h, w, c, U.stream())
    torch.cuda.synchronize()
    return la.results(b)


def run_onepass(la: Launch, kind):
    k, dt = la.k, la.k.dt
    n, c, h, w = k.shape
    lib = L.load()
    assert lib.mrisr_act_bwd_onepass_ok(dt, la.ncons, la.carr, n, h, w, c) == kind
    slots = lib.mrisr_act_bwd_onepass_slots()
    b = la.buffers(slots)
    arrive = torch.zeros(n * lib.mrisr_act_bwd_onepass_barrier_words(), dtype=torch.int32, device=U.DEV)
    fin = la.fin(b)
    L.call("mrisr_act_bwd_onepass", dt, la.xd.data_ptr(), la.scale.data_ptr(), la.shift.data_ptr(), la.mr.data_ptr(), la.ncons, la.carr,
           b["red"].data_ptr(), arrive.data_ptr(), C.byref(fin), b["dx"].data_ptr(), n, h, w, c, U.stream())
    torch.cuda.synchronize()
    r = la.results(b)
    assert np.isfinite(r["dx"]).all(), "a block gave up waiting at the image barrier"
    nvec = c // 8
    blocks = -(-(h * w // 4) // ((256 // nvec) * 2)) if kind == 2 else -(-(h * w) // ((256 // nvec) * 8))
    words = arrive.cpu().view(n, -1)
    assert (words[:, 0:256:16].sum(1) == blocks).all() and (words[:, 256] == min(blocks, 16)).all()     # everybody was counted
    return r, blocks


def run_unshuffle(la: Launch):
    """mrisr_act_bwd_reduce with g = NULL + mrisr_act_bwd_apply_fused_unshuffle (dbias; dalpha when the consumer is weighted)."""
    k, dt = la.k, la.k.dt
    n, c, h, w = k.shape
    b = la.buffers()
    wa = la.blend is not None
    L.call("mrisr_act_bwd_reduce", dt, la.xd.data_ptr(), la.scale.data_ptr(), la.shift.data_ptr(), la.mr.data_ptr(), 1, la.carr,
           la.blend, None, b["red"].data_ptr(), b["slots"].data_ptr() if wa else None, n, h, w, c, G, U.stream())
    fin = la.fin(b, with_alpha=wa)
    dxs = torch.full((n, h // 2, w // 2, 4 * c), float("nan"), dtype=U.tdt(dt), device=U.DEV)
    L.call("mrisr_act_bwd_apply_fused_unshuffle", dt, la.xd.data_ptr(), la.scale.data_ptr(), la.shift.data_ptr(), la.carr, la.blend,
           C.byref(fin), dxs.data_ptr(), b["dbias"].data_ptr(), n, h, w, c, U.stream())
    torch.cuda.synchronize()
    more = dict(dbias=b["dbias"].cpu().double().numpy())
    if wa:
        more["dalpha"] = b["dalpha"].cpu().double().numpy()
    r = la.results(b, **more)
    r["dx"] = F.pixel_shuffle(U.nchw(dxs), 2).double().numpy()
    return r


def check(tag, out, ref, k=None):
    """Every output inside its bound.  With a pooled ties or kink case ``k`` (pooled gradients of magnitude >= 0.5) in which
    nothing is left out: the set of elements that take the pooled gradient equals the specification's exactly, read off the
    stored g or else off dx (normbwdutil.routing_sets).  The random cases are not checked this way: their pooled gradients
    come arbitrarily close to 0, where the set cannot be read off the result; there the per-element bound stands alone."""
    r = NB.ratios(out, ref)
    if "g" in out:
        r["g"] = NB.worst_ratio(out["g"], ref["g"], ref["g_b"], ~ref["excluded"])
    line = f"{tag}: error / bound " + ", ".join(f"{n} {v:.3f}" for n, v in r.items())
    sets = None
    if k is not None and k.pooled and (k.ties or k.kink) and not ref["excluded"].any():
        sets = NB.routing_sets(out, ref)
        line += f", routing read off {'g' if 'g' in out else 'dx'} on {sets[2].mean():.3f} of the elements"
    print(line)
    assert all(v <= 1.0 for v in r.values()), (tag, r)
    if sets is not None:
        got, want, live = sets
        assert live.mean() >= 0.75, (tag, live.mean())
        assert np.array_equal(got, want), (tag, int((got != want).sum()))
    return r


_SPECS = {}


def spec_for(la: Launch, **kw):
    k = la.k
    key = (k.name, k.dt, k.shape, tuple(sorted(kw.items())), la.meanrstd[0].tobytes(), la.meanrstd[1].tobytes())
    if key in _SPECS:
        return _SPECS[key]
    ref = _SPECS[key] = NB.spec(k, la.meanrstd, **kw)
    return ref


def head_out_of(k):
    return NB.spec(k, k.stats32())


# ------------------------------------------------------------------------------------------------ reduce (g) + finalize + apply
@pytest.mark.parametrize("dt", DTS, ids=IDS(DTS))
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", ["pad_A", "pad+pool_A", "up_A", "pad+pool_B"])
def test_reduce_g_finalize_apply(name, tag, dt):
    k = get_case(dt, tag + name)
    la = Launch(k)
    ref = spec_for(la, stores_g=True)
    check(f"{NB.DTNAME[dt]} {k.name} plain", run_g_apply(la), ref, k)
    if name == "pad_A":
        ref = spec_for(la, stores_g=True, shuffled=True)
        check(f"{NB.DTNAME[dt]} {k.name} pixel-shuffled", run_g_apply(la, shuffled=True), ref)


# ------------------------------------------------------------------------------------------------ reduce (g NULL) + apply_fused
@pytest.mark.parametrize("dt", DTS, ids=IDS(DTS))
@pytest.mark.parametrize("in_kernel", [False, True])
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", ["same_A", "same2_A", "pad_A", "pool_A", "pool+skip_A", "same_T", "pool_T"])
def test_reduce_apply_fused(name, tag, in_kernel, dt):
    k = get_case(dt, tag + name)
    la = Launch(k)
    ref = spec_for(la)
    check(f"{NB.DTNAME[dt]} {k.name} {'GnBwdFin' if in_kernel else 'finalize'}", run_fused(la, in_kernel), ref, k)


@pytest.mark.parametrize("dt", DTS, ids=IDS(DTS))
@pytest.mark.parametrize("tag", ["", "kink_"])
@pytest.mark.parametrize("name", ["head_A", "head_H"])
def test_head_consumer(name, tag, dt):
    k = get_case(dt, tag + name)
    la = Launch(k, head_out_of(k))
    check(f"{NB.DTNAME[dt]} {k.name}", run_fused(la, True), spec_for(la))


# ------------------------------------------------------------------------------------------------ one pass
@pytest.mark.parametrize("dt", DT16, ids=IDS(DT16))
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name,kind,blocks", [("same_P", 1, 1), ("same_B", 1, 2), ("same2_A", 1, 1), ("pool+skip_A", 2, 1), ("pool_A", 2, 1),
                                              ("same_O", 1, 9), ("pool+skip_O", 2, 9)])
def test_onepass(name, kind, blocks, tag, dt):
    k = get_case(dt, tag + name)
    la = Launch(k)
    out, nblk = run_onepass(la, kind)
    assert nblk >= blocks
    check(f"{NB.DTNAME[dt]} {k.name} onepass ({nblk} blocks per image)", out, spec_for(la), k)


# ------------------------------------------------------------------------------------------------ pixel-shuffled producer
@pytest.mark.parametrize("dt", DTS, ids=IDS(DTS))
@pytest.mark.parametrize("tag", ["", "kink_"])
@pytest.mark.parametrize("shape,wm", NB.UNSHUFFLE)
def test_apply_fused_unshuffle(shape, wm, tag, dt):
    k = other_cases(dt, NB.unshuffle_cases)[(shape, wm, tag)]
    la = Launch(k)
    ref = spec_for(la, shuffled=True)
    check(f"{NB.DTNAME[dt]} {k.name}", run_unshuffle(la), ref)


# ------------------------------------------------------------------------------------------------ the blend pair
@pytest.mark.parametrize("dt", DT16, ids=IDS(DT16))
@pytest.mark.parametrize("alpha", [0.0, 1.5])
@pytest.mark.parametrize("kink", [False, True])
@pytest.mark.parametrize("c,hw", NB.BLEND_SHAPES)
def test_blend_pair_against_the_specification(c, hw, kink, alpha, dt):
    br = other_cases(dt, NB.blend_cases)[(c, hw, alpha, kink)]
    las = [Launch(b) for b in br]
    n, h, w = 2, hw[0], hw[1]
    bufs = [la.buffers() for la in las]
    gd = las[0].keep[0]
    ad = las[0].ad
    bb = [L.BlendBranch(la.xd.data_ptr(), la.scale.data_ptr(), la.shift.data_ptr(), la.mr.data_ptr(), b["red"].data_ptr(), b["slots"].data_ptr(),
                        la.k.cons[0].wm, 0) for la, b in zip(las, bufs)]
    L.call("mrisr_act_bwd_blend_reduce", dt, gd.data_ptr(), C.byref(bb[0]), C.byref(bb[1]), ad.data_ptr(), n, h, w, c, G, U.stream())
    dalpha = torch.zeros(1, device=U.DEV)
    fins = []
    for la, b in zip(las, bufs):
        b["dalpha"] = dalpha
        la.ad = ad
        fins.append(la.fin(b, with_alpha=True))
    dx_ps = torch.full((n, h // 2, w // 2, 4 * c), float("nan"), dtype=U.tdt(dt), device=U.DEV)
    L.call("mrisr_act_bwd_blend_apply", dt, gd.data_ptr(), C.byref(bb[0]), C.byref(bb[1]), ad.data_ptr(), C.byref(fins[0]), C.byref(fins[1]),
           dx_ps.data_ptr(), bufs[1]["dx"].data_ptr(), bufs[0]["dbias"].data_ptr(), n, h, w, c, U.stream())
    torch.cuda.synchronize()
    refs = [spec_for(las[0], shuffled=True), spec_for(las[1])]
    out0 = las[0].results(bufs[0], dbias=bufs[0]["dbias"].cpu().double().numpy())
    out0["dx"] = F.pixel_shuffle(U.nchw(dx_ps), 2).double().numpy()
    check(f"{NB.DTNAME[dt]} {br[0].name}", out0, refs[0])
    check(f"{NB.DTNAME[dt]} {br[1].name}", las[1].results(bufs[1]), refs[1])
    both = dict(dalpha=refs[0]["dalpha"] + refs[1]["dalpha"], dalpha_b=refs[0]["dalpha_b"] + refs[1]["dalpha_b"])
    ratio = NB.worst_ratio(dalpha.cpu().double().numpy(), both["dalpha"], both["dalpha_b"])
    print(f"{NB.DTNAME[dt]} {br[0].name} dalpha: error / bound {ratio:.3f}")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ forward side of gamma <= 0
@pytest.mark.parametrize("dt", DTS, ids=IDS(DTS))
@pytest.mark.parametrize("shape", NB.FORWARD_SHAPES)
def test_forward_pool_and_upsample_with_negative_and_zero_gamma(shape, dt):
    """mrisr_norm_pool2, the convolution's SP_POOL2 loader (3x3 weights that are the identity at the centre tap;
    the library has no 1x1 convolution of a pooled source) and mrisr_norm_upsample2 on the ties case:
    the pool is taken on the ACTIVATION (its maximum sits at the smallest x where scale < 0).  Within one storage rounding of
    float64 (plus the float32 evaluation of pre)."""
    n, c, h, w = shape
    k = other_cases(dt, NB.forward_cases)[shape]
    la = Launch(k)
    sc, sh = la.scale.cpu().double().view(n, c, 1, 1).numpy(), la.shift.cpu().double().view(n, c, 1, 1).numpy()
    pre = k.x * sc + sh
    act = np.where(pre > 0, pre, NB.SLOPE * pre)
    slack = 4 * NB.U32 * (np.abs(k.x * sc) + np.abs(sh))
    ust = NB.UNIT[dt]
    pooled, pslack = NB.windows(act).max(-1), NB.windows(slack).max(-1)
    out = torch.full((n, h // 2, w // 2, c), float("nan"), dtype=U.tdt(dt), device=U.DEV)
    L.call("mrisr_norm_pool2", dt, la.xd.data_ptr(), la.scale.data_ptr(), la.shift.data_ptr(), out.data_ptr(), n, h, w, c, U.stream())
    torch.cuda.synchronize()
    r1 = NB.worst_ratio(U.nchw(out).double().numpy(), pooled, ust * np.abs(pooled) + pslack + NB.HALF_SUBNORMAL[dt])
    eye = torch.zeros(c, c, 3, 3)
    eye[:, :, 1, 1] = torch.eye(c)
    src = U.SrcSpec(t32(k.x), L.SRC_NORM, L.SP_POOL2, la.scale.cpu().view(n, c), la.shift.cpu().view(n, c))
    got, _ = U.conv_forward(dt, [src], eye, h // 2, w // 2, 3, with_stats=False)
    r2 = NB.worst_ratio(got.double().numpy(), pooled, ust * np.abs(pooled) + pslack + NB.HALF_SUBNORMAL[dt])
    up = F.interpolate(torch.from_numpy(act), scale_factor=2, mode="bilinear", align_corners=True).numpy()
    uabs = F.interpolate(torch.from_numpy(np.abs(act) + slack), scale_factor=2, mode="bilinear", align_corners=True).numpy()
    o2 = torch.full((n, 2 * h, 2 * w, c), float("nan"), dtype=U.tdt(dt), device=U.DEV)
    L.call("mrisr_norm_upsample2", dt, la.xd.data_ptr(), la.scale.data_ptr(), la.shift.data_ptr(), o2.data_ptr(), n, h, w, c, U.stream())
    torch.cuda.synchronize()
    wslack = 4 * 2 * max(h, w) * NB.U32 * 2 * np.abs(act).max()          # float32 source coordinate, as in the adjoint's bound
    r3 = NB.worst_ratio(U.nchw(o2).double().numpy(), up, ust * np.abs(up) + NB.KF * NB.U32 * uabs + wslack + NB.HALF_SUBNORMAL[dt])
    print(f"{NB.DTNAME[dt]} {shape}: error / bound norm_pool2 {r1:.3f}, SP_POOL2 loader {r2:.3f}, norm_upsample2 {r3:.3f}")
    assert r1 <= 1.0 and r2 <= 1.0 and r3 <= 1.0
