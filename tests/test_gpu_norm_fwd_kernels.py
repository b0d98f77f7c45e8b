"""csrc/norm.hip, the head half of csrc/head_stem.hip and the general epilogue of stem_wgrad through their C entry points,
against the float64 specification of tests/normfwdutil.py (pinned on the CPU by test_norm_fwd_ref_host.py).  A rewrite of the
kernels that keeps the C ABI must keep this file passing unchanged.

What is run: all three storage types; N = 3 unless a case says otherwise; every output and every accumulated buffer between guard
bands (hiputil.Guarded), pure outputs filled with NaN first, accumulated ones (dw, db, channel sums, statistics, the stem's dw)
started from a non-zero pattern.  The shapes are the smallest that reach each branch (normfwdutil's case tables say which).

Bars, derived and not measured (normfwdutil's docstring): per element u_T |ref| + n_ops 2^-24 M + floor_T; float32 accumulators
the same with u_T = 0 and n_ops = trips of a thread + reduction depth + one per block; statistics (per_lane + n_ops) 2^-24
sum |terms| against the float64 sum of exactly the values the kernel adds up - upsample2_stats: the UNROUNDED float32
interpolant; stem_forward and gn_stats: the STORED, rounded values.  gn_finalize: 2 float32 ulps of the float64 result (the shift included, although
its two terms cancel: the kernel forms it in float64; plus 2^-52 of those terms).

The sigmoid of head_forward goes through __expf, whose error the source does not give.  Measured on the MI355X on logits that
are exact in float32 (test_head_sigmoid_on_exact_logits): worst |out - sigmoid64(z)| = 7.381e-08 in all three storage types (SIGMOID_WORST
below); the bar held
everywhere is 10 x that, which stays below the project's 1e-5.  Where the logit is rounded, its derived bar enters through the
sigmoid's slope (normfwdutil.sigmoid_slack).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from mri_superresolution_amd import _lib as L          # noqa: E402
import hiputil as U                                    # noqa: E402
import normfwdutil as NU                               # noqa: E402

DT = {"f32": L.F32, "bf16": L.BF16, "f16": L.F16}
E_ARG, E_SHAPE, E_UNSUPPORTED = -1, -2, -5
PROJECT_SIGMOID_BAR = 1e-5
SIGMOID_WORST = 7.381e-8
SIGMOID_BAR = 10 * SIGMOID_WORST
assert SIGMOID_BAR < PROJECT_SIGMOID_BAR
N = NU.N_IMAGES
NAN = float("nan")


def _report(line):
    """The measured figure behind an assertion, in the test's captured output (pytest -rA or -s shows it)."""
    print(line)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(U.DEV)


def _nan_out(shape, dtype):
    return U.Guarded(torch.full(tuple(shape), NAN, dtype=dtype))


def _np(t):
    return t.detach().cpu().double().numpy()


def _within(got, ref, bar, what):
    """Every element finite and within its own bar; reports the worst error / bar."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} elements left unwritten or not finite"
    ratio = np.abs(got - ref) / bar
    worst = float(ratio.max())
    _report(f"{what}: worst error / bar {worst:.3f}")
    if worst > 1:
        i = np.unravel_index(ratio.argmax(), ratio.shape)
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} of {ratio.size} elements past their bar; worst at {tuple(map(int, i))}: "
                             f"got {got[i]!r}, reference {ref[i]!r}, bar {bar[i]:.3e} ({worst:.2f} x)")
    return worst


@functools.lru_cache(maxsize=None)
def _act_case(shape, dt, seed):
    return NU.act_input(shape, dt, seed)


# ------------------------------------------------------------------------------------------------ gn_finalize
def _gn_finalize(stats, gamma, beta, n, c, count, eps):
    sd = torch.from_numpy(np.ascontiguousarray(stats)).to(U.DEV)
    scale, shift = _nan_out((n, c), torch.float32), _nan_out((n, c), torch.float32)
    mr = _nan_out((n, NU.GROUPS, 2), torch.float32)
    gd, bd = _f32(gamma), _f32(beta)
    L.call("mrisr_gn_finalize", sd.data_ptr(), gd.data_ptr(), bd.data_ptr(), scale.data_ptr(), shift.data_ptr(), mr.data_ptr(), n, c,
           NU.GROUPS, float(count), float(eps), U.stream())
    torch.cuda.synchronize()
    for g, name in ((scale, "scale"), (shift, "shift"), (mr, "meanrstd")):
        g.check(f"gn_finalize: {name}")
    return _np(scale.t), _np(shift.t), _np(mr.t)


def _check_gn(got, ref, what):
    scale, shift, mr = got
    r_scale, r_shift, r_mean, r_rstd, m_shift = ref
    _within(scale, r_scale, 2 * NU.ulp32(r_scale), what + " scale")
    _within(shift, r_shift, 2 * NU.ulp32(r_shift) + 2.0 ** -52 * m_shift, what + " shift")
    _within(mr[..., 0], r_mean, 2 * NU.ulp32(r_mean), what + " mean")          # every (n, group) pair written (none left NaN)
    _within(mr[..., 1], r_rstd, 2 * NU.ulp32(r_rstd), what + " rstd")


@pytest.mark.parametrize("eps", [1e-5, 1e-3])
@pytest.mark.parametrize("kind", ["plain", "offset"])
@pytest.mark.parametrize("n,c", NU.GN_SIZES)
def test_gn_finalize_sixteen_slots(n, c, kind, eps):
    """All 16 slots filled with different partial sums; N > 1: the slot stride (k N + n) groups + g; N C on and off 256."""
    x, gamma, beta = NU.gn_input(n, c, kind, 40)
    stats = NU.slot_stats(x)
    count = float((c // NU.GROUPS) * NU.GN_PIXELS)
    ref = NU.gn_finalize64(stats, gamma, beta, count, eps)
    _check_gn(_gn_finalize(stats, gamma, beta, n, c, count, eps), ref, f"gn_finalize {n}x{c} {kind} eps {eps:g}")


@pytest.mark.parametrize("n,c", NU.GN_SIZES)
def test_gn_finalize_clamps_a_negative_variance(n, c):
    stats, count = NU.clamp_stats(n, c)
    rng = np.random.default_rng(45)
    gamma, beta = (0.5 + rng.random(c)).astype(np.float32), (0.3 * rng.standard_normal(c)).astype(np.float32)
    for eps in (1e-5, 1e-3):
        got = _gn_finalize(stats, gamma, beta, n, c, count, eps)
        ref = NU.gn_finalize64(stats, gamma, beta, count, eps)
        assert (ref[3] == 1 / np.sqrt(float(np.float32(eps)))).all()
        assert (got[2][..., 1] == np.float32(ref[3])).all(), "rstd must be exactly 1 / sqrt(eps): the clamp"
        _check_gn(got, ref, f"gn_finalize clamp {n}x{c} eps {eps:g}")


# ------------------------------------------------------------------------------------------------ blend, pool, upsample of the activation
@pytest.mark.parametrize("kind", NU.HW_KINDS)
@pytest.mark.parametrize("cc", NU.C_CASES)
@pytest.mark.parametrize("dt", NU.DTYPES)
def test_norm_blend(dt, cc, kind):
    c = NU.channels(cc, dt)
    h, w = NU.blend_hw(c, dt, kind)
    t0, x0, s0, sh0 = _act_case((N, h, w, c), dt, 101)
    t1, x1, s1, sh1 = _act_case((N, h, w, c), dt, 102)
    dev = [t0.to(U.DEV), _f32(s0), _f32(sh0), t1.to(U.DEV), _f32(s1), _f32(sh1)]
    for alpha in (0.0, 20.0, -20.0, 0.3):
        ad = _f32([alpha])
        out = _nan_out((N, h, w, c), NU.TORCH[dt])
        L.call("mrisr_norm_blend", DT[dt], *[t.data_ptr() for t in dev], ad.data_ptr(), out.data_ptr(), N, h, w, c, U.stream())
        torch.cuda.synchronize()
        out.check("norm_blend: out")
        ref, mag = NU.blend64(x0, s0, sh0, x1, s1, sh1, alpha)
        _within(_np(out.t), ref, NU.elem_bar(ref, mag, NU.N_BLEND, dt), f"norm_blend {dt} C{c} {h}x{w} alpha {alpha}")


def _pool(dt, c, h, w, seed):
    t, x, sc, sh = _act_case((N, h, w, c), dt, seed)
    out = _nan_out((N, h // 2, w // 2, c), NU.TORCH[dt])
    xd, scd, shd = t.to(U.DEV), _f32(sc), _f32(sh)
    L.call("mrisr_norm_pool2", DT[dt], xd.data_ptr(), scd.data_ptr(), shd.data_ptr(), out.data_ptr(), N, h, w, c, U.stream())
    torch.cuda.synchronize()
    out.check("norm_pool2: out")
    ref, mag, _ = NU.norm_pool64(x, sc, sh)
    _within(_np(out.t), ref, NU.elem_bar(ref, mag, NU.N_POOL, dt), f"norm_pool2 {dt} C{c} {h}x{w}")


@pytest.mark.parametrize("kind", NU.HW_KINDS)
@pytest.mark.parametrize("cc", NU.C_CASES)
@pytest.mark.parametrize("dt", NU.DTYPES)
def test_norm_pool2_odd_planes(dt, cc, kind):
    """Odd H and W: the last row and column are dropped; a swapped or shifted window element misses the bar by whole values."""
    c = NU.channels(cc, dt)
    _pool(dt, c, *NU.pool_hw(c, dt, kind), 111)


@pytest.mark.parametrize("dt", NU.DTYPES)
def test_norm_pool2_smallest_plane_and_refusal(dt):
    c = NU.VEC[dt]
    _pool(dt, c, 2, 2, 112)
    _pool(dt, 24, 2, 5, 113)
    x = torch.zeros(N * 5 * c, dtype=NU.TORCH[dt], device=U.DEV)
    sc = torch.ones(N * c, device=U.DEV)
    out = torch.full((N * 5 * c,), 7.0, dtype=NU.TORCH[dt], device=U.DEV)
    lib = L.load()
    for h, w in ((1, 5), (5, 1)):
        assert lib.mrisr_norm_pool2(DT[dt], x.data_ptr(), sc.data_ptr(), sc.data_ptr(), out.data_ptr(), N, h, w, c, U.stream()) == E_SHAPE
    torch.cuda.synchronize()
    assert (out == 7.0).all()          # nothing was launched


@pytest.mark.parametrize("kind", NU.HW_KINDS)
@pytest.mark.parametrize("cc", NU.C_CASES)
@pytest.mark.parametrize("dt", NU.DTYPES)
def test_norm_upsample2(dt, cc, kind):
    c = NU.channels(cc, dt)
    h, w = NU.norm_up_hw(c, dt, kind)
    t, x, sc, sh = _act_case((N, h, w, c), dt, 121)
    out = _nan_out((N, 2 * h, 2 * w, c), NU.TORCH[dt])
    xd, scd, shd = t.to(U.DEV), _f32(sc), _f32(sh)
    L.call("mrisr_norm_upsample2", DT[dt], xd.data_ptr(), scd.data_ptr(), shd.data_ptr(), out.data_ptr(), N, h, w, c, U.stream())
    torch.cuda.synchronize()
    out.check("norm_upsample2: out")
    ref, mag = NU.norm_up64(x, sc, sh)
    _within(_np(out.t), ref, NU.elem_bar(ref, mag, NU.N_NORM_UP, dt), f"norm_upsample2 {dt} C{c} {h}x{w}")


# ------------------------------------------------------------------------------------------------ upsample2_stats
def _stats_within(got, start, s_ref, ss_ref, m_s, m_ss, per_lane, n_s, n_ss, what):
    """got, start: [slots][N][groups][2] after and before the launch; the slot sums against the float64 sums."""
    d = got.sum(0) - start.sum(0)
    _within(d[..., 0], s_ref, (per_lane + n_s) * NU.U32 * m_s, what + " sums")
    _within(d[..., 1], ss_ref, (per_lane + n_ss) * NU.U32 * m_ss, what + " sums of squares")


@pytest.mark.parametrize("case", list(NU.UP_STATS_CASES))
@pytest.mark.parametrize("dt", NU.DTYPES)
def test_upsample2_stats(dt, case):
    """z against the float64 interpolant; both statistics, accumulated onto a non-zero buffer, against the float64 sums of the
    UNROUNDED interpolant (what the kernel adds up: 16 float32 terms per thread, then float64); stats = NULL writes z alone."""
    n, cc, h, w = NU.UP_STATS_CASES[case]
    c = NU.channels(cc, dt)
    t, x = NU.raw_input((n, h, w, c), dt, 60)
    xd = t.to(U.DEV)
    ref, mag = NU.up2_64(x)
    bar = NU.elem_bar(ref, mag, NU.N_UP, dt)
    start = NU.stats_start(n)
    for with_stats in (True, False):
        z = _nan_out((n, 2 * h, 2 * w, c), NU.TORCH[dt])
        stats = U.Guarded(torch.from_numpy(start.copy()))
        L.call("mrisr_upsample2_stats", DT[dt], xd.data_ptr(), z.data_ptr(), stats.data_ptr() if with_stats else None, n, h, w, c,
               NU.GROUPS, U.stream())
        torch.cuda.synchronize()
        z.check("upsample2_stats: z")
        stats.check("upsample2_stats: stats")          # no slot beyond 16 N groups 2 is touched
        what = f"upsample2_stats {dt} {case} C{c} {h}x{w}" + ("" if with_stats else " stats=NULL")
        _within(_np(z.t), ref, bar, what + " z")
        got = stats.t.cpu().numpy()
        if not with_stats:
            assert np.array_equal(got, start), what
            continue
        s, ss, _ = NU.group_stats64(ref)
        m_s, m_ss, _ = NU.group_stats64(mag)
        _stats_within(got, start, s, ss, m_s, m_ss, 16, NU.N_UP, 2 * NU.N_UP + 1, what)
        blocks = -(-4 * h * w // ((256 // (c // NU.VEC[dt])) * 16))
        touched = (got != start).any((1, 2, 3)).sum()
        assert touched == min(NU.STAT_SLOTS, blocks + n - 1), f"{what}: {touched} slots changed, {blocks} blocks per image"


# ------------------------------------------------------------------------------------------------ upsample2_adjoint
@pytest.mark.parametrize("case", list(NU.ADJ_CASES))
@pytest.mark.parametrize("dt", NU.DTYPES)
def test_upsample2_adjoint(dt, case):
    n, cc, h, w = NU.ADJ_CASES[case]
    c = NU.channels(cc, dt)
    t, dz = NU.raw_input((n, 2 * h, 2 * w, c), dt, 70)
    dzd = t.to(U.DEV)
    out = _nan_out((n, h, w, c), NU.TORCH[dt])
    L.call("mrisr_upsample2_adjoint", DT[dt], dzd.data_ptr(), out.data_ptr(), n, h, w, c, U.stream())
    torch.cuda.synchronize()
    out.check("upsample2_adjoint: dz_low")
    ref, mag = NU.up2_adjoint64(dz)
    got = _np(out.t)
    what = f"upsample2_adjoint {dt} {case} C{c}"
    _within(got, ref, NU.elem_bar(ref, mag, NU.N_ADJ, dt), what)
    if dt == "f32":
        # <up(x), dz> == <x, adj(dz)>, the left side from the forward reference alone: each side's error is bounded by the sum
        # of its element bars
        _, x = NU.raw_input((n, h, w, c), dt, 71)
        up, up_mag = NU.up2_64(x)
        lhs, rhs = (up * dz).sum(), (x * got).sum()
        bar = (np.abs(x) * NU.elem_bar(ref, mag, NU.N_ADJ, dt)).sum() + 1e-13 * (up_mag * np.abs(dz)).sum()
        _report(f"{what}: inner products differ by {abs(lhs - rhs):.3e} (bar {bar:.3e})")
        assert abs(lhs - rhs) <= bar, what


# ------------------------------------------------------------------------------------------------ channel_sum
@pytest.mark.parametrize("kind", NU.CHANNEL_SUM_PIX)
@pytest.mark.parametrize("cc", NU.CHANNEL_SUM_C)
@pytest.mark.parametrize("dt", NU.DTYPES)
def test_channel_sum(dt, cc, kind):
    c = NU.channels(cc, dt)
    npix = NU.channel_sum_pixels(c, dt, kind)
    t, x = NU.raw_input((npix, c), dt, 80)
    out0 = NU.start_pattern((c,))
    out = U.Guarded(torch.from_numpy(out0.copy()))
    xd = t.to(U.DEV)
    L.call("mrisr_channel_sum", DT[dt], xd.data_ptr(), out.data_ptr(), npix, c, U.stream())
    torch.cuda.synchronize()
    out.check("channel_sum: out")
    ref, mag = NU.channel_sum64(x, out0)
    _within(_np(out.t), ref, NU.accum_bar(mag, NU.n_channel_sum(npix, c, dt)), f"channel_sum {dt} C{c} {npix} pixels")


# ------------------------------------------------------------------------------------------------ gn_stats through conv_forward
@pytest.mark.parametrize("hw", [(31, 33), (32, 32), (25, 41)], ids=["1023", "1024", "1025"])
@pytest.mark.parametrize("cout", [8, 16, 24])
@pytest.mark.parametrize("dt", NU.DTYPES)
def test_gn_stats_through_conv_forward(dt, cout, hw):
    """Groups of 1, 2 and 3 channels: conv_forward leaves the statistics to the stand-alone gn_stats pass (blocks of 1024
    pixels).  A 1 x 1 identity convolution of a dyadic tensor: the stored output is the input, and both statistics are exact."""
    h, w = hw
    x = U.dyadic((N, cout, h, w), 90, 0.6, values=(-2, -1, 1, 2))
    wt = torch.eye(cout).view(cout, cout, 1, 1)
    stats0 = U.int_pattern((L.STAT_SLOTS, N, 8, 2), torch.float64)
    out, st, ran = U.conv_forward_guarded(DT[dt], [U.SrcSpec(x)], wt, h, w, 1, stats0=stats0)
    assert ran.startswith("conv_igemm_kernel<"), ran
    U.assert_exact(out, x.double(), DT[dt], "A", f"{ran}: identity")
    o = out.double().view(N, 8, cout // 8, h, w)              # the STORED tensor
    U.assert_exact(st[..., 0], o.sum((2, 3, 4)) + stats0.sum(0)[..., 0], "f64", "A", "gn_stats sums")
    U.assert_exact(st[..., 1], (o * o).sum((2, 3, 4)) + stats0.sum(0)[..., 1], "f64", "A", "gn_stats sums of squares")


@pytest.mark.parametrize("dt", NU.DTYPES)
def test_pixel_shuffle_statistics_need_whole_groups(dt):
    """A pixel-shuffle output has Cout / 4 channels.  With groups that divide them the group is never narrower than 4 of the
    conv's channels, so the stand-alone gn_stats pass is not reached; Cout 16 with 8 groups would reach it with a group size of
    zero and is refused before anything is launched."""
    keep = []
    x = U.dyadic((N, 8, 6, 6), 91, 0.6)
    d = U.make_desc(DT[dt], [U.SrcSpec(x)], 6, 6, 8, 16, 3, out_mode=L.OUT_PIXEL_SHUFFLE2, keep=keep)
    wp = U.pack(U.dyadic((16, 8, 3, 3), 92, 0.5), DT[dt], 0)
    out = torch.full((N, 12, 12, 4), 7.0, dtype=NU.TORCH[dt], device=U.DEV)
    stats = torch.zeros(L.STAT_SLOTS * N * 8 * 2, dtype=torch.float64, device=U.DEV)
    d.wpacked, d.out, d.stats = wp.data_ptr(), out.data_ptr(), stats.data_ptr()
    assert L.load().mrisr_conv_forward(C.byref(d), U.stream()) == E_SHAPE
    assert b"pixel shuffle" in L.load().mrisr_last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (stats == 0).all()


# ------------------------------------------------------------------------------------------------ head
def _head_params(k, c, seed):
    rng = np.random.default_rng(seed)
    return (0.3 * rng.standard_normal((k, c))).astype(np.float32), (0.2 * rng.standard_normal(k)).astype(np.float32)


def _head_forward(dt, xd, sc, sh, w, b, n, hw, c, k, single=False):
    out = _nan_out((n, k, hw), torch.float32)
    args = [DT[dt], xd.data_ptr(), _f32(sc), _f32(sh), _f32(w), _f32(b)]
    ptrs = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    if single:
        L.call("mrisr_head_forward", *ptrs, out.data_ptr(), n, 1, hw, c, U.stream())
    else:
        L.call("mrisr_head_forward_multi", *ptrs, out.data_ptr(), n, 1, hw, c, k, U.stream())
    torch.cuda.synchronize()
    del args
    out.check("head_forward: out")
    return _np(out.t)


@pytest.mark.parametrize("hw", NU.HEAD_FWD_HW)
@pytest.mark.parametrize("cc", NU.HEAD_C)
@pytest.mark.parametrize("dt", NU.DTYPES)
def test_head_forward(dt, cc, hw):
    """K = 1 .. 4 (and the one-channel entry point); H W on both sides of the 256-pixel block.  Bar: the logit's derived bar through
    the sigmoid's slope, plus SIGMOID_BAR."""
    c = NU.channels(cc, dt)
    t, x, sc, sh = _act_case((N, hw, 1, c), dt, 131)
    x = x.reshape(N, hw, c)
    xd = t.to(U.DEV)
    for k in NU.HEAD_K:
        w, b = _head_params(k, c, 132 + k)
        z, mz, ref = NU.head_forward64(x, sc, sh, w, b)
        dz = NU.n_logit(c) * NU.U32 * mz
        bar = NU.sigmoid_slack(z, dz) + SIGMOID_BAR
        got = _head_forward(dt, xd, sc, sh, w, b, N, hw, c, k)
        what = f"head_forward {dt} C{c} HW{hw} K{k}"
        _within(got, ref, bar, what)
        _report(f"{what}: worst |out - ref| {np.abs(got - ref).max():.3e}; logit bar through the slope at most {NU.sigmoid_slack(z, dz).max():.3e}")
        assert np.abs(got - ref).max() <= PROJECT_SIGMOID_BAR
        if k == 1:
            assert np.array_equal(_head_forward(dt, xd, sc, sh, w, b, N, hw, c, 1, single=True), got)


@pytest.mark.parametrize("dt", NU.DTYPES)
def test_head_sigmoid_on_exact_logits(dt):
    """Logits that float32 holds exactly (dyadic activations, weights and bias; scale 1, shift 0, nothing negative): what is left
    is the kernel's sigmoid alone.  The worst error over this test is the figure in the module docstring."""
    c, hw, k = 16, 257, 4
    x = U.dyadic((N, hw, c), 140, 0.7, values=(0.25, 0.5, 1, 2)).numpy()
    t, x64 = NU.stored(x, dt)
    assert np.array_equal(x64, x)
    sc, sh = np.ones((N, c), np.float32), np.zeros((N, c), np.float32)
    w = U.dyadic((k, c), 141, 0.8, values=(-1, -0.5, -0.25, 0.25, 0.5, 1)).numpy()
    b = np.array([-2, -0.5, 0.5, 2], np.float32)
    z, mz, ref = NU.head_forward64(x64.reshape(N, hw, c), sc, sh, w, b)
    assert mz.max() < 2 ** 10 and np.array_equal(z * 64, np.round(z * 64)) and z.min() < -4 and z.max() > 4
    got = _head_forward(dt, t.to(U.DEV), sc, sh, w, b, N, hw, c, k)
    worst = np.abs(got - ref).max()
    _report(f"head_forward {dt} sigmoid on exact logits in [{z.min():.2f}, {z.max():.2f}]: worst |out - sigmoid64(z)| {worst:.3e} "
            f"(recorded {SIGMOID_WORST:.3e}, bar {SIGMOID_BAR:.3e})")
    assert worst <= SIGMOID_BAR


@pytest.mark.parametrize("hw", NU.HEAD_BWD_HW)
@pytest.mark.parametrize("cc", NU.HEAD_C)
@pytest.mark.parametrize("dt", NU.DTYPES)
def test_head_backward(dt, cc, hw):
    """da, and dw / db accumulated onto a non-zero start; H W on both sides of the 2048-pixel block; dout zero on image 1."""
    c = NU.channels(cc, dt)
    t, x, sc, sh = _act_case((N, hw, 1, c), dt, 151)
    x = x.reshape(N, hw, c)
    xd, scd, shd = t.to(U.DEV), _f32(sc), _f32(sh)
    rng = np.random.default_rng(152)
    for k in NU.HEAD_K:
        w, b = _head_params(k, c, 153 + k)
        out = NU.head_forward64(x, sc, sh, w, b)[2].astype(np.float32)          # what the kernel reads as the forward's output
        dout = rng.standard_normal((N, k, hw)).astype(np.float32)
        dout[1] = 0
        ref = NU.head_backward64(x, sc, sh, w, out, dout)
        dw0, db0 = NU.start_pattern((k, c)), NU.start_pattern((k,), mod=5)
        da = _nan_out((N, hw, c), NU.TORCH[dt])
        dw, db = U.Guarded(torch.from_numpy(dw0.copy())), U.Guarded(torch.from_numpy(db0.copy()))
        wd, od, dd = _f32(w), _f32(out), _f32(dout)
        ptrs = [DT[dt], xd.data_ptr(), scd.data_ptr(), shd.data_ptr(), wd.data_ptr(), od.data_ptr(), dd.data_ptr(), da.data_ptr(),
                dw.data_ptr(), db.data_ptr(), N, 1, hw, c]
        if k == 1:
            L.call("mrisr_head_backward", *ptrs, U.stream())
        else:
            L.call("mrisr_head_backward_multi", *ptrs, k, U.stream())
        torch.cuda.synchronize()
        for g, name in ((da, "da"), (dw, "dw"), (db, "db")):
            g.check(f"head_backward: {name}")
        what = f"head_backward {dt} C{c} HW{hw} K{k}"
        got_da = _np(da.t)
        _within(got_da, ref["da"], NU.elem_bar(ref["da"], ref["m_da"], NU.n_da(k), dt), what + " da")
        assert (got_da[1] == 0).all(), "dout is zero on image 1"
        _within(_np(dw.t), ref["dw"] + dw0, NU.accum_bar(ref["m_dw"] + np.abs(dw0), NU.n_dw(N, hw, c, dt)), what + " dw")
        _within(_np(db.t), ref["db"] + db0, NU.accum_bar(ref["m_db"] + np.abs(db0), NU.n_db(N, hw, c, dt)), what + " db")


@pytest.mark.parametrize("dt", NU.DTYPES)
def test_head_refusals(dt):
    lib = L.load()
    c, hw = 16, 9
    x = torch.zeros(N * hw * 32, dtype=NU.TORCH[dt], device=U.DEV)
    f = torch.ones(8 * 32, device=U.DEV)
    out = torch.full((N * 8 * hw,), 7.0, device=U.DEV)
    da = torch.full((N * hw * 32,), 7.0, dtype=NU.TORCH[dt], device=U.DEV)
    dw = torch.full((8 * 32,), 7.0, device=U.DEV)
    for k, cc in ((0, c), (5, c), (-1, c), (2, c + NU.VEC[dt] // 2), (1, NU.VEC[dt] - 1)):
        assert lib.mrisr_head_forward_multi(DT[dt], x.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), out.data_ptr(),
                                            N, 1, hw, cc, k, U.stream()) == E_SHAPE, (k, cc)
        assert lib.mrisr_head_backward_multi(DT[dt], x.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), out.data_ptr(), out.data_ptr(),
                                             da.data_ptr(), dw.data_ptr(), dw.data_ptr(), N, 1, hw, cc, k, U.stream()) == E_SHAPE, (k, cc)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (da == 7.0).all() and (dw == 7.0).all()          # nothing was launched


# ------------------------------------------------------------------------------------------------ stem
@pytest.mark.parametrize("case", NU.STEM_CASES, ids=lambda v: f"{v[0]}-c{v[1]}-{v[2]}x{v[3]}")
def test_stem_general_shapes_exact(case):
    """What test_gpu_exact.py's stem test (Cout 32, 11 x 21) does not reach: dyadic image, weights and output gradient, every result
    bit for bit; the statistics and dw accumulated onto a non-zero start."""
    dt, cout, h, w, _ = case
    x = U.dyadic((N, 1, h, w), 200, 0.6, values=(-2, -1, 1, 2))
    wt = U.dyadic((cout, 1, 3, 3), 201, 0.6)
    ref = F.conv2d(x.double(), wt.double(), padding=1)
    xd, wd = x.to(U.DEV).contiguous(), wt.reshape(cout, 9).contiguous().to(U.DEV)
    out = _nan_out((N, h, w, cout), NU.TORCH[dt])
    stats0 = U.int_pattern((L.STAT_SLOTS, N, 8, 2), torch.float64)
    stats = U.Guarded(stats0)
    L.call("mrisr_stem_forward", DT[dt], xd.data_ptr(), wd.data_ptr(), out.data_ptr(), stats.data_ptr(), N, h, w, cout, 8, U.stream())
    torch.cuda.synchronize()
    out.check("stem out")
    stats.check("stem stats")
    U.assert_exact(U.nchw(out.t), ref, DT[dt], "A", "stem forward")
    o = ref.view(N, 8, cout // 8, h, w)
    st = stats.t.cpu().sum(0)
    U.assert_exact(st[..., 0], o.sum((2, 3, 4)) + stats0.sum(0)[..., 0], "f64", "A", "stem sums")
    U.assert_exact(st[..., 1], (o * o).sum((2, 3, 4)) + stats0.sum(0)[..., 1], "f64", "A", "stem sums of squares")
    dy = U.dyadic((N, cout, h, w), 202, 0.25)
    wr = torch.zeros(cout, 1, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wr, padding=1).backward(dy.double())
    wa = torch.zeros(cout, 1, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().abs(), wa, padding=1).backward(dy.double().abs())
    assert float(wa.grad.max()) + 3 < 2 ** 24
    dw0 = U.int_pattern((cout, 9), torch.float32)
    dw = U.Guarded(dw0)
    dyd = U.nhwc(dy, DT[dt])
    L.call("mrisr_stem_wgrad", DT[dt], xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), N, h, w, cout, U.stream())
    torch.cuda.synchronize()
    dw.check("stem dw")
    U.assert_exact(dw.t.cpu(), wr.grad.view(cout, 9) + dw0.double(), L.F32, "A", "stem wgrad")


def test_stem_statistics_are_those_of_the_stored_tensor():
    """bfloat16, undyadic weights: the stored output differs from the float32 result, and the statistics are the sums of the
    STORED values (32 float32 terms per thread, then float64) - not of the unrounded ones, which lie several bars away."""
    dt, cout, h, w = "bf16", 32, 11, 21
    rng = np.random.default_rng(210)
    x = torch.from_numpy(rng.random((N, 1, h, w)).astype(np.float32))
    wt = torch.from_numpy(rng.standard_normal((cout, 1, 3, 3)).astype(np.float32))
    xd, wd = x.to(U.DEV).contiguous(), wt.reshape(cout, 9).contiguous().to(U.DEV)
    out = _nan_out((N, h, w, cout), NU.TORCH[dt])
    start = NU.stats_start(N)
    stats = U.Guarded(torch.from_numpy(start.copy()))
    L.call("mrisr_stem_forward", DT[dt], xd.data_ptr(), wd.data_ptr(), out.data_ptr(), stats.data_ptr(), N, h, w, cout, 8, U.stream())
    torch.cuda.synchronize()
    out.check("stem out")
    stats.check("stem stats")
    o = _np(out.t)
    s, ss, sa = NU.group_stats64(o)
    per_lane = NU.stem_block_pixels(w, cout, dt, 32)[0] // NU.stem_block_pixels(w, cout, dt, 32)[1]
    unrounded = F.conv2d(x.double(), wt.double(), padding=1).permute(0, 2, 3, 1).numpy()
    su, ssu, _ = NU.group_stats64(unrounded)
    apart = np.maximum(np.abs(s - su) / ((per_lane + 0) * NU.U32 * sa), np.abs(ss - ssu) / ((per_lane + 1) * NU.U32 * ss))
    assert np.median(apart) > 3, f"the two candidates are not told apart: {np.median(apart)}"
    _stats_within(stats.t.cpu().numpy(), start, s, ss, sa, ss, per_lane, 0, 1, "stem_forward bf16 statistics of the stored tensor")


def test_stem_row_cache_refusals():
    """An image too wide for the LDS row cache (64 KiB forward, 48 KiB weight gradient), from the return code: refused before a launch."""
    lib = L.load()
    small = torch.zeros(1 << 16, device=U.DEV)
    out = torch.full((1 << 16,), 7.0, device=U.DEV)
    for dt in NU.DTYPES:
        assert NU.stem_row_cache_bytes(4096, 32, dt, 32) > 64 * 1024 and NU.stem_row_cache_bytes(2500, 32, dt, 64) > 48 * 1024
        assert lib.mrisr_stem_forward(DT[dt], small.data_ptr(), small.data_ptr(), out.data_ptr(), None, 1, 1, 4096, 32, 8, U.stream()) == E_UNSUPPORTED
        assert b"row cache" in lib.mrisr_last_error()
        assert lib.mrisr_stem_wgrad(DT[dt], small.data_ptr(), small.data_ptr(), out.data_ptr(), 1, 1, 2500, 32, U.stream()) == E_UNSUPPORTED
        assert b"row cache" in lib.mrisr_last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all()
