"""Pins tests/normfwdutil.py - the float64 specification test_gpu_norm_fwd_kernels.py holds csrc/norm.hip and the head of
csrc/head_stem.hip to - on the CPU: the float32 tap emulation against aten, every operation against torch float64 (1e-12), the
adjoint window claim of csrc/common.h, and the properties of the seeded inputs and case tables the GPU file relies on.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import normfwdutil as NU

TAP_SIZES = tuple(range(1, 65)) + (255, 256, 257, 511, 512)
WINDOW_SIZES = tuple(range(1, 4201)) + (8191, 8192, 16384, 16385, 30000, 65536)
TOL = 1e-12


def _close(a, b, what, tol=TOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    err = np.abs(a - b).max() / max(1.0, np.abs(b).max())
    assert err <= tol, f"{what}: {err:.3e}"


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


# ------------------------------------------------------------------------------------------------ taps
def test_up2_taps_reproduce_aten_float32_on_one_hot_rows():
    for n in TAP_SIZES:
        i0, i1, w1 = NU.up2_taps(n)
        eye = torch.eye(n, dtype=torch.float32).view(1, n, n, 1)          # channel j: the one-hot row j
        got = F.interpolate(eye, scale_factor=(2, 1), mode="bilinear", align_corners=True)[0, :, :, 0].numpy()      # [j][Y]
        want = np.zeros((n, 2 * n), dtype=np.float32)
        big = np.arange(2 * n)
        np.add.at(want, (i0, big), (np.float32(1) - w1).astype(np.float32))
        np.add.at(want, (i1, big), w1)
        assert np.array_equal(got != 0, want != 0), f"n {n}: taps differ"
        # aten forms w0 * a + w1 * b with w0 = 1 - w1: on a one-hot row the products are the weights themselves
        assert np.array_equal(got, want), f"n {n}: weights differ by {np.abs(got - want).max():.3e}"
        assert (w1 >= 0).all() and (w1 < 1).all() and (i0 <= i1).all() and i1.max() == n - 1


def test_bilinear_and_adjoint_equal_aten_float64():
    """The gather / scatter code with the coordinate in float64 (as aten has it for a float64 tensor); the float32 taps
    of the kernels go through the same code and keep it a pair of transposes."""
    rng = np.random.default_rng(5)
    for n in TAP_SIZES:
        other = 1 if n > 64 else (n % 3) + 1
        for h, w in ((n, other), (other, n)):
            x = rng.standard_normal((2, h, w, 3))
            xt = _nchw(x).requires_grad_(True)
            up = F.interpolate(xt, scale_factor=2, mode="bilinear", align_corners=True)
            got, mag = NU.up2_64(x, NU.up2_taps64)
            _close(got, _nhwc(up), f"up {h}x{w}")
            assert (mag >= np.abs(got) - 1e-12).all()
            dz = rng.standard_normal((2, 2 * h, 2 * w, 3))
            up.backward(_nchw(dz))
            adj, amag = NU.up2_adjoint64(dz, NU.up2_taps64)
            _close(adj, _nhwc(xt.grad), f"adjoint {h}x{w}")
            assert (amag >= np.abs(adj) - 1e-12).all()
            assert abs((got * dz).sum() - (x * adj).sum()) <= 1e-10 * (mag * np.abs(dz)).sum()
            got32, mag32 = NU.up2_64(x)                      # the kernels' float32 taps: the same pair of transposes
            adj32 = NU.up2_adjoint64(dz)[0]
            assert abs((got32 * dz).sum() - (x * adj32).sum()) <= 1e-10 * (mag32 * np.abs(dz)).sum()


def test_adjoint_window_claim():
    """csrc/common.h, up2_adjoint_weights: every Y with a non-zero float32 weight on low index y lies in [2y-1, 2y+2] - for
    every extent the engine can hand to the adjoint kernels, and the larger sizes listed."""
    for n in WINDOW_SIZES:
        bad = NU.window_violations(n)
        assert not bad, f"n {n}: (y, Y) outside the window: {bad[:4]}"
    from mri_superresolution_amd import engine
    checked = max(n for n in range(1, len(WINDOW_SIZES)) if WINDOW_SIZES[n - 1] == n)       # the contiguous part: 1 .. 4200
    assert checked == 4200 and engine.MAX_TRAIN_EXTENT <= checked
    # the width is bounded further by the stem weight gradient's row cache (48 KiB): the widest image of the reference's
    # configuration (64 filters) it takes lies inside the range as well
    for dt in NU.DTYPES:
        widest = max(w for w in range(1, 8192) if NU.stem_row_cache_bytes(w, 64, dt, 64) <= 48 * 1024)
        assert widest <= checked, (dt, widest)


# ------------------------------------------------------------------------------------------------ operations against torch float64
def _act_t(x64, sc, sh):
    x = _nchw(x64)
    n, c = sc.shape
    return F.leaky_relu(x * torch.from_numpy(sc).double().view(n, c, 1, 1) + torch.from_numpy(sh).double().view(n, c, 1, 1), NU.SLOPE)


@pytest.mark.parametrize("dt", NU.DTYPES)
def test_activation_blend_pool_and_upsample_equal_torch_float64(dt):
    shape = (2, 7, 9, 24)
    _, x0, s0, t0 = NU.act_input(shape, dt, 11)
    _, x1, s1, t1 = NU.act_input(shape, dt, 12)
    a0, a1 = _act_t(x0, s0, t0), _act_t(x1, s1, t1)
    v, m, _ = NU.act64(x0, s0, t0)
    _close(v, _nhwc(a0), "activation")
    assert (m >= np.abs(v) - 1e-15).all()
    for alpha in (0.0, 20.0, -20.0, 0.3):
        sg = torch.sigmoid(torch.tensor(np.float32(alpha)).double())
        got, mag = NU.blend64(x0, s0, t0, x1, s1, t1, alpha)
        _close(got, _nhwc(sg * a0 + (1 - sg) * a1), f"blend {alpha}")
        assert (mag >= np.abs(got) - 1e-15).all()
    pv, pm, _ = NU.norm_pool64(x0, s0, t0)
    _close(pv, _nhwc(F.max_pool2d(a0, 2)), "pool")
    assert pv.shape == (2, 3, 4, 24) and (pm >= np.abs(pv) - 1e-15).all()
    uv, um = NU.norm_up64(x0, s0, t0, NU.up2_taps64)
    _close(uv, _nhwc(F.interpolate(a0, scale_factor=2, mode="bilinear", align_corners=True)), "norm_upsample2")
    assert (um >= np.abs(uv) - 1e-15).all()


@pytest.mark.parametrize("k", NU.HEAD_K)
def test_head_forward_and_backward_equal_autograd_float64(k):
    n, hw, c = 2, 37, 24
    rng = np.random.default_rng(20 + k)
    _, x, sc, sh = NU.act_input((n, hw, 1, c), "bf16", 21)
    x = x.reshape(n, hw, c)
    w = (0.3 * rng.standard_normal((k, c))).astype(np.float32)
    b = (0.2 * rng.standard_normal(k)).astype(np.float32)
    z, mz, out = NU.head_forward64(x, sc, sh, w, b)
    act = _act_t(x.reshape(n, hw, 1, c), sc, sh).requires_grad_(True)                   # [N][C][HW][1]
    wt, bt = torch.from_numpy(w).double().requires_grad_(True), torch.from_numpy(b).double().requires_grad_(True)
    ref = torch.sigmoid(F.conv2d(act, wt.view(k, c, 1, 1), bt))                         # [N][K][HW][1]
    _close(out, ref.detach().numpy()[..., 0], "head forward")
    assert (mz >= np.abs(z) - 1e-15).all()
    dout = rng.standard_normal((n, k, hw)).astype(np.float32)
    dout[1] = 0
    ref.backward(torch.from_numpy(dout).double().unsqueeze(-1))
    got = NU.head_backward64(x, sc, sh, w, out, dout)          # (out in float64 here: the same values autograd saved)
    _close(got["da"], act.grad.numpy()[..., 0].transpose(0, 2, 1), "da")
    _close(got["dw"], wt.grad.numpy(), "dw")
    _close(got["db"], bt.grad.numpy(), "db")
    assert (got["da"][1] == 0).all() and (got["m_dw"] >= np.abs(got["dw"]) - 1e-15).all()


def test_channel_sums_and_group_statistics():
    _, x = NU.raw_input((5, 11, 24), "f16", 30)
    out0 = NU.start_pattern((24,))
    got, mag = NU.channel_sum64(x.reshape(-1, 24), out0)
    _close(got, out0.astype(np.float64) + torch.from_numpy(x).sum((0, 1)).numpy(), "channel sums")
    assert (out0 != 0).all() and (mag >= np.abs(got)).all()
    s, ss, sa = NU.group_stats64(x)
    xt = torch.from_numpy(x).view(5, 11, 8, 3)
    _close(s, xt.sum((1, 3)).numpy(), "sums")
    _close(ss, (xt * xt).sum((1, 3)).numpy(), "sums of squares")
    assert (sa >= np.abs(s)).all()


@pytest.mark.parametrize("n,c", NU.GN_SIZES)
@pytest.mark.parametrize("eps", [1e-5, 1e-3])
def test_gn_finalize_equals_group_norm_float64(n, c, eps):
    x, gamma, beta = NU.gn_input(n, c, "plain", 40)
    stats = NU.slot_stats(x)
    assert all(len({float(v) for v in stats[:, i, g, 0]}) == NU.STAT_SLOTS for i in range(n) for g in range(NU.GROUPS)), "slots repeat"
    count = float((c // NU.GROUPS) * NU.GN_PIXELS)
    scale, shift, mean, rstd, _ = NU.gn_finalize64(stats, gamma, beta, count, eps)
    e32 = float(np.float32(eps))
    ref = F.group_norm(torch.from_numpy(x).permute(0, 2, 1).contiguous(), NU.GROUPS, torch.from_numpy(gamma).double(),
                       torch.from_numpy(beta).double(), e32).permute(0, 2, 1).numpy()
    _close(x * scale[:, None, :] + shift[:, None, :], ref, "scale, shift", 1e-12)
    xg = x.reshape(n, NU.GN_PIXELS, NU.GROUPS, -1)
    _close(mean, xg.mean((1, 3)), "mean")
    _close(rstd, 1 / np.sqrt(xg.var((1, 3)) + e32), "rstd")
    # mean 1000, deviation 1: ss / count - mean^2 cancels 6 digits, so the one-pass variance holds 1e-16 * 1e6 relative
    xo, go, bo = NU.gn_input(n, c, "offset", 41)
    _, _, mo, ro, _ = NU.gn_finalize64(NU.slot_stats(xo), go, bo, count, eps)
    xg = xo.reshape(n, NU.GN_PIXELS, NU.GROUPS, -1)
    _close(mo, xg.mean((1, 3)), "offset mean")
    _close(ro, 1 / np.sqrt(xg.var((1, 3)) + e32), "offset rstd", 1e-9)


def test_clamp_statistics_have_a_negative_float64_variance():
    for n, c in NU.GN_SIZES:
        stats, count = NU.clamp_stats(n, c)
        tot = stats.sum(0)
        mean = tot[..., 0] / count
        assert (tot[..., 1] / count - mean * mean < 0).all() and (tot[..., 0] > 0).all()
        _, _, _, rstd, _ = NU.gn_finalize64(stats, np.ones(c, np.float32), np.zeros(c, np.float32), count, 1e-5)
        assert (rstd == 1 / np.sqrt(float(np.float32(1e-5)))).all()


# ------------------------------------------------------------------------------------------------ the inputs and the case tables
@pytest.mark.parametrize("dt", NU.DTYPES)
def test_activation_inputs_keep_their_share_and_distance(dt):
    shape = (3, 11, 13, 24)
    _, x, sc, sh = NU.act_input(shape, dt, 50)
    v, _, pre = NU.act64(x, sc, sh)
    share = (pre < 0).mean()
    assert abs(share - NU.NEG_SHARE) < 0.02 and np.abs(pre).min() >= NU.MIN_ABS_PRE
    assert (v[pre < 0] == pre[pre < 0] * NU.SLOPE).all() and (v[pre > 0] == pre[pre > 0]).all()       # both branches are taken
    _, _, winner = NU.norm_pool64(x, sc, sh)
    assert set(np.unique(winner)) == {0, 1, 2, 3}, "a pool position never wins"
    # the smallest shapes the GPU file builds pass the maker's own assertion too
    NU.act_input((NU.N_IMAGES, 1, 1, NU.VEC[dt]), dt, 51)
    NU.act_input((NU.N_IMAGES, 2, 2, NU.VEC[dt]), dt, 52)


@pytest.mark.parametrize("dt", NU.DTYPES)
@pytest.mark.parametrize("cc", NU.C_CASES)
def test_pixel_cases_reach_one_two_and_three_blocks(dt, cc):
    c = NU.channels(cc, dt)
    for kernel, shape_of, items_of in (("blend", NU.blend_hw, lambda h, w: h * w), ("pool", NU.pool_hw, lambda h, w: (h // 2) * (w // 2)),
                                       ("norm_up", NU.norm_up_hw, lambda h, w: (h + 1) * (w + 1))):
        blocks, tails = [], []
        for kind in NU.HW_KINDS:
            h, w = shape_of(c, dt, kind)
            items = items_of(h, w)
            per_block, lanes = NU.pixel_blocks(items, c, dt, NU.PER_LANE[kernel])
            blocks.append(-(-items // per_block))
            tails.append(items - (blocks[-1] - 1) * per_block)
            assert items * (4 if kernel == "norm_up" else 1) <= 70000, (kernel, kind, h, w)
        assert blocks == [1, 1, 1, 2, 3], (kernel, blocks)
        full = NU.full_block(c, dt, NU.PER_LANE[kernel])
        assert tails[2] == full and tails[3] <= 3 and tails[4] <= 6, (kernel, tails)        # a full block; short tails after it
    if cc == 24:
        assert 256 % (c // NU.VEC[dt]) != 0, "C = 24 must leave idle threads (pl >= ppb)"


def test_statistics_cases_reach_their_branches_and_tell_rounded_from_unrounded():
    n, cc, h, w = NU.UP_STATS_CASES["wrap"]
    assert -(-4 * h * w // ((256 // (cc // 4)) * 16)) > NU.STAT_SLOTS          # float32: more blocks per image than slots
    # bfloat16: the sums of the unrounded interpolant (what upsample2_stats adds up) and of the stored tensor differ by
    # more than the bar of the GPU file in at least one statistic of every (n, group) of the larger cases, and by several bars
    # in the typical one - so that file does tell them apart
    for name, (n, cc, h, w) in NU.UP_STATS_CASES.items():
        c = NU.channels(cc, "bf16")
        _, x = NU.raw_input((n, h, w, c), "bf16", 60)
        z, mag = NU.up2_64(x)
        zr = torch.from_numpy(z).float().to(torch.bfloat16).double().numpy()
        s, ss, _ = NU.group_stats64(z)
        sr, ssr, _ = NU.group_stats64(zr)
        ms, mss, _ = NU.group_stats64(mag)
        bar_s, bar_ss = (16 + NU.N_UP) * NU.U32 * ms, (16 + 2 * NU.N_UP + 1) * NU.U32 * mss
        apart = np.maximum(np.abs(s - sr) / bar_s, np.abs(ss - ssr) / bar_ss)
        if name in ("c24", "wrap", "two_blocks_tail"):
            assert apart.min() > 1.5, (name, apart.min())          # every (n, group) tells them apart
        assert np.median(apart) > 3, (name, np.median(apart))


def test_stem_cases_reach_the_general_epilogue_and_the_wide_row_branch():
    general = lambda cout, dt: (lambda nvec: (nvec & (nvec - 1)) != 0 or nvec > 64 or cout > 128)(cout // NU.VEC[dt])     # noqa: E731
    for dt, cout, h, w, _ in NU.STEM_CASES:
        assert NU.stem_row_cache_bytes(w, cout, dt, 32) + 16 * NU.GROUPS <= 64 * 1024 and NU.stem_row_cache_bytes(w, cout, dt, 64) <= 48 * 1024
    assert all(general(cout, dt) for dt, cout, *_ in NU.STEM_CASES if cout in (24, 48, 256, 512))
    nvec256 = 256 // NU.VEC["bf16"]
    assert nvec256 & (nvec256 - 1) == 0
    ppblk, _ = NU.stem_block_pixels(71, 512, "f32", 32)
    assert 256 // (512 // 4) * 32 < 71 and ppblk % 71 != 0 and ppblk >= 71
