"""Forward GroupNorm passes (csrc/norm.hip) and the head of csrc/head_stem.hip: float64 specifications, the derived error bars
and the seeded inputs of test_norm_fwd_ref_host.py (which pins them to aten on the CPU) and test_gpu_norm_fwd_kernels.py.
Host code only: nothing here touches the GPU.

Every function takes the values the kernel actually reads - the input as float64 of the STORED (already rounded) tensor,
float32 scale, shift and weights - and computes in float64 throughout.  Tensors are NHWC as the kernels take them (the head's
out / dout are [N][K][HW]).  Next to the value every function returns its magnitude M: the sum of the absolute values of the
terms it added, per output element.

Element bar (derived, not measured):   |got - ref64| <= u_T |ref64| + n_ops 2^-24 M + floor_T
u_T: unit roundoff of the storage type; floor_T: half its smallest subnormal; n_ops: the float32 roundings on the longest path
from an input to one output, counted from the kernel text (the N_* constants below, each with its derivation; a fused
multiply-add only lowers the count).  The second term carries a factor (1 + u_T): the stored value is the rounding of the
float32 result, not of the reference.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

DTYPES = ("f32", "bf16", "f16")
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
VEC = {"f32": 4, "bf16": 8, "f16": 8}                           # elements of a 16-byte vector
U_T = {"f32": 2.0 ** -24, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
FLOOR_T = {"f32": 2.0 ** -150, "bf16": 2.0 ** -134, "f16": 2.0 ** -25}
U32 = 2.0 ** -24
SLOPE = float(np.float32(0.2))                                  # LRELU_SLOPE as the kernels hold it
STAT_SLOTS = 16
GROUPS = 8
MIN_ABS_PRE = 1e-3                                              # no pre-activation closer to zero than this

# ------------------------------------------------------------------------------------------------ n_ops, from the kernel text
N_ACT = 3            # lrelu(x * scale + shift): product, sum, slope product
N_BLEND = N_ACT + 7  # coefficient: __expf as scaling product + exp2 (2), 1 + e, reciprocal, 1 - a (5); a * act, the sum (2)
N_POOL = N_ACT       # fmaxf rounds nothing
N_UP = 6             # per axis: 1 - w, the product, the sum (3); two axes
N_NORM_UP = N_ACT + N_UP
N_ADJ = 12           # weights: 1 - w1 and the second += (2) per axis; per axis one product and at most 3 roundings of the 4-term chain
N_DZ = 3             # dout * o * (1 - o): 1 - o and two products


def n_logit(c):
    """z = b + sum_c act * w, one chain: the first term sees its activation (3), its product and C additions."""
    return N_ACT + 1 + c


def n_da(k):
    """da = sum_k dz * w: dz (3), the product, K additions."""
    return N_DZ + 1 + k


def head_bwd_geometry(n, hw, c, dt):
    """(pixel lanes, trips of a thread, blocks) of head_bwd_kernel: blocks of 2048 pixels, 256 / (C / VEC) pixel lanes."""
    ppb = 256 // (c // VEC[dt])
    return ppb, math.ceil(min(hw, 2048) / ppb), n * math.ceil(hw / 2048)


def n_dw(n, hw, c, dt):
    """dw += sum dz * act: dz (3), act (3), product, the thread's trips, one LDS adder per pixel lane, one global atomic per block."""
    ppb, trips, blocks = head_bwd_geometry(n, hw, c, dt)
    return N_DZ + N_ACT + 1 + trips + ppb + blocks


def n_db(n, hw, c, dt):
    """db += sum dz: dz (3), the thread's trips, the wave sum (6), one LDS adder per wave (4), one global atomic per block."""
    _, trips, blocks = head_bwd_geometry(n, hw, c, dt)
    return N_DZ + trips + 6 + 4 + blocks


def n_channel_sum(npix, c, dt):
    """32 trips per thread, the LDS column of 256 / (C / VEC) lanes, one global atomic per block."""
    ppb = 256 // (c // VEC[dt])
    return 32 + ppb + math.ceil(npix / (ppb * 32))


def elem_bar(ref, mag, n_ops, dt):
    return U_T[dt] * np.abs(ref) + (1 + U_T[dt]) * n_ops * U32 * mag + FLOOR_T[dt]


def accum_bar(mag, n_ops):
    """float32 accumulators (dw, db, channel sums): the element bar with u_T = 0."""
    return n_ops * U32 * mag


def ulp32(x):
    """Spacing of float32 at |x| (float64 array)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ blocking rules, restated
def pixel_blocks(items, c, dt, per_lane):
    """(items per block, lanes) of common.h's pixel_blocks for C / VEC <= 256."""
    lanes = 256 // (c // VEC[dt])
    per_block = lanes * per_lane
    if per_block > items:
        per_block = math.ceil(items / lanes) * lanes
    return per_block, lanes


def full_block(c, dt, per_lane):
    return (256 // (c // VEC[dt])) * per_lane


def stem_block_pixels(w, cout, dt, mult):
    """(pixels per block, pixel lanes) of head_stem.hip's stem_block_pixels (mult: 32 forward, 64 weight gradient)."""
    ppb = 256 // (cout // VEC[dt])
    ppblk = ppb * mult
    if ppblk < w:
        ppblk = math.ceil(w / ppb) * ppb
    return ppblk, ppb


def stem_row_cache_bytes(w, cout, dt, mult, cin=1):
    ppblk, _ = stem_block_pixels(w, cout, dt, mult)
    return cin * (ppblk // w + 4) * w * 4


PER_LANE = {"blend": 32, "pool": 16, "norm_up": 8, "adjoint": 4}       # per_lane argument of each entry point
HW_KINDS = ("one", "below", "full", "above", "two_and_tail")


def item_counts(c, dt, per_lane):
    """Items of the five cases: one item, one short of a full block, a full block, one more, two blocks and 3 items."""
    pb = full_block(c, dt, per_lane)
    return dict(zip(HW_KINDS, (1, pb - 1, pb, pb + 1, 2 * pb + 3)))


def split2(count):
    """count = a * b with a <= b, a the largest factor below the square root (1 x count for a prime)."""
    a = max(d for d in range(1, int(math.isqrt(count)) + 1) if count % d == 0)
    return a, count // a


def split2_from(count, least=2):
    """The smallest count' >= count that factors into a * b with a, b >= least, and that (a, b)."""
    while True:
        a, b = split2(count)
        if a >= least:
            return count, a, b
        count += 1


def blend_hw(c, dt, kind):
    return split2(item_counts(c, dt, PER_LANE["blend"])[kind])


def pool_hw(c, dt, kind):
    """Input (H, W), both odd: the last row and column are dropped; the pooled plane has exactly the case's items."""
    ho, wo = split2(item_counts(c, dt, PER_LANE["pool"])[kind])
    return 2 * ho + 1, 2 * wo + 1


def norm_up_hw(c, dt, kind):
    """Low-resolution (h, w): (h + 1)(w + 1) groups.  One item is not a shape (h, w >= 1): the smallest plane, 1 x 1 (4 groups);
    a prime count moves to the next one that factors."""
    want = item_counts(c, dt, PER_LANE["norm_up"])[kind]
    if kind == "one":
        return 1, 1
    _, a, b = split2_from(want)
    return a - 1, b - 1


# ------------------------------------------------------------------------------------------------ bilinear x2, align_corners
@functools.lru_cache(maxsize=None)
def up2_taps(n):
    """float32 emulation of common.h's up2_coord for every output index Y of an axis of n: (i0, i1 int64 [2n], w1 float32 [2n]).
    scale = f32(n-1) / f32(2n-1), src = scale * f32(Y), each rounded once (no contraction), i0 = min(int(src), n-1),
    i1 = i0 + (i0 < n-1), w1 = src - i0."""
    scale = np.float32(n - 1) / np.float32(2 * n - 1)
    src = (scale * np.arange(2 * n, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n - 1)
    i1 = i0 + (i0 < n - 1)
    w1 = (src - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, w1


@functools.lru_cache(maxsize=None)
def up2_taps64(n):
    """The same rule with the coordinate in float64, as aten computes it for a float64 tensor: pins the gather and scatter
    code of up2_64 / up2_adjoint64 against F.interpolate in float64 (test_norm_fwd_ref_host.py); the kernels' taps are up2_taps."""
    src = (n - 1) / (2 * n - 1) * np.arange(2 * n, dtype=np.float64)
    i0 = np.minimum(src.astype(np.int64), n - 1)
    return i0, i0 + (i0 < n - 1), src - i0


def adjoint_rows(n):
    """For every low index y: the output indices Y that put a non-zero weight on it, as (y [m], Y [m])."""
    i0, i1, w1 = up2_taps(n)
    big = np.arange(2 * n)
    w0 = (np.float32(1) - w1).astype(np.float32)
    y = np.concatenate([i0[w0 != 0], i1[w1 != 0]])
    return y, np.concatenate([big[w0 != 0], big[w1 != 0]])


def window_violations(n):
    """Pairs (y, Y) with a non-zero weight outside common.h's claim Y in [2y-1, 2y+2]."""
    y, big = adjoint_rows(n)
    bad = (big < 2 * y - 1) | (big > 2 * y + 2)
    return list(zip(y[bad].tolist(), big[bad].tolist()))


def _shape_on(axis, ndim, v):
    s = [1] * ndim
    s[axis] = -1
    return v.reshape(s)


def up2_axis(x, axis, taps=up2_taps):
    i0, i1, w1 = taps(x.shape[axis])
    w = _shape_on(axis, x.ndim, w1.astype(np.float64))
    return np.take(x, i0, axis) * (1.0 - w) + np.take(x, i1, axis) * w


def up2_64(x, taps=up2_taps):
    """[N][h][w][C] -> [N][2h][2w][C] and M (n_ops: N_UP)."""
    x = np.asarray(x, dtype=np.float64)
    return up2_axis(up2_axis(x, 2, taps), 1, taps), up2_axis(up2_axis(np.abs(x), 2, taps), 1, taps)


def up2_adj_axis(d, axis, taps=up2_taps):
    n = d.shape[axis] // 2
    i0, i1, w1 = taps(n)
    w = _shape_on(0, d.ndim, w1.astype(np.float64))
    dm = np.moveaxis(d, axis, 0)
    out = np.zeros((n,) + dm.shape[1:], dtype=np.float64)
    np.add.at(out, i0, dm * (1.0 - w))
    np.add.at(out, i1, dm * w)
    return np.moveaxis(out, 0, axis)


def up2_adjoint64(dz, taps=up2_taps):
    """[N][2h][2w][C] -> [N][h][w][C]: the transpose of up2_64, and M (n_ops: N_ADJ)."""
    dz = np.asarray(dz, dtype=np.float64)
    return up2_adj_axis(up2_adj_axis(dz, 2, taps), 1, taps), up2_adj_axis(up2_adj_axis(np.abs(dz), 2, taps), 1, taps)


# ------------------------------------------------------------------------------------------------ element-wise operations
def _per_image(v, ndim):
    v = np.asarray(v, dtype=np.float64)
    return v.reshape((v.shape[0],) + (1,) * (ndim - 2) + (v.shape[1],))


def act64(x, scale, shift):
    """lrelu(x * scale + shift), x [N]...[C], scale / shift [N][C] float32.  Returns (value, M, pre-activation); n_ops: N_ACT."""
    x = np.asarray(x, dtype=np.float64)
    s, t = _per_image(scale, x.ndim), _per_image(shift, x.ndim)
    y = x * s + t
    g = np.where(y > 0, 1.0, SLOPE)
    return y * g, (np.abs(x * s) + np.abs(t)) * g, y


def blend64(x0, sc0, sh0, x1, sc1, sh1, alpha):
    """sigmoid(alpha) act0 + (1 - sigmoid(alpha)) act1 and M (n_ops: N_BLEND)."""
    a = 1.0 / (1.0 + math.exp(-float(np.float32(alpha))))
    v0, m0, _ = act64(x0, sc0, sh0)
    v1, m1, _ = act64(x1, sc1, sh1)
    return a * v0 + (1.0 - a) * v1, a * m0 + (1.0 - a) * m1


def pool64(v, m):
    """Floor-semantics 2 x 2 maximum of [N][H][W][C] (the last odd row / column dropped).  Returns (value, M, winner 0..3 as
    2 dy + dx); M is the largest M of the window: a maximum is off by no more than its worst operand.  n_ops: N_POOL."""
    n, h, w, c = v.shape
    ho, wo = h // 2, w // 2
    win = lambda t: t[:, :2 * ho, :2 * wo].reshape(n, ho, 2, wo, 2, c).transpose(0, 1, 3, 5, 2, 4).reshape(n, ho, wo, c, 4)  # noqa: E731
    vw = win(v)
    return vw.max(-1), win(m).max(-1), vw.argmax(-1)


def norm_pool64(x, scale, shift):
    v, m, _ = act64(x, scale, shift)
    return pool64(v, m)


def norm_up64(x, scale, shift, taps=up2_taps):
    """Bilinear x2 of the activated tensor and M (n_ops: N_NORM_UP)."""
    v, m, _ = act64(x, scale, shift)
    return up2_64(v, taps)[0], up2_64(m, taps)[0]


def channel_sum64(x, out0):
    """out0 [C] + sum over pixels of x [npix][C], and M (n_ops: n_channel_sum)."""
    x = np.asarray(x, dtype=np.float64)
    out0 = np.asarray(out0, dtype=np.float64)
    return out0 + x.sum(0), np.abs(out0) + np.abs(x).sum(0)


def group_stats64(v, groups=GROUPS):
    """Per (n, group) of [N]...[C]: (sum, sum of squares, sum of |v|) as [N][groups] each."""
    v = np.asarray(v, dtype=np.float64)
    g = v.reshape(v.shape[0], -1, groups, v.shape[-1] // groups)
    return g.sum((1, 3)), (g * g).sum((1, 3)), np.abs(g).sum((1, 3))


# ------------------------------------------------------------------------------------------------ gn_finalize
def gn_finalize64(stats, gamma, beta, count, eps):
    """stats [16][N][groups][2] float64 -> (scale [N][C], shift [N][C], mean [N][groups], rstd [N][groups], M of shift).
    The slots are added in slot order, as the kernel adds them; eps is the float32 the kernel receives."""
    stats = np.asarray(stats, dtype=np.float64)
    groups, c = stats.shape[2], len(gamma)
    tot = np.zeros(stats.shape[1:], dtype=np.float64)
    for k in range(stats.shape[0]):
        tot = tot + stats[k]
    mean = tot[..., 0] / count
    var = np.maximum(tot[..., 1] / count - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + float(np.float32(eps)))
    rep = c // groups
    scale = np.asarray(gamma, dtype=np.float64)[None] * np.repeat(rstd, rep, 1)
    ms = np.repeat(mean, rep, 1) * scale
    b = np.asarray(beta, dtype=np.float64)[None]
    return scale, b - ms, mean, rstd, np.abs(b) + np.abs(ms)


def slot_stats(x, groups=GROUPS, slots=STAT_SLOTS):
    """[slots][N][groups][2]: the statistics of x [N][P][C] with the pixels dealt over the slots in unequal runs, so that every
    slot holds a different partial sum."""
    x = np.asarray(x, dtype=np.float64)
    n, p, c = x.shape
    cuts = np.linspace(0, p, slots + 1).astype(int)
    cuts[1:-1] += np.arange(1, slots) % 3 - 1
    out = np.zeros((slots, n, groups, 2))
    for k in range(slots):
        part = x[:, cuts[k]:cuts[k + 1]]
        if part.shape[1]:
            s, ss, _ = group_stats64(part, groups)
            out[k, ..., 0], out[k, ..., 1] = s, ss
    return out


GN_SIZES = ((1, 8), (3, 24), (5, 104), (2, 256))       # N * C: 8, 72, 520 (two blocks and 8 threads), 512 (two full blocks)
GN_PIXELS = 67


def gn_input(n, c, kind, seed):
    """x [N][67][C] float64, gamma, beta float32.  kind: "plain" (mean 0.3, deviation 1) or "offset" (mean 1000, deviation 1)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, GN_PIXELS, c)) + (1000.0 if kind == "offset" else 0.3)
    x = x + np.arange(n)[:, None, None] * 0.25 + (np.arange(c) // (c // GROUPS))[None, None, :] * 0.125     # every (n, group) differs
    gamma = (0.5 + rng.random(c)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(c)).astype(np.float32)
    return x, gamma, beta


def clamp_stats(n, c, groups=GROUPS):
    """Statistics of a constant tensor whose float64 ss / count - mean^2 is negative for every (n, group): the kernel's clamp is
    taken and rstd = 1 / sqrt(eps).  Returns (stats [16][N][groups][2] with everything in one slot per (n, group), count)."""
    count = float((c // groups) * GN_PIXELS)
    out = np.zeros((STAT_SLOTS, n, groups, 2))
    consts = iter(np.float64(np.float32(0.1)) * (1 + np.arange(4000)))
    for i in range(n):
        for g in range(groups):
            for v in consts:
                s, ss = count * v, count * (v * v)
                m = s / count
                if ss / count - m * m < 0:
                    out[(3 * i + 5 * g) % STAT_SLOTS, i, g] = (s, ss)
                    break
            else:
                raise AssertionError("no constant with a negative float64 variance found")
    return out, count


# ------------------------------------------------------------------------------------------------ head
def head_forward64(x, scale, shift, w, b):
    """x [N][HW][C], w [K][C], b [K] -> (logit [N][K][HW], M of the logit, sigmoid).  n_ops of the logit: n_logit(C)."""
    a, ma, _ = act64(x, scale, shift)
    w64, b64 = np.asarray(w, dtype=np.float64), np.asarray(b, dtype=np.float64)
    z = (a @ w64.T + b64).transpose(0, 2, 1)
    mz = (ma @ np.abs(w64).T + np.abs(b64)).transpose(0, 2, 1)
    return z, mz, 1.0 / (1.0 + np.exp(-z))


def sigmoid_slack(z, dz):
    """|sigmoid(z + e) - sigmoid(z)| for |e| <= dz, to second order: s' dz + |s''|_max dz^2 / 2 (|s''| <= 0.0963)."""
    s = 1.0 / (1.0 + np.exp(-z))
    return s * (1 - s) * dz + 0.05 * dz * dz


def head_backward64(x, scale, shift, w, out, dout):
    """out, dout [N][K][HW] float32 as the kernel reads them.  Returns dict: da [N][HW][C], dw [K][C], db [K] and their M."""
    a, ma, _ = act64(x, scale, shift)
    w64 = np.asarray(w, dtype=np.float64)
    o, d = np.asarray(out, dtype=np.float64), np.asarray(dout, dtype=np.float64)
    dz = d * o * (1.0 - o)
    adz = np.abs(dz)
    return {"da": np.einsum("nkp,kc->npc", dz, w64), "m_da": np.einsum("nkp,kc->npc", adz, np.abs(w64)),
            "dw": np.einsum("nkp,npc->kc", dz, a), "m_dw": np.einsum("nkp,npc->kc", adz, ma),
            "db": dz.sum((0, 2)), "m_db": adz.sum((0, 2))}


# ------------------------------------------------------------------------------------------------ seeded inputs
def stored(values, dt):
    """(tensor in the storage type, its float64 values) of float values."""
    t = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(TORCH[dt])
    return t, t.double().numpy()


NEG_SHARE = 0.3


def act_input(shape, dt, seed, neg_share=NEG_SHARE):
    """Stored x [N]...[C] with float32 scale, shift [N][C] such that the share ``neg_share`` of x * scale + shift is negative and
    no value lies within MIN_ABS_PRE of zero (asserted on every element).  Returns (tensor, float64 values, scale, shift)."""
    rng = np.random.default_rng(seed)
    n, c = shape[0], shape[-1]
    sc = (0.5 + rng.random((n, c))).astype(np.float32)
    sh = (0.3 * rng.standard_normal((n, c))).astype(np.float32)
    y = (0.05 + 1.95 * rng.random(shape)) * np.where(rng.random(shape) < neg_share, -1.0, 1.0)
    t, x64 = stored((y - _per_image(sh, len(shape))) / _per_image(sc, len(shape)), dt)
    pre = act64(x64, sc, sh)[2]
    assert (np.abs(pre) >= MIN_ABS_PRE).all(), f"pre-activation within {MIN_ABS_PRE} of zero: {np.abs(pre).min()}"
    return t, x64, sc, sh


def raw_input(shape, dt, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return stored(scale * rng.standard_normal(shape), dt)


def start_pattern(shape, mod=7):
    """Non-zero start of an accumulated float32 buffer: small integers and halves."""
    n = math.prod(shape)
    return (((np.arange(n) * 5 + 3) % mod - mod // 2) * 0.5 + 0.25).astype(np.float32).reshape(shape)


def stats_start(n, groups=GROUPS):
    k = np.arange(STAT_SLOTS * n * groups * 2, dtype=np.float64)
    return ((k * 5 + 3) % 7 - 3).reshape(STAT_SLOTS, n, groups, 2)


# ------------------------------------------------------------------------------------------------ case tables
N_IMAGES = 3
C_CASES = ("vec", 24, 32)


def channels(cc, dt):
    return VEC[dt] if cc == "vec" else cc


# upsample2_stats (n, c or "vec", h, w): what each reaches
UP_STATS_CASES = {
    "h1": (3, 8, 1, 5),                  # one source row: y0 == y1 everywhere (8 channels: one per group)
    "w1": (3, 8, 5, 1),                  # one source column
    "c24": (3, 24, 7, 9),                # C / VEC not a power of two: idle threads (pl >= ppb)
    "wrap": (3, 64, 33, 33),             # float32: 4356 pixels in blocks of 256 -> 18 blocks per image, the 16 slots wrap
    "two_blocks_tail": (3, 32, 23, 23),  # a second (16-bit) / third (float32) block with a short tail
}
# upsample2_adjoint (n, c or "vec", h, w)
ADJ_CASES = {
    "1x1": (3, "vec", 1, 1), "1x5": (3, "vec", 1, 5), "5x1": (3, "vec", 5, 1), "2x2": (3, "vec", 2, 2), "3x2": (3, 24, 3, 2),
    "7x9": (3, 24, 7, 9),
    "multi_block_odd_grid": (3, 32, 37, 45),      # 19 x 23 blocks of 2 x 2 outputs (odd width): 437 > 256 (16-bit) / 128 (float32) per block
}
# channel_sum (c or "vec", pixels): one pixel; a block and a tail; several blocks
CHANNEL_SUM_C = ("vec", 24, 256)
CHANNEL_SUM_PIX = ("one", "block_tail", "blocks")


def channel_sum_pixels(c, dt, kind):
    blk = (256 // (c // VEC[dt])) * 32
    return {"one": 1, "block_tail": blk + 5, "blocks": 3 * blk + 7}[kind]


HEAD_K = (1, 2, 3, 4)
HEAD_C = ("vec", 16, 24, 128)
HEAD_FWD_HW = (1, 255, 257)          # blocks of 256 pixels
HEAD_BWD_HW = (2047, 2049)           # blocks of 2048 pixels

# stem: (dtype, Cout, H, W, what it reaches)
STEM_CASES = (
    ("f32", 24, 11, 21, "nvec 6: general epilogue, idle threads"), ("bf16", 24, 11, 21, "nvec 3"), ("f16", 48, 11, 21, "nvec 6"),
    ("f32", 48, 9, 13, "nvec 12"), ("bf16", 48, 9, 13, "nvec 6"),
    ("bf16", 256, 5, 9, "general epilogue with nvec 32, a power of two (Cout > 128)"),
    ("f32", 512, 3, 71, "ppblk < W and no multiple of W: 2 lanes, forward 64 < 71 -> 72 pixels"),
    ("f32", 32, 7, 1, "W = 1"), ("bf16", 32, 1, 19, "H = 1"), ("f16", 24, 1, 1, "one pixel"),
)
