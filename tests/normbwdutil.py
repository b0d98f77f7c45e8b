"""GroupNorm(8, C) + LeakyReLU(0.2) backward (csrc/norm_bwd*.hip): a float64 specification with derived error bounds, inputs
under which the mean terms of the backward are as large as the direct term, and a float32 restatement of the kernels'
arithmetic with switchable defects ("mutants").  Helper module of test_norm_bwd_host.py and test_gpu_norm_bwd.py.

Every backward kernel computes, per image n and channel c of group k,

    dx = g A + x B + C,    A = rstd gamma,   B = -rstd^2 S2,   C = mean rstd^2 S2 - rstd S1,
    g  = LeakyReLU'(pre) * sum over consumers of dL/dact,        pre = x scale + shift,
    S1 = mean over the group of g gamma,   S2 = mean over the group of g gamma xhat,   xhat = (x - mean) rstd,
    dbeta = sum g,   dgamma = sum g xhat   (over images and pixels).

Rules of the specification: the 2x2 max-pool routes its gradient to the FIRST maximum of the activation in scan order
(aten); LeakyReLU' is 1 where pre > 0 and 0.2 otherwise (so 0.2 at pre == 0).

The bounds (``spec``), derived from the formula, never from device output.  u_st = unit roundoff of the storage type
(2^-8 bf16, 2^-11 fp16, 2^-24 fp32), u = 2^-24, K = 16.
  reduced quantities   a sum of n float32 terms t_i evaluated in any order is within n u sum |t_i| of the exact sum (the
                       bound test_gpu_blend_bwd.ref_f64 uses).  The kernels form sum g xhat as rstd (sum g x - mean sum g)
                       per thread, so its terms are rstd g x and rstd mean g.  When pass 1 stores g in the storage type and
                       sums the stored values, every term carries one more relative error u_st.  Elements left out of the
                       comparison (gate band, below) may take either branch: their whole |dL/dact| is added.
  S1, S2               the same bound over the group (n = count), divided by count: dS1 = u sum |gamma g|, dS2 likewise.
  dx, per element      u_st |dx|                          the final store (plus half a subnormal of the storage type),
                     + u_st |g A|                         when the launch sequence stores g,
                     + K u (|g|_abs |A| + |x B| + |mean rstd^2 S2| + |rstd S1|)
                                                          the float32 evaluation: at most 9 gathered consumer terms, the
                                                          blend weight (sigmoid through __expf), three products, two sums;
                                                          |g|_abs sums the consumer terms by magnitude and C is taken term by
                                                          term, because float32 rounds each product before the subtraction,
                     + |A| (weight slack of the bilinear adjoint)   its float32 source coordinate Y (h-1)/(2h-1) is off by up
                                                          to 4 (2h) u, which moves weight between neighbouring taps,
                     + |x| dB + dC,   dB = rstd^2 dS2,   dC = |mean| rstd^2 dS2 + rstd dS1.

Gate band: the device forms scale = fl(gamma rstd), shift = fl(beta - fl(mean scale)), pre = fl(x scale + shift): at most four
roundings relative to |x scale| + |mean scale| + |beta| (|shift| term by term, it is a rounded difference).  An element whose
float64 |pre| is within 4 u of that sum from zero may take either branch on the device and is left out - unless pre is zero
by construction (x scale, mean scale and beta all exactly 0: the device gets an exact zero too).  A pool window is left out
when an activation within the two elements' bands of the window's maximum comes from a different x (equal x, or scale == 0,
give bit-equal activations on the device: an exact tie, resolved by the first-maximum rule).  At most CAP = 0.05 % of a
case's elements may be left out.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

G = 8
EPS = 1e-5
SLOPE = 0.2
U32 = 2.0 ** -24
KF = 16
TBAND = 4
CAP = 5e-4
F32, BF16, F16 = 0, 1, 2                     # the library's dtype codes (mri_superresolution_amd._lib)
TDT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
UNIT = {F32: 2.0 ** -24, BF16: 2.0 ** -8, F16: 2.0 ** -11}
HALF_SUBNORMAL = {F32: 2.0 ** -150, BF16: 2.0 ** -134, F16: 2.0 ** -25}
DTNAME = {F32: "fp32", BF16: "bf16", F16: "fp16"}


def rounded(a: np.ndarray, dt) -> np.ndarray:
    """``a`` rounded once (to nearest even) to the storage type, as float64."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    return t.to(torch.float32).to(TDT[dt]).to(torch.float64).numpy()


def sigmoid(v: float) -> float:
    return 1.0 / (1.0 + math.exp(-v))


# ------------------------------------------------------------------------------------------------ consumers
class Cons:
    """One consumer of the node's activation.  kind "plain": da (N, C_total, Hc, Wc), the node at channels
    [c_off, c_off + C) and pixel offset ``off`` (zero padding behind it); "pool": da (N, C, H//2, W//2) of MaxPool2d(2);
    "up": da (N, C, 2H, 2W) of the bilinear x2 (align_corners=True); "head": da (N, H, W) = dL/dout of
    out = sigmoid(sum_c act w_c + b).  ``wm``: 0 plain, 1 weighted sigmoid(alpha), 2 weighted 1 - sigmoid(alpha)."""

    def __init__(self, kind, da, c_off=0, off=(0, 0), wm=0, head_w=None, head_b=0.0):
        assert kind in ("plain", "pool", "up", "head")
        self.kind, self.da, self.c_off, self.off, self.wm = kind, np.asarray(da, dtype=np.float64), c_off, off, wm
        self.head_w = None if head_w is None else np.asarray(head_w, dtype=np.float64)
        self.head_b = float(head_b)


def up2_matrix(h: int, slack: float = 0.0) -> np.ndarray:
    """(2h, h) matrix of the bilinear x2 with align_corners=True: src(Y) = Y (h-1)/(2h-1), in exact integer arithmetic.
    ``slack`` > 0: instead, that much weight on every tap a float32 evaluation of src could touch."""
    m = np.zeros((2 * h, h))
    for y2 in range(2 * h):
        num, den = y2 * (h - 1), 2 * h - 1
        i0, w1 = num // den, (num % den) / den
        i1 = min(i0 + 1, h - 1)
        if slack:
            for i in range(max(i0 - 1, 0), min(i0 + 2, h - 1) + 1):
                m[y2, i] = slack
        else:
            m[y2, i0] += 1.0 - w1
            m[y2, i1] += w1
    return m


def windows(a: np.ndarray) -> np.ndarray:
    """(N, C, H, W) -> (N, C, H//2, W//2, 4), window element q = 2 dy + dx (the scan order of the pool)."""
    n, c, h, w = a.shape
    hp, wp = h // 2, w // 2
    return a[:, :, :2 * hp, :2 * wp].reshape(n, c, hp, 2, wp, 2).transpose(0, 1, 2, 4, 3, 5).reshape(n, c, hp, wp, 4)


def unwindows(v: np.ndarray, h: int, w: int) -> np.ndarray:
    """Inverse of ``windows``; an odd last row / column is filled with zeros."""
    n, c, hp, wp, _ = v.shape
    out = np.zeros((n, c, h, w), dtype=v.dtype)
    out[:, :, :2 * hp, :2 * wp] = v.reshape(n, c, hp, wp, 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(n, c, 2 * hp, 2 * wp)
    return out


def route(key: np.ndarray, mode: str = "first") -> np.ndarray:
    """0/1 weights (.., 4) of the window elements that take the pooled gradient: the first / last / all maxima of key."""
    eq = key == key.max(-1, keepdims=True)
    if mode == "all":
        return eq
    if mode == "last":
        return eq & (np.cumsum(eq[..., ::-1], -1)[..., ::-1] == 1)
    assert mode == "first"
    return eq & (np.cumsum(eq, -1) == 1)


def gather(cons, ds, sel, a, shape, dtype, slack=False):
    """dL/dact of the node from its consumers' gradients ``ds`` (one array per consumer, in ``dtype``; for a head
    consumer the pair (dz (N, H, W), w (C))), summed in consumer order.  ``sel``: the pool's routing weights
    (N, C, H//2, W//2, 4); ``a``: sigmoid(alpha).  ``slack``: only the bilinear adjoint's weight slack (see module docstring)."""
    n, c, h, w = shape
    out = np.zeros(shape, dtype=dtype)
    for k, d in zip(cons, ds):
        wgt = dtype(1.0 if k.wm == 0 else (a if k.wm == 1 else 1.0 - a))
        if k.kind == "up":
            oy, ox = k.off
            dd = d[:, k.c_off:k.c_off + c, oy:oy + 2 * h, ox:ox + 2 * w]
            if slack:
                sy, sx = 4 * 2 * h * U32, 4 * 2 * w * U32
                my, mx = up2_matrix(h), up2_matrix(w)
                full = np.einsum("Yy,ncYX,Xx->ncyx", my + up2_matrix(h, sy), dd, mx + up2_matrix(w, sx))
                out += wgt * (full - np.einsum("Yy,ncYX,Xx->ncyx", my, dd, mx)).astype(dtype)
            else:
                out += wgt * np.einsum("Yy,ncYX,Xx->ncyx", up2_matrix(h).astype(dtype), dd, up2_matrix(w).astype(dtype)).astype(dtype)
        elif slack:
            continue
        elif k.kind == "plain":
            oy, ox = k.off
            hv, wv = min(h, d.shape[2] - oy), min(w, d.shape[3] - ox)
            out[:, :, :hv, :wv] += wgt * d[:, k.c_off:k.c_off + c, oy:oy + hv, ox:ox + wv]
        elif k.kind == "pool":
            out += unwindows(sel.astype(dtype) * (wgt * d)[..., None], h, w)
        else:
            dz, hw = d
            out += dz[:, None] * hw[None, :, None, None]
    return out


# ------------------------------------------------------------------------------------------------ the case
class Case:
    """Inputs of one node: x (N, C, H, W), gamma, beta, consumers - float64 arrays holding storage-rounded values."""

    def __init__(self, name, dt, x, gamma, beta, cons, alpha=None, meanrstd=None, ties=False, kink=False):
        self.name, self.dt, self.x, self.gamma, self.beta, self.cons = name, dt, x, gamma, beta, cons
        self.alpha, self.meanrstd, self.ties, self.kink = alpha, meanrstd, ties, kink
        self.stores_g = False          # the launch sequence this case goes through stores g in the storage type
        self.shuffled = False          # the node's producer is pixel-shuffled (its bias gradient falls out of pass 2)
        self.shape = x.shape

    @property
    def pooled(self):
        return any(k.kind == "pool" for k in self.cons)

    @property
    def count(self):
        n, c, h, w = self.shape
        return float((c // G) * h * w)

    def stats32(self):
        """(mean, rstd), each (N, G), as mrisr_gn_finalize leaves them in float32 (from exact float64 sums), or the pair
        handed to the case."""
        if self.meanrstd is not None:
            return self.meanrstd
        n, c, h, w = self.shape
        xg = self.x.reshape(n, G, -1)
        mean = xg.sum(2) / self.count
        var = np.maximum((xg * xg).sum(2) / self.count - mean * mean, 0.0)
        rstd = (1.0 / np.sqrt(var + np.float64(np.float32(EPS)))).astype(np.float32)
        return mean.astype(np.float32).astype(np.float64), rstd.astype(np.float64)


def _per_channel(v, c):
    """(N, G) -> (N, C, 1, 1)."""
    return np.repeat(v, c // G, axis=1)[:, :, None, None]


def _head_parts(k: Cons, act):
    z = np.einsum("nchw,c->nhw", act, k.head_w) + k.head_b
    o = 1.0 / (1.0 + np.exp(-z))
    return o, k.da * o * (1.0 - o)


def spec(case: Case, meanrstd=None, stores_g=False, shuffled=False):
    """The float64 specification of the node's backward with its bounds (module docstring).  ``meanrstd``: (mean, rstd),
    each (N, G), used in place of the statistics of x - the kernels take their meanrstd argument as given.  Returns a dict:
    dx, dgamma, dbeta (+ dbias with ``shuffled``, dalpha with a blend-weighted first consumer, head_dw / head_db / head_out
    with a head consumer), ``<name>_b`` the bound of each, ``excluded`` (elements left out of the dx comparison), ``recv``
    (elements that take the pooled gradient), g / g_b (what pass 1 stores), S1, S2 (N, G)."""
    x, dt = case.x, case.dt
    n, c, h, w = case.shape
    gs, ust = c // G, UNIT[dt]
    if meanrstd is None:
        if case.meanrstd is not None:
            meanrstd = case.meanrstd
        else:
            xg = x.reshape(n, G, -1)
            mean = xg.mean(2)
            meanrstd = (mean, 1.0 / np.sqrt(((xg - mean[..., None]) ** 2).mean(2) + EPS))
    mean, rstd = _per_channel(meanrstd[0], c), _per_channel(meanrstd[1], c)
    gam, bet = case.gamma.reshape(1, c, 1, 1), case.beta.reshape(1, c, 1, 1)
    xhat = (x - mean) * rstd
    scale = gam * rstd
    shift = bet - mean * scale
    pre = x * scale + shift
    mag = np.abs(x * scale) + np.abs(mean * scale) + np.abs(bet)
    band = TBAND * U32 * mag
    by_construction = (x * scale == 0) & (mean * scale == 0) & (bet == 0)
    excluded = (np.abs(pre) <= band) & ~by_construction
    deriv = np.where(pre > 0, 1.0, SLOPE)
    act = np.where(pre > 0, pre, SLOPE * pre)
    a = sigmoid(case.alpha) if case.alpha is not None else 0.0

    r, sel, recv = {}, None, np.zeros(case.shape, dtype=bool)
    if case.pooled:
        aw, bw, xw = windows(act), windows(band), windows(x)
        sel = route(aw, "first")
        first = lambda v: (v * sel).sum(-1, keepdims=True)        # noqa: E731
        cand = aw >= aw.max(-1, keepdims=True) - (bw + first(bw))
        same = (xw == first(xw)) | (windows(np.broadcast_to(scale, case.shape)) == 0)
        excluded |= unwindows(np.broadcast_to((cand & ~same).any(-1, keepdims=True), aw.shape), h, w).astype(bool)
        recv = unwindows(sel, h, w).astype(bool)
    ds, dabs, dall = [], [], []
    for k in case.cons:
        if k.kind == "head":
            o, dz = _head_parts(k, act)
            r["head_out"] = o
            terms = dz[:, None] * act
            r["head_dw"], r["head_db"] = terms.sum((0, 2, 3)), dz.sum().reshape(1)
            nt = n * h * w
            r["head_dw_b"] = (nt + KF) * U32 * (np.abs(dz)[:, None] * mag).sum((0, 2, 3))
            r["head_db_b"] = (nt + KF) * U32 * np.abs(dz).sum().reshape(1)
            ds.append((dz, k.head_w))
            dabs.append((np.abs(dz), np.abs(k.head_w)))
        else:
            ds.append(k.da)
            dabs.append(np.abs(k.da))
    f64 = np.float64
    gact = gather(case.cons, ds, sel, a, case.shape, f64)
    gabs = gather(case.cons, dabs, sel, a, case.shape, f64)
    gall = gather(case.cons, dabs, None if sel is None else np.ones_like(sel), a, case.shape, f64)     # either branch, any routing
    gslack = gather(case.cons, dabs, sel, a, case.shape, f64, slack=True)
    g = gact * deriv
    r["g"], r["g_b"] = g, ust * np.abs(g) + HALF_SUBNORMAL[dt] + KF * U32 * gabs * deriv + gslack * deriv
    loose = np.where(excluded, gall, 0.0)                       # what a left-out element may add to or take from a sum
    su = ust if stores_g else 0.0

    nt = n * h * w
    t_b, t_g = np.abs(g), rstd * np.abs(g) * (np.abs(x) + np.abs(mean))
    r["dbeta"], r["dgamma"] = g.sum((0, 2, 3)), (g * xhat).sum((0, 2, 3))
    r["dbeta_b"] = (nt * U32 + su) * t_b.sum((0, 2, 3)) + loose.sum((0, 2, 3))
    r["dgamma_b"] = (nt * U32 + su) * t_g.sum((0, 2, 3)) + (loose * np.abs(xhat)).sum((0, 2, 3))

    grp = lambda v: v.reshape(n, G, -1)          # noqa: E731
    cnt = case.count
    s1, s2 = grp(g * gam).mean(2), grp(g * gam * xhat).mean(2)
    ds1 = ((cnt + KF) * U32 + su) * grp(np.abs(gam) * t_b).sum(2) / cnt + grp(np.abs(gam) * loose).sum(2) / cnt
    ds2 = ((cnt + KF) * U32 + su) * grp(np.abs(gam) * t_g).sum(2) / cnt + grp(np.abs(gam) * loose * np.abs(xhat)).sum(2) / cnt
    r["S1"], r["S2"] = s1, s2
    S1, S2, dS1, dS2 = (_per_channel(v, c) for v in (s1, s2, ds1, ds2))
    A, B = rstd * gam, -rstd * rstd * S2
    c1, c2 = mean * rstd * rstd * S2, rstd * S1
    dx = g * A + x * B + (c1 - c2)
    dB, dC = rstd * rstd * dS2, np.abs(mean) * rstd * rstd * dS2 + rstd * dS1
    r["dx"] = dx
    r["dx_b"] = (ust * np.abs(dx) + HALF_SUBNORMAL[dt] + su * np.abs(g * A)
                 + KF * U32 * (gabs * deriv * np.abs(A) + np.abs(x * B) + np.abs(c1) + np.abs(c2))
                 + np.abs(A) * deriv * gslack + np.abs(x) * dB + dC)
    r["A"], r["B"], r["C"] = np.broadcast_to(A, case.shape), np.broadcast_to(B, case.shape), np.broadcast_to(c1 - c2, case.shape)
    r["excluded"], r["recv"] = excluded, recv
    if case.pooled:      # the pooled gradient (times LeakyReLU') an element carries, and would carry if it were the window's recipient
        pk = [k for k in case.cons if k.kind == "pool"]
        r["pool_part"] = gather(pk, [k.da for k in pk], sel, a, case.shape, f64) * deriv
        r["pool_hyp"] = np.abs(gather(pk, [k.da for k in pk], np.ones_like(sel), a, case.shape, f64) * deriv)
    if shuffled:      # the producing conv's bias gradient: channel sums of the un-shuffled dx, summed from the STORED values
        un = lambda v: F.pixel_unshuffle(torch.from_numpy(np.ascontiguousarray(v)), 2).numpy()      # noqa: E731
        r["dbias"] = un(dx).sum((0, 2, 3))
        each = r["dx_b"] + np.where(excluded, np.abs(A) * gall, 0.0)
        r["dbias_b"] = (n * (h // 2) * (w // 2)) * U32 * np.abs(un(dx)).sum((0, 2, 3)) + un(each).sum((0, 2, 3))
    k0 = case.cons[0]
    if k0.wm and k0.kind == "plain":       # this branch's term of dL/dalpha: +-sigmoid'(alpha) sum d act
        d0 = gather([Cons("plain", k0.da, k0.c_off, k0.off)], [k0.da], None, a, case.shape, f64)
        sgn = 1.0 if k0.wm == 1 else -1.0
        r["dalpha"] = np.array([sgn * a * (1 - a) * (d0 * act).sum()])
        r["dalpha_b"] = np.array([(x.size + KF) * U32 * a * (1 - a) * (np.abs(d0) * mag).sum()
                                  + a * (1 - a) * (np.abs(d0) * np.where(excluded, band, 0.0)).sum()])
    return r


# ------------------------------------------------------------------------------------------------ autograd check
def autograd_reference(case: Case):
    """float64 autograd of F.group_norm + F.leaky_relu + the consumer transforms (no ties, no kinks in ``case``)."""
    n, c, h, w = case.shape
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))      # noqa: E731
    x, gam, bet = t(case.x).requires_grad_(True), t(case.gamma).requires_grad_(True), t(case.beta).requires_grad_(True)
    alpha = torch.tensor(float(case.alpha if case.alpha is not None else 0.0), dtype=torch.float64, requires_grad=True)
    act = F.leaky_relu(F.group_norm(x, G, gam, bet, EPS), SLOPE)
    sg = torch.sigmoid(alpha)
    loss, extra = 0, {}
    for k in case.cons:
        wgt = 1.0 if k.wm == 0 else (sg if k.wm == 1 else 1 - sg)
        da = t(k.da)
        if k.kind == "plain":
            oy, ox = k.off
            hc, wc = da.shape[2:]
            padded = F.pad(act, [ox, max(wc - w - ox, 0), oy, max(hc - h - oy, 0)])[:, :, :hc, :wc]
            loss = loss + (wgt * padded * da[:, k.c_off:k.c_off + c]).sum()
        elif k.kind == "pool":
            loss = loss + (wgt * F.max_pool2d(act, 2) * da).sum()
        elif k.kind == "up":
            oy, ox = k.off
            up = F.interpolate(act, scale_factor=2, mode="bilinear", align_corners=True)
            loss = loss + (wgt * up * da[:, k.c_off:k.c_off + c, oy:oy + 2 * h, ox:ox + 2 * w]).sum()
        else:
            hw, hb = t(k.head_w).requires_grad_(True), torch.tensor([k.head_b], dtype=torch.float64, requires_grad=True)
            out = torch.sigmoid((act * hw.view(1, c, 1, 1)).sum(1) + hb)
            loss = loss + (out * da).sum()
            extra = {"head_dw": hw, "head_db": hb}
    loss.backward()
    r = {"dx": x.grad.numpy(), "dgamma": gam.grad.numpy(), "dbeta": bet.grad.numpy()}
    if alpha.grad is not None:
        r["dalpha"] = alpha.grad.numpy().reshape(1)
    r.update({k: v.grad.numpy() for k, v in extra.items()})
    return r


# ------------------------------------------------------------------------------------------------ inputs
def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64).numpy()


def _rand(gen, *shape):
    return torch.rand(*shape, generator=gen, dtype=torch.float64).numpy()


def make_case(name, dt, shape, kinds, seed, *, ties=False, kink=False, alpha=None, wm=0, gamma_sign=None, up_scale=1.0,
              zero_gamma=None, a0=1.5, b0=2.25):
    """A case with power: group means of x clearly non-zero, gamma of mixed sign
    with |gamma| in [0.8, 1.5] (pooled cases: channel 3 exactly 0), upstream gradients of non-zero mean and correlated
    with xhat: s (a0 + b0 tanh(xhat)) + 0.5 randn with s = sign(gamma) - the sign follows gamma because S1 and S2 average g gamma,
    which would otherwise cancel inside a group of mixed sign.  With u = s xhat ~ N(0, 1) and LeakyReLU' = 1 for u > 0, else 0.2:
    S1 ~ |gamma| (0.6 a0 + 0.24 s b0), S2 ~ |gamma| (0.32 s a0 + 0.36 b0); b0 / a0 = 1.5 keeps both positive for either sign.
    ``kinds``: consumer kinds in launch order - "plain" (own geometry, channel window 8 of C + 8), "plain0" (own geometry, no
    window), "pad" (padded: (H + 1, W + 2), offset (0, 1), channel window 16), "pool", "up", "head".
    ties: x on the grid k/4, |k| <= 6, both ends of it heavy (so that most windows tie at their maximum whatever the sign of
    gamma) and unequally so (the group means stay away from zero); pooled gradients of magnitude >= 0.5 (in the kink cases too).
    kink: x from {-1, -1/2, 0, 0, 1/2, 1}, beta = 0 and HANDED statistics mean 0, rstd = 1/sqrt(1 + eps): pre is exactly +-0 on
    a third of the elements."""
    gen = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    if ties:
        levels, prob = np.array([-6, -3, -1, 0, 2, 4, 6]) / 4, np.array([0.40, 0.03, 0.03, 0.03, 0.03, 0.03, 0.45])
        x = levels[np.searchsorted(np.cumsum(prob), _rand(gen, *shape) * prob.sum())]
    elif kink:
        x = np.array([-1, -0.5, 0, 0, 0.5, 1.0])[torch.randint(0, 6, shape, generator=gen).numpy()]
    else:
        x = rounded(1.5 * _randn(gen, *shape) + 0.7, dt)
    sign = np.where(_rand(gen, c) < 0.5, -1.0, 1.0)
    sign[0], sign[1] = 1.0, -1.0
    if gamma_sign is not None:
        sign = gamma_sign
    gamma = np.float64(np.float32(sign * (0.8 + 0.7 * _rand(gen, c))))
    pooled = "pool" in kinds
    if (pooled if zero_gamma is None else zero_gamma):
        gamma[3] = 0.0
    beta = np.zeros(c) if kink else np.float64(np.float32(0.1 * _randn(gen, c)))
    meanrstd = None
    if kink:
        meanrstd = (np.zeros((n, G)), np.full((n, G), np.float64(np.float32(1.0 / math.sqrt(1.0 + np.float64(np.float32(EPS)))))))
    case = Case(name, dt, x, gamma, beta, [], alpha=alpha, meanrstd=meanrstd, ties=ties, kink=kink)
    mean, rstd = case.stats32()
    xhat = (x - _per_channel(mean, c)) * _per_channel(rstd, c)
    s = np.where(gamma < 0, -1.0, 1.0).reshape(1, c, 1, 1)
    corr = s * (a0 + b0 * np.tanh(xhat))                 # (N, C, H, W)
    corr_far = s * (a0 / 3 + b0 * np.tanh(xhat))         # pool / bilinear: the window average dilutes the part that follows xhat
    for kind in kinds:
        if kind in ("plain", "plain0", "pad"):
            coff, (oy, ox), (hc, wc) = {"plain": (8, (0, 0), (h, w)), "plain0": (0, (0, 0), (h, w)), "pad": (16, (0, 1), (h + 1, w + 2))}[kind]
            da = 0.5 * _randn(gen, n, c + coff, hc, wc)
            hv, wv = min(h, hc - oy), min(w, wc - ox)
            da[:, coff:, oy:oy + hv, ox:ox + wv] += corr[:, :, :hv, :wv]
            case.cons.append(Cons("plain", rounded(up_scale * da, dt), coff, (oy, ox), wm))
        elif kind == "pool":
            cp = windows(corr_far).mean(-1)
            if ties or kink:
                da = s * (0.5 + np.abs(cp) + 0.25 * _rand(gen, *cp.shape))
            else:
                da = 4.0 * cp + 0.5 * _randn(gen, *cp.shape)
            case.cons.append(Cons("pool", rounded(up_scale * da, dt), 0, (0, 0), wm))
        elif kind == "up":
            da = 0.25 * (np.repeat(np.repeat(s * (0.6 * a0 + b0 * np.tanh(xhat)), 2, 2), 2, 3) + 0.5 * _randn(gen, n, c, 2 * h, 2 * w))
            case.cons.append(Cons("up", rounded(up_scale * da, dt), 0, (0, 0), wm))
        else:
            assert kind == "head"
            hw = np.float64(np.float32(s.reshape(c) * (0.3 + 0.2 * _rand(gen, c))))
            dout = 8.0 * (1.0 + 0.5 * np.tanh((s * xhat).mean(1)) + 0.25 * _randn(gen, n, h, w))
            case.cons.append(Cons("head", np.float64(np.float32(dout)), head_w=hw, head_b=0.1))
    return case


# ------------------------------------------------------------------------------------------------ float32 restatement
MUTANTS = ("drop_B", "drop_C", "next_group", "mean_sign", "kink_one", "tie_last", "tie_all", "pool_on_x", "inv_count_gs",
           "dgamma_gx")


def mutant_applies(m, case: Case):
    if m == "kink_one":
        return case.kink
    if m in ("tie_last", "tie_all"):
        return case.ties and case.pooled
    if m == "pool_on_x":
        return case.pooled and not case.kink
    if m in ("mean_sign", "dgamma_gx"):
        return not case.kink            # the handed mean is exactly 0 and rstd 1 - 5e-6 there: both compute the correct value
    return True


def _sum_chunks(terms_a, terms_b, mean, rstd, perm, chunk=16):
    """Per (n, c): sum g and rstd (sum g x - mean sum g) as the kernels form them - float32, a thread's ``chunk`` pixels first
    (in the order ``perm``), then the partial sums one after the other."""
    n, c, p = terms_a.shape
    pad = (-p) % chunk
    f = lambda t: np.pad(t[:, :, perm], ((0, 0), (0, 0), (0, pad))).reshape(n, c, -1, chunk)       # noqa: E731
    acc = lambda t: np.add.accumulate(t, axis=-1, dtype=np.float32)[..., -1]        # noqa: E731
    sa, sb = acc(f(terms_a)), acc(f(terms_b))
    raw = acc(sb)
    sb = (rstd * (sb - mean * sa)).astype(np.float32)
    return acc(sa), acc(sb), raw


def restate(case: Case, rng: np.random.Generator, mutant=None, stores_g=False):
    """The kernels' arithmetic in float32 (numpy): pass 1 (g, the per-(n, c) sums in a random order), the coefficients, pass 2,
    with the storage rounding of g (``stores_g``) and dx.  ``mutant``: one of MUTANTS, a deliberate defect."""
    f32 = np.float32
    n, c, h, w = case.shape
    gs, dt = c // G, case.dt
    m32, r32 = (_per_channel(v, c).astype(f32) for v in case.stats32())
    x = case.x.astype(f32)
    gam, bet = case.gamma.astype(f32).reshape(1, c, 1, 1), case.beta.astype(f32).reshape(1, c, 1, 1)
    sc = gam * r32
    sh = bet - m32 * sc
    pre = x * sc + sh
    act = np.maximum(pre, f32(SLOPE) * pre)
    deriv = np.where((pre >= 0) if mutant == "kink_one" else (pre > 0), f32(1.0), f32(SLOPE))
    a = f32(sigmoid(case.alpha)) if case.alpha is not None else f32(0)
    sel = None
    if case.pooled:
        sel = route(windows(x if mutant == "pool_on_x" else act), {"tie_last": "last", "tie_all": "all"}.get(mutant, "first"))
    ds = []
    for k in case.cons:
        if k.kind == "head":
            z = np.einsum("nchw,c->nhw", act.astype(np.float64), k.head_w) + k.head_b
            o = (1.0 / (1.0 + np.exp(-z))).astype(f32)            # the forward's float32 output
            ds.append((k.da.astype(f32) * o * (f32(1) - o), k.head_w.astype(f32)))
        else:
            ds.append(k.da.astype(f32))
    g = gather(case.cons, ds, sel, a, case.shape, f32) * deriv
    if stores_g:
        g = rounded(g, dt).astype(f32)
    perm = rng.permutation(h * w)
    fl = lambda t: t.reshape(n, c, h * w)        # noqa: E731
    ra, rb, raw = _sum_chunks(fl(g), fl(g * x), m32[:, :, 0], r32[:, :, 0], perm)
    acc = lambda t, ax: np.add.accumulate(t, axis=ax, dtype=f32).take(-1, axis=ax)      # noqa: E731
    out = {"dbeta": acc(ra, 0).astype(np.float64), "dgamma": acc(raw if mutant == "dgamma_gx" else rb, 0).astype(np.float64)}
    g1 = case.gamma.astype(f32).reshape(1, c)
    inv = f32(1.0 / case.count) * (f32(gs) if mutant == "inv_count_gs" else f32(1))
    s1 = acc((g1 * ra).reshape(n, G, gs), 2) * inv
    s2 = acc((g1 * rb).reshape(n, G, gs), 2) * inv
    if mutant == "next_group":
        s1, s2 = np.roll(s1, -1, axis=1), np.roll(s2, -1, axis=1)
    S1, S2 = _per_channel(s1, c), _per_channel(s2, c)
    ca, cb = r32 * gam, -r32 * r32 * S2
    cc = (-m32 if mutant == "mean_sign" else m32) * r32 * r32 * S2 - r32 * S1
    if mutant == "drop_B":
        dx = g * ca + cc
    elif mutant == "drop_C":
        dx = g * ca + x * cb
    else:
        dx = g * ca + x * cb + cc
    out["dx"] = rounded(dx, dt)
    out["g"] = g.astype(np.float64)
    return out


def worst_ratio(got, ref, bound, keep=None):
    """max |got - ref| / bound over the elements of ``keep`` (all by default); inf for a non-finite result."""
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    ratio = np.abs(got - ref) / bound
    if keep is not None:
        ratio = ratio[keep]
    return float(ratio.max()) if ratio.size else 0.0


def ratios(out: dict, ref: dict):
    """Worst error-to-bound ratio per output present in both (dx over the elements that are not left out)."""
    r = {}
    for name in ("dx", "dgamma", "dbeta", "dbias", "dalpha", "head_dw", "head_db"):
        if name in out and name in ref:
            r[name] = worst_ratio(out[name], ref[name], ref[name + "_b"], ~ref["excluded"] if name == "dx" else None)
    return r


def routing_sets(out: dict, ref: dict):
    """Which elements took the pooled gradient, read off the stored g (when ``out`` has one) or off dx: an element's value minus
    everything but the pooled share is that share (>= 0.1 |A| in the ties and kink cases, whose pooled gradients have magnitude
    >= 0.5) for the recipient and 0 for the other three, each within the element's bound.  Elements whose hypothetical share is
    not above 4 bounds cannot be told apart and are left out (among them every channel with gamma == 0 when read off dx).
    Returns (got, want, live): the device's set, the specification's, and the elements that can be told apart."""
    if "g" in out:
        resid, hyp, floor_ = np.abs(out["g"] - (ref["g"] - ref["pool_part"])), ref["pool_hyp"], ref["g_b"]
    else:
        resid, hyp, floor_ = np.abs(out["dx"] - (ref["dx"] - ref["pool_part"] * ref["A"])), ref["pool_hyp"] * np.abs(ref["A"]), ref["dx_b"]
    live = hyp > 4 * floor_
    return (resid > 0.5 * hyp) & live, ref["recv"] & live, live


# ------------------------------------------------------------------------------------------------ the cases of both tests
def case_list(dt):
    """The cases of the per-node launch sequences, by name.  Together with unshuffle_cases, blend_cases and forward_cases
    these are ALL the inputs test_gpu_norm_bwd.py runs (it builds none of its own), and test_norm_bwd_host.py goes through
    every one of them (all_cases), so the host test proves the power of exactly those inputs."""
    A, B, P, T, O = (2, 32, 18, 26), (2, 32, 19, 27), (2, 32, 8, 32), (1, 16, 6, 40), (3, 32, 72, 64)
    # a pool-only node hands its gradient to the window's largest u = s xhat: S1 follows s and S2 does not, so a group of
    # mixed sign would cancel one of them - the sign is mixed BETWEEN the groups there (and for the head, whose gradient is
    # the same for every channel up to w_c)
    bygroup = lambda c: np.repeat(np.array([1.0, -1.0] * (G // 2)), c // G)          # noqa: E731
    mk = lambda name, shape, kinds, seed, **kw: make_case(name, dt, shape, kinds, seed, **({"gamma_sign": bygroup(shape[1])} if kinds in (["pool"], ["head"]) else {}), **kw)       # noqa: E731
    cases = []
    for tag, kw in (("", {}), ("ties_", {"ties": True}), ("kink_", {"kink": True})):
        cases += [
            mk(tag + "pad_A", A, ["pad"], 11, **kw), mk(tag + "pad+pool_A", A, ["pad", "pool"], 12, **kw),
            mk(tag + "up_A", A, ["up"], 13, **kw),
            mk(tag + "same_A", A, ["plain"], 14, **kw), mk(tag + "same2_A", A, ["plain", "plain0"], 15, **kw),
            mk(tag + "pool_A", A, ["pool"], 16, **kw), mk(tag + "pool+skip_A", A, ["plain", "pool"], 17, **kw),
            mk(tag + "pad+pool_B", B, ["pad", "pool"], 18, **kw),
            mk(tag + "same_T", T, ["plain0"], 19, **kw), mk(tag + "pool_T", T, ["pool"], 20, **kw),
            mk(tag + "same_P", P, ["plain"], 23, **kw), mk(tag + "same_B", B, ["plain"], 24, **kw),
        ]
        if tag != "ties_":       # (no pool in this sequence: a ties case would add nothing to the plain one)
            cases += [mk(tag + "head_A", A, ["head"], 21, **kw), mk(tag + "head_H", (1, 16, 33, 7), ["head"], 22, **kw)]
        cases += [mk(tag + "same_O", O, ["plain"], 25, **kw), mk(tag + "pool+skip_O", O, ["plain", "pool"], 26, **kw)]
    for k in cases:
        k.stores_g = k.name.split("_")[-2].startswith(("pad", "up"))
    return cases


def blend_pair(dt, c, hw, alpha, seed=31, **kw):
    """The two alpha-blend branches (0: pixel-shuffled, weight 1 - sigmoid(alpha); 1: plain, weight sigmoid(alpha)) with ONE
    shared upstream gradient, correlated with both branches' xhat (both gammas carry the same signs, so that neither branch's
    S1 cancels); scaled by 4 so that |S1|, |S2| >= 0.1 also under the weight 1 - sigmoid(1.5) = 0.18 - by 12 in the kink
    variant, whose x on {-1 .. 1} under the handed rstd = 1 has an xhat of standard deviation 0.65, not 1: the part of the
    gradient that follows xhat is that much weaker."""
    gen = torch.Generator().manual_seed(seed)
    sign = np.where(_rand(gen, c) < 0.5, -1.0, 1.0)
    sign[0], sign[1] = 1.0, -1.0
    shape = (2, c) + tuple(hw)
    br = [make_case(f"blend_ps_C{c}_{hw[0]}x{hw[1]}_a{alpha}", dt, shape, ["plain0"], seed + 1, alpha=alpha, wm=2, gamma_sign=sign, a0=0.75, b0=2.0, **kw),
          make_case(f"blend_bil_C{c}_{hw[0]}x{hw[1]}_a{alpha}", dt, shape, ["plain0"], seed + 2, alpha=alpha, wm=1, gamma_sign=sign, a0=0.75, b0=2.0, **kw)]
    g0, g1 = br[0].cons[0].da, br[1].cons[0].da
    shared = rounded((12.0 if kw.get("kink") else 4.0) * (g0 + g1), dt)
    for b in br:
        b.cons[0].da = shared
        if kw.get("kink"):
            b.name = "kink_" + b.name
    br[0].shuffled = True
    return br


BLEND_SHAPES = [(16, (12, 20)), (32, (12, 20)), (16, (32, 48)), (32, (32, 48))]


def blend_cases(dt):
    """{(c, hw, alpha, kink): the pair} of the blend tests (16-bit storage only)."""
    if dt == F32:
        return {}
    return {(c, hw, alpha, kink): blend_pair(dt, c, hw, alpha, kink=kink)
            for c, hw in BLEND_SHAPES for alpha in (0.0, 1.5) for kink in (False, True)}


UNSHUFFLE = [((2, 32, 18, 26), 0), ((1, 16, 6, 40), 2)]


def unshuffle_cases(dt):
    """{(shape, weight_mode, tag): case} of mrisr_act_bwd_apply_fused_unshuffle: one plain consumer of the node's geometry,
    unweighted or weighted 1 - sigmoid(0.3) (then with twice the gradient, so that |S1|, |S2| >= 0.1 under that weight)."""
    out = {}
    for shape, wm in UNSHUFFLE:
        for tag in ("", "kink_"):
            kw = dict(alpha=0.3, wm=2, a0=3.0, b0=4.5) if wm else {}
            k = make_case(f"{tag}unshuffle_wm{wm}", dt, shape, ["plain0"], 41 + wm, kink=bool(tag), **kw)
            k.shuffled = True
            out[(shape, wm, tag)] = k
    return out


FORWARD_SHAPES = [(1, 16, 8, 8), (2, 32, 11, 19)]


def forward_cases(dt):
    """{shape: the ties case} of the forward pool / upsample kernels (a pooled node, so that the backward bounds and mutants
    can be run on it as well)."""
    bygroup = lambda c: np.repeat(np.array([1.0, -1.0] * (G // 2)), c // G)          # noqa: E731
    return {shape: make_case(f"ties_forward_{shape[2]}x{shape[3]}", dt, shape, ["pool"], 51, ties=True, gamma_sign=bygroup(shape[1]))
            for shape in FORWARD_SHAPES}


def all_cases(dt):
    cs = case_list(dt) + list(unshuffle_cases(dt).values()) + list(forward_cases(dt).values())
    for pair in blend_cases(dt).values():
        cs += pair
    return cs
