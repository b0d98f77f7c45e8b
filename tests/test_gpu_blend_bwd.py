"""csrc/norm_bwd_shuffle.hip: the GroupNorm + LeakyReLU backward of the two alpha-blend branches in ONE pair of launches
(mrisr_act_bwd_blend_reduce / mrisr_act_bwd_blend_apply: the shared gradient of the blended tensor is read once per pass),
against a float64 CPU restatement and against the four launches it replaces (mrisr_act_bwd_reduce twice,
mrisr_act_bwd_apply_fused_unshuffle, mrisr_act_bwd_apply_fused).  Weights as the engine registers them
(unet_model.py:206-207): the bilinear (plain) branch takes sigmoid(alpha), weight_mode 1, the pixel-shuffled one the rest."""
from __future__ import annotations

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import hiputil as U
from mri_superresolution_amd import _lib as L

pytestmark = pytest.mark.gpu

G = 8               # the network's GroupNorm group count
WM_PS, WM_BIL = 2, 1
E_UNSUPPORTED = -5     # MRISR_E_UNSUPPORTED (include/mrisr.h)


def rnd(*shape, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=gen) * scale


def gn_state(x, gamma, beta, dt):
    """stats -> mrisr_gn_finalize on the device for x (N,C,H,W): (scale, shift, meanrstd) as the forward pass leaves them."""
    n, c, h, w = x.shape
    xr = U.rounded(x, dt).double().view(n, G, -1)
    stats = torch.zeros(L.STAT_SLOTS, n, G, 2, dtype=torch.float64)
    stats[3] = torch.stack([xr.sum(2), (xr * xr).sum(2)], -1)
    stats = stats.contiguous().to(U.DEV)
    scale, shift, mr = torch.empty(n * c, device=U.DEV), torch.empty(n * c, device=U.DEV), torch.empty(n * G * 2, device=U.DEV)
    gd, bd = gamma.to(U.DEV), beta.to(U.DEV)
    L.call("mrisr_gn_finalize", stats.data_ptr(), gd.data_ptr(), bd.data_ptr(), scale.data_ptr(), shift.data_ptr(),
           mr.data_ptr(), n, c, G, float((c // G) * h * w), 1e-5, U.stream())
    torch.cuda.synchronize()
    return scale, shift, mr


class Case:
    """Inputs of one case on the CPU (rounded to the storage dtype) and on the device."""

    def __init__(self, dt, n, c, h, w, alpha):
        self.dt, self.n, self.c, self.h, self.w = dt, n, c, h, w
        self.alpha = torch.tensor([alpha])
        self.g = U.rounded(rnd(n, c, h, w, seed=5), dt)
        self.x = [U.rounded(rnd(n, c, h, w, seed=6 + b, scale=1.5), dt) for b in range(2)]       # 0: pixel-shuffled, 1: plain
        self.gamma = [1 + 0.2 * rnd(c, seed=8 + b) for b in range(2)]
        self.beta = [0.1 * rnd(c, seed=10 + b) for b in range(2)]
        self.gd = U.nhwc(self.g, dt)
        self.xd = [U.nhwc(x, dt) for x in self.x]
        self.state = [gn_state(self.x[b], self.gamma[b], self.beta[b], dt) for b in range(2)]
        self.gammad = [t.to(U.DEV) for t in self.gamma]
        self.ad = self.alpha.to(U.DEV)
        self.count = float((c // G) * h * w)

    def outputs(self):
        n, c, h, w = self.n, self.c, self.h, self.w
        z = lambda *s: torch.zeros(*s, device=U.DEV)        # noqa: E731
        return dict(dx_ps=torch.full((n, h // 2, w // 2, 4 * c), float("nan"), dtype=U.tdt(self.dt), device=U.DEV),
                    dx_bil=torch.full((n, h, w, c), float("nan"), dtype=U.tdt(self.dt), device=U.DEV),
                    dgamma=[z(c), z(c)], dbeta=[z(c), z(c)], dalpha=z(1), dbias=z(4 * c),
                    red=[z(n * c * 2 + 256), z(n * c * 2 + 256)])

    def fin(self, o, b):
        nc2 = self.n * self.c * 2
        return L.GnBwdFin(o["red"][b].data_ptr(), self.gammad[b].data_ptr(), self.state[b][2].data_ptr(), o["dgamma"][b].data_ptr(),
                          o["dbeta"][b].data_ptr(), o["red"][b][nc2:].data_ptr(), self.ad.data_ptr(), o["dalpha"].data_ptr(),
                          self.count, 1.0 if (WM_PS, WM_BIL)[b] == 1 else -1.0, G)

    def branch(self, o, b):
        sc, sh, mr = self.state[b]
        return L.BlendBranch(self.xd[b].data_ptr(), sc.data_ptr(), sh.data_ptr(), mr.data_ptr(), o["red"][b].data_ptr(),
                             o["red"][b][self.n * self.c * 2:].data_ptr(), (WM_PS, WM_BIL)[b], 0)


def run_new(k: Case, reduce=True):
    o = k.outputs()
    bp, bb = k.branch(o, 0), k.branch(o, 1)
    n, c, h, w = k.n, k.c, k.h, k.w
    if reduce:
        L.call("mrisr_act_bwd_blend_reduce", k.dt, k.gd.data_ptr(), C.byref(bp), C.byref(bb), k.ad.data_ptr(), n, h, w, c, G, U.stream())
    fp, fb = k.fin(o, 0), k.fin(o, 1)
    L.call("mrisr_act_bwd_blend_apply", k.dt, k.gd.data_ptr(), C.byref(bp), C.byref(bb), k.ad.data_ptr(), C.byref(fp), C.byref(fb),
           o["dx_ps"].data_ptr(), o["dx_bil"].data_ptr(), o["dbias"].data_ptr(), n, h, w, c, U.stream())
    torch.cuda.synchronize()
    return o


def run_old(k: Case):
    """The four launches the engine issued for the two nodes."""
    o = k.outputs()
    n, c, h, w = k.n, k.c, k.h, k.w
    nc2 = n * c * 2
    carrs = []
    for b in range(2):
        sc, sh, mr = k.state[b]
        carr = (L.Consumer * 2)()
        carr[0].da, carr[0].C_total, carr[0].c_off, carr[0].H, carr[0].W = k.gd.data_ptr(), c, 0, h, w
        carr[0].spatial, carr[0].weight_mode = L.SP_NONE, (WM_PS, WM_BIL)[b]
        carrs.append(carr)
        L.call("mrisr_act_bwd_reduce", k.dt, k.xd[b].data_ptr(), sc.data_ptr(), sh.data_ptr(), mr.data_ptr(), 1, carr, k.ad.data_ptr(),
               None, o["red"][b].data_ptr(), o["red"][b][nc2:].data_ptr(), n, h, w, c, G, U.stream())
    fp, fb = k.fin(o, 0), k.fin(o, 1)
    sc, sh, _ = k.state[0]
    L.call("mrisr_act_bwd_apply_fused_unshuffle", k.dt, k.xd[0].data_ptr(), sc.data_ptr(), sh.data_ptr(), carrs[0], k.ad.data_ptr(),
           C.byref(fp), o["dx_ps"].data_ptr(), o["dbias"].data_ptr(), n, h, w, c, U.stream())
    sc, sh, _ = k.state[1]
    L.call("mrisr_act_bwd_apply_fused", k.dt, k.xd[1].data_ptr(), sc.data_ptr(), sh.data_ptr(), 1, carrs[1], k.ad.data_ptr(), None,
           C.byref(fb), o["dx_bil"].data_ptr(), n, h, w, c, U.stream())
    torch.cuda.synchronize()
    return o


def ref_f64(k: Case):
    """GroupNorm(8, C) + LeakyReLU(0.2) backward of both branches under L = sum g * (a act_bil + (1 - a) act_ps), a = sigmoid(alpha),
    in float64; next to every reduced quantity the fp32 summation bound n_terms * 2^-24 * sum |terms| of its sum."""
    n, c, h, w = k.n, k.c, k.h, k.w
    a = torch.sigmoid(k.alpha.double())
    g = k.g.double()
    eps32 = 2.0 ** -24
    r = dict(dgamma=[], dbeta=[], dgamma_b=[], dbeta_b=[])
    acts = []
    for b in range(2):
        wgt = a if (WM_PS, WM_BIL)[b] == 1 else 1 - a
        x = k.x[b].double().view(n, G, c // G, h, w)
        mean = x.mean((2, 3, 4), keepdim=True)
        rstd = 1.0 / torch.sqrt(x.var((2, 3, 4), unbiased=False, keepdim=True) + 1e-5)
        xhat = ((x - mean) * rstd).view(n, c, h, w)
        gam, bet = k.gamma[b].double().view(1, c, 1, 1), k.beta[b].double().view(1, c, 1, 1)
        pre = xhat * gam + bet
        acts.append(F.leaky_relu(pre, 0.2))
        dy = wgt * g * torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, 0.2))
        tg, tb = dy * xhat, dy
        nt = n * h * w
        r["dgamma"].append(tg.sum((0, 2, 3)))
        r["dbeta"].append(tb.sum((0, 2, 3)))
        r["dgamma_b"].append(nt * eps32 * tg.abs().sum((0, 2, 3)))
        r["dbeta_b"].append(nt * eps32 * tb.abs().sum((0, 2, 3)))
        dyg = (dy * gam).view(n, G, c // G, h, w)
        xh = xhat.view(n, G, c // G, h, w)
        dx = rstd * (dyg - dyg.mean((2, 3, 4), keepdim=True) - xh * (dyg * xh).mean((2, 3, 4), keepdim=True))
        r["dx_ps" if b == 0 else "dx_bil"] = dx.view(n, c, h, w)
    sgn = 1.0 if WM_BIL == 1 else -1.0
    ta = a * (1 - a) * g * (acts[1] - acts[0]) * sgn
    r["dalpha"] = ta.sum().view(1)
    r["dalpha_b"] = (2 * ta.numel()) * eps32 * (a * (1 - a) * g.abs() * (acts[1].abs() + acts[0].abs())).sum().view(1)
    un = F.pixel_unshuffle(r["dx_ps"], 2)
    r["dbias"] = un.sum((0, 2, 3))
    r["dbias_b"] = (n * (h // 2) * (w // 2)) * eps32 * un.abs().sum((0, 2, 3))
    return r


def errs(got, ref):
    e = got - ref
    return float(e.abs().max()), float(e.pow(2).mean().sqrt())


# every pixel on an edge / a partly empty block / a few hundred windows per image / several blocks per image and pass at both
# widths (a block of pass 1 covers 512 windows at C = 32 and 1024 at C = 16, a block of pass 2 twice that)
SHAPES = [(4, 4), (12, 20), (32, 48), (96, 64)]


@pytest.mark.parametrize("alpha", [0.0, 1.5])
@pytest.mark.parametrize("dt", [L.BF16, L.F16])
@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("c", [32, 16])
def test_blend_pair_vs_f64_and_four_launches(c, hw, dt, alpha):
    k = Case(dt, 2, c, hw[0], hw[1], alpha)
    ref = ref_f64(k)
    new, old = run_new(k), run_old(k)
    tag = f"C={c} {hw[0]}x{hw[1]} {'bf16' if dt == L.BF16 else 'fp16'} alpha={alpha}"
    eps = float(torch.finfo(U.tdt(dt)).eps)
    for name in ("dx_ps", "dx_bil"):
        gn, go = ((F.pixel_shuffle(U.nchw(o[name]), 2) if name == "dx_ps" else U.nchw(o[name])).double() for o in (new, old))
        assert torch.isfinite(gn).all() and torch.isfinite(go).all()
        (mn, rn), (mo, ro) = errs(gn, ref[name]), errs(go, ref[name])
        half_ulp = 0.5 * eps * 2.0 ** torch.frexp(ref[name].abs().max()).exponent.item() / 2.0
        print(f"{tag} {name}: max err new {mn:.3e} old {mo:.3e} (+{half_ulp:.1e}), rms new {rn:.3e} old {ro:.3e}")
        assert mn <= 1.25 * mo + half_ulp, (name, mn, mo, half_ulp)
        assert rn <= 1.25 * ro, (name, rn, ro)
    red = [("dalpha", new["dalpha"], old["dalpha"], ref["dalpha"], ref["dalpha_b"]),
           ("dbias", new["dbias"], old["dbias"], ref["dbias"], ref["dbias_b"])]
    for b, br in enumerate(("ps", "bil")):
        red.append((f"dgamma_{br}", new["dgamma"][b], old["dgamma"][b], ref["dgamma"][b], ref["dgamma_b"][b]))
        red.append((f"dbeta_{br}", new["dbeta"][b], old["dbeta"][b], ref["dbeta"][b], ref["dbeta_b"][b]))
    for name, vn, vo, vr, bound in red:
        en, eo = (vn.double().cpu() - vr).abs(), (vo.double().cpu() - vr).abs()
        print(f"{tag} {name}: worst err new {float(en.max()):.3e} old {float(eo.max()):.3e}, fp32 summation bound {float(bound.max()):.3e}, "
              f"|ref| max {float(vr.abs().max()):.3e}")
        assert torch.isfinite(vn).all()
        assert bool((en <= 1.5 * eo + bound).all()), (name, en, eo, bound)


@pytest.mark.parametrize("dt", [L.BF16, L.F16])
@pytest.mark.parametrize("c,hw", [(16, (12, 20)), (32, (32, 48))])
def test_blend_apply_unshuffled_layout_is_exact(dt, c, hw):
    """Indexing alone: zero group sums, unit statistics and x = 1 make pass 2 the identity on w * g, with w = 1/2 at alpha = 0;
    g = twice a coordinate (n, c, y or x: small integers, exact in both dtypes), so dx must BE that coordinate: plain for the
    bilinear branch, pixel_unshuffle of it for the pixel-shuffled one."""
    n, (h, w) = 2, hw
    k = Case(dt, n, c, h, w, 0.0)
    ones = torch.ones(n, c, h, w)
    k.xd = [U.nhwc(ones, dt), U.nhwc(ones, dt)]
    mr = torch.zeros(n * G * 2, device=U.DEV)
    mr[1::2] = 1.0
    k.state = [(torch.ones(n * c, device=U.DEV), torch.zeros(n * c, device=U.DEV), mr) for _ in range(2)]
    k.gammad = [torch.ones(c, device=U.DEV) for _ in range(2)]
    coords = torch.meshgrid(torch.arange(n), torch.arange(c), torch.arange(h), torch.arange(w), indexing="ij")
    for coord in coords:
        pat = coord.float()
        k.gd = U.nhwc(2 * pat, dt)
        o = run_new(k, reduce=False)          # red stays zero: cB = cC = 0, cA = 1
        assert torch.equal(U.nchw(o["dx_bil"]), pat)
        assert torch.equal(U.nchw(o["dx_ps"]), F.pixel_unshuffle(pat, 2))
        assert torch.equal(o["dbias"].cpu(), F.pixel_unshuffle(pat, 2).sum((0, 2, 3)))      # integers below 2^24: exact in any order


def test_blend_predicate_and_refusals():
    lib = L.load()
    assert lib.mrisr_act_bwd_blend_ok(L.BF16, 2, 12, 20, 32) == 1 and lib.mrisr_act_bwd_blend_ok(L.F16, 16, 512, 512, 32) == 1
    assert lib.mrisr_act_bwd_blend_ok(L.F32, 2, 12, 20, 32) == 0
    assert lib.mrisr_act_bwd_blend_ok(L.BF16, 2, 11, 20, 32) == 0 and lib.mrisr_act_bwd_blend_ok(L.BF16, 2, 12, 19, 32) == 0
    assert lib.mrisr_act_bwd_blend_ok(L.BF16, 2, 12, 20, 12) == 0 and lib.mrisr_act_bwd_blend_ok(L.BF16, 2, 12, 20, 4096) == 0
    k = Case(L.BF16, 2, 16, 12, 20, 0.3)
    o = k.outputs()
    bp, bb, fp, fb = k.branch(o, 0), k.branch(o, 1), k.fin(o, 0), k.fin(o, 1)
    for dt, h, w in ((L.BF16, 11, 20), (L.BF16, 12, 19), (L.F32, 12, 20)):
        assert lib.mrisr_act_bwd_blend_reduce(dt, k.gd.data_ptr(), C.byref(bp), C.byref(bb), k.ad.data_ptr(), 2, h, w, 16, G,
                                              U.stream()) == E_UNSUPPORTED
        assert lib.mrisr_act_bwd_blend_apply(dt, k.gd.data_ptr(), C.byref(bp), C.byref(bb), k.ad.data_ptr(), C.byref(fp), C.byref(fb),
                                             o["dx_ps"].data_ptr(), o["dx_bil"].data_ptr(), None, 2, h, w, 16, U.stream()) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert float(o["red"][0].abs().sum()) == 0.0 and bool(torch.isnan(o["dx_bil"].float()).all())      # nothing was launched


def _full_model_grads(monkeypatch, merged: bool):
    from mri_superresolution_amd.models.unet_model import UNetSuperRes
    from mri_superresolution_amd.utils.losses import CombinedLoss
    from oracle.inputs import make_pair
    from oracle.unet_ref import formula_state_dict
    f, seed = 16, 1
    calls = []
    real_call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a, **kw: (calls.append(name), real_call(name, *a, **kw))[1])
    if not merged:
        monkeypatch.setattr(L.load(), "mrisr_act_bwd_blend_ok", lambda *a: 0)
    m = UNetSuperRes(1, 1, f)
    m.load_state_dict(formula_state_dict(f, seed))
    m = m.cuda().set_compute_dtype(torch.bfloat16).train()
    low, high = make_pair(2, 32, 32, seed)
    loss = CombinedLoss(ssim_weight=0.4, device=torch.device("cuda"))(m(low.cuda()), high.cuda())
    loss.backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    return {k: p.grad.detach().float().cpu() for k, p in m.named_parameters()}, calls, float(loss)


def test_engine_takes_the_merged_path_and_gradients_agree(monkeypatch):
    """Full model (f = 16, N = 2, 32 x 32, bf16): one forward + backward with the merged launches, and two with the predicate
    answering 0 (the four per-node launches; their own run-to-run spread is printed next to every figure).  The runs differ as two
    runs of either path differ: the order of float atomics in the per-(n,c) sums, after which single 16-bit roundings of dx flip by
    one ulp and travel down the gradient chain.
    - Every parameter: max |merged - separate| within the model tests' run-to-run tolerance for float atomics
      (test_gpu_model.test_grad_accumulation_and_eval_mode: 1e-4 of the largest gradient) or, where that is larger, 4 bf16 ulps
      (4 * 2^-8) of the parameter's own largest element: what a handful of flipped roundings in the 16-bit chain is worth; and
      cosine >= 0.9999 between the two runs.
    - What the merged kernels produce themselves in fp32 (dalpha, the two nodes' dgamma / dbeta, the pixel-shuffle conv's bias
      gradient): the 1e-4 tolerance alone, signs equal."""
    from oracle.bf16_emul import cos_ratio
    gm, cm, lm = _full_model_grads(monkeypatch, True)
    gs, cs, ls = _full_model_grads(monkeypatch, False)
    g2, _, _ = _full_model_grads(monkeypatch, False)
    assert cm.count("mrisr_act_bwd_blend_reduce") == 1 and cm.count("mrisr_act_bwd_blend_apply") == 1
    assert "mrisr_act_bwd_apply_fused_unshuffle" not in cm
    assert "mrisr_act_bwd_blend_reduce" not in cs and cs.count("mrisr_act_bwd_apply_fused_unshuffle") == 1
    assert cs.count("mrisr_act_bwd_reduce") == cm.count("mrisr_act_bwd_reduce") + 2
    assert abs(lm - ls) <= 1e-6           # the forward is the same code
    assert set(gm) == set(gs)
    tol = 1e-4 * max(float(v.abs().max()) for v in gs.values())
    direct = ("alpha", "final_up_bilinear.2.weight", "final_up_bilinear.2.bias", "final_up_pixelshuffle.norm.weight",
              "final_up_pixelshuffle.norm.bias", "final_up_pixelshuffle.conv.bias")
    bad = []
    for k in gs:
        d, d_old = float((gm[k] - gs[k]).abs().max()), float((g2[k] - gs[k]).abs().max())
        cos, _ = cos_ratio(gm[k], gs[k])
        tk = tol if k in direct else max(tol, 4 * 2.0 ** -8 * float(gs[k].abs().max()))
        print(f"{k}: max |merged - separate| {d:.3e} (separate run to run {d_old:.3e}; bound {tk:.3e}, max |grad| "
              f"{float(gs[k].abs().max()):.3e}), cosine {cos:.7f}")
        if not (d <= tk and cos >= 0.9999):
            bad.append((k, d, tk, cos))
        if k in direct:
            big = gs[k].abs() > tol           # (a sign is only defined beyond the noise the tolerance stands for)
            assert torch.equal(torch.sign(gm[k][big]), torch.sign(gs[k][big])), k
    assert not bad, bad
