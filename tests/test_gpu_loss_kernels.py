"""csrc/loss.hip through its C entry points against the float64 specification of tests/lossutil.py (pinned on the CPU by
test_loss_ref_host.py): mrisr_ssim_l1_forward_win + mrisr_loss_finalize, mrisr_ssim_l1_backward_win, mrisr_image_metrics +
mrisr_metrics_finalize.  A rewrite of the kernels that keeps the C ABI must keep this file passing unchanged.

What is run: every window the switch instantiates (3 .. 15) at shapes smaller than the halo, on and beside the tile edges
(forward tile 32 x 32, backward tile 32 x 8) and over several blocks (lossutil.SHAPES); the clamp gate closed (anti_pair) and
open over planes of opposite SSIM sign (mixed_batch); the device-side upstream gradient; val_range 255; L1 ties; every
null-pointer form; the refusals.  Every output buffer lies between guard bands (hiputil.Guarded).

Bars: per-plane SSIM 5e-6, per-plane L1 sum 1e-6 relative, total / L1 mean / SSIM mean 1e-5, coefficient planes 1e-4 of each
plane's maximum, metrics as test_gpu_eval.py (mse, mae 1e-6 relative, rmse == sqrt(mse), psnr 1e-5, ssim 5e-6).
Gradient: BWD_BAR of the float64 gradient's maximum.  The project's bar is 2e-4; the worst case measured on the MI355X over
every case of this file is 1.03e-5 (mixed_batch, window 13, the nearly identical plane against its own maximum; 2.2e-6 is the
worst of the (0.6, 0.4) cases), more than 10 x below the bar everywhere, so the bar held here is 10 x that: 1.03e-4.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mri_superresolution_amd import _lib as L          # noqa: E402
import hiputil as U                                    # noqa: E402
import lossutil as LU                                  # noqa: E402

PROJECT_BWD_BAR = 2e-4
MEASURED_WORST = 1.03e-5
BWD_BAR = 10 * MEASURED_WORST
assert BWD_BAR < PROJECT_BWD_BAR
E_ARG, E_UNSUPPORTED = -1, -5
SIGMA = 1.5


def _sid(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _report(line):
    """The measured figure behind an assertion, in the test's captured output (pytest -rA or -s shows it)."""
    print(line)


# ------------------------------------------------------------------------------------------------ references, computed once
@functools.lru_cache(maxsize=None)
def _pair(kind, shape, val_range=1.0):
    a, b = {"noisy": LU.noisy_pair, "anti": LU.anti_pair, "mixed": LU.mixed_batch}[kind](shape)
    return a * val_range, b * val_range


@functools.lru_cache(maxsize=None)
def _ref(kind, shape, win, l1_w, ssim_w, val_range=1.0, clamp=True):
    a, b = _pair(kind, shape, val_range)
    return LU.loss_and_grad64(a, b, l1_w, ssim_w, win, SIGMA, val_range, clamp=clamp)


# ------------------------------------------------------------------------------------------------ launches
class Run:
    """One pair on the device and the entry points on it."""

    def __init__(self, a, b, win, val_range=1.0):
        self.n, self.h, self.w = a.shape
        self.a, self.b = a.contiguous().to(U.DEV), b.contiguous().to(U.DEV)
        self.win, self.val_range = win, val_range
        self.dims = (self.n, self.h, self.w)

    def forward(self, coef=True, sums=None):
        """Returns (sums Guarded [N][2] float64, coef Guarded [3][N][H][W] or None); ``sums``: accumulate into these."""
        if sums is None:
            sums = U.Guarded(torch.zeros(self.n, 2, dtype=torch.float64))
        cf = U.Guarded(torch.full((3,) + self.dims, float("nan"), dtype=torch.float32)) if coef else None
        L.call("mrisr_ssim_l1_forward_win", self.a.data_ptr(), self.b.data_ptr(), sums.data_ptr(), L.ptr(cf), *self.dims,
               self.val_range, SIGMA, self.win, U.stream())
        torch.cuda.synchronize()
        sums.check("forward: sums")
        if cf is not None:
            cf.check("forward: coef")
        return sums, cf

    def finalize(self, sums, l1_w, ssim_w):
        out = U.Guarded(torch.full((3 + self.n,), float("nan"), dtype=torch.float32))
        L.call("mrisr_loss_finalize", sums.data_ptr(), *self.dims, l1_w, ssim_w, out.data_ptr(), U.stream())
        torch.cuda.synchronize()
        out.check("loss_finalize: out")
        return out.t.cpu().double().numpy()

    def backward(self, cf, sums, l1_w, ssim_w, gscale=None):
        da = U.Guarded(torch.full(self.dims, float("nan"), dtype=torch.float32))
        gs = None if gscale is None else torch.tensor([gscale], dtype=torch.float32, device=U.DEV)
        L.call("mrisr_ssim_l1_backward_win", self.a.data_ptr(), self.b.data_ptr(), L.ptr(cf), L.ptr(sums), L.ptr(gs), l1_w, ssim_w,
               da.data_ptr(), *self.dims, SIGMA, self.win, U.stream())
        torch.cuda.synchronize()
        da.check("backward: da")
        got = da.t.cpu()
        assert torch.isfinite(got).all(), "backward: elements left unwritten or not finite"
        return got


def _grad_ratio(got, ref_grad, what):
    """Asserts the gradient within BWD_BAR of the reference's maximum; returns error / maximum."""
    scale = np.abs(ref_grad).max()
    assert scale > 0, what
    err = np.abs(got.double().numpy() - ref_grad).max() / scale
    _report(f"loss.hip backward {what}: err / max {err:.2e} (bar {BWD_BAR:.1e})")
    assert err <= BWD_BAR, f"{what}: {err:.3e}"
    return err


def _check_sums(sums, ref, dims, what):
    n, h, w = dims
    s = sums.t.cpu().numpy()
    e_ssim = np.abs(s[:, 1] / (h * w) - ref.ssim_planes).max()
    e_l1 = (np.abs(s[:, 0] - ref.l1_sums) / ref.l1_sums).max()
    _report(f"loss.hip forward {what}: per-plane ssim err {e_ssim:.2e} (bar 5e-6), L1 sum rel err {e_l1:.2e} (bar 1e-6)")
    assert e_ssim <= 5e-6 and e_l1 <= 1e-6, what


def _check_finalize(out, ref, what, l1_w, ssim_w):
    errs = abs(out[0] - ref.total), abs(out[1] - ref.l1_mean), abs(out[2] - ref.ssim_mean), np.abs(out[3:] - ref.ssim_planes).max()
    _report(f"loss.hip finalize {what} ({l1_w}, {ssim_w}): total {errs[0]:.2e}, L1 mean {errs[1]:.2e}, ssim mean {errs[2]:.2e} "
            f"(bars 1e-5), per-plane {errs[3]:.2e} (bar 5e-6)")
    assert max(errs[:3]) <= 1e-5 and errs[3] <= 5e-6, what


# ------------------------------------------------------------------------------------------------ forward + backward, every window
@pytest.mark.parametrize("win", LU.WINDOWS)
@pytest.mark.parametrize("shape", LU.SHAPES, ids=_sid)
def test_forward_finalize_and_backward_against_float64(shape, win):
    what = f"{_sid(shape)} w{win}"
    ref = _ref("noisy", shape, win, 0.6, 0.4)
    assert (ref.l1_sums > 0).all() and 0.0 < ref.ssim_mean < 1.0 - 1e-3
    run = Run(*_pair("noisy", shape), win)
    sums, cf = run.forward()
    _check_sums(sums, ref, shape, what)
    _check_finalize(run.finalize(sums, 0.6, 0.4), ref, what, 0.6, 0.4)
    # without the coefficient planes: the same sums
    sums0, _ = run.forward(coef=False)
    _check_sums(sums0, ref, shape, what + " coef=NULL")
    assert np.allclose(sums0.t.cpu().numpy(), sums.t.cpu().numpy(), rtol=1e-12, atol=0)
    # the sums are accumulators: a second pass on the same buffer doubles them exactly
    once = sums0.t.cpu().clone()
    run.forward(coef=False, sums=sums0)
    assert torch.equal(sums0.t.cpu(), 2 * once), what
    assert torch.isfinite(cf.t).all()
    _grad_ratio(run.backward(cf, sums, 0.6, 0.4), ref.grad, what + " (0.6, 0.4)")


@pytest.mark.parametrize("shape,win", LU.cover(), ids=_sid)
def test_backward_weight_forms_and_device_scale(shape, win):
    what = f"{_sid(shape)} w{win}"
    run = Run(*_pair("noisy", shape), win)
    sums, cf = run.forward()
    numel = float(np.prod(shape))
    # SSIM only; L1 only without coefficient planes; the ssim() form: no sums (no gate), weights (0, -1)
    _grad_ratio(run.backward(cf, sums, 0.0, 1.0), _ref("noisy", shape, win, 0.0, 1.0).grad, what + " (0, 1)")
    l1 = run.backward(None, sums, 1.0, 0.0)
    _grad_ratio(l1, _ref("noisy", shape, win, 1.0, 0.0).grad, what + " (1, 0) coef=NULL")
    sign = torch.sign(run.a.cpu() - run.b.cpu()).double()
    assert np.allclose(l1.double().numpy(), (sign / numel).numpy(), rtol=1e-6, atol=0)
    assert torch.equal(run.backward(None, None, 1.0, 0.0), l1)
    _grad_ratio(run.backward(cf, None, 0.0, -1.0), _ref("noisy", shape, win, 0.0, -1.0, clamp=False).grad, what + " (0, -1) sums=NULL")
    # the device-side upstream gradient: a power of two scales the result exactly
    base = run.backward(cf, sums, 0.6, 0.4)
    ref = _ref("noisy", shape, win, 0.6, 0.4)
    for gscale in (1024.0, 2.0 ** -10):
        got = run.backward(cf, sums, 0.6, 0.4, gscale=gscale)
        assert torch.equal(got, base * gscale), f"{what}: gscale {gscale}"
        _grad_ratio(got, ref.grad * gscale, what + f" gscale {gscale:g}")
    assert torch.equal(run.backward(cf, sums, 0.6, 0.4, gscale=1.0), base)


@pytest.mark.parametrize("win", [5, 11])
@pytest.mark.parametrize("shape", [(2, 3, 5), (1, 31, 33), (3, 7, 65)], ids=_sid)
def test_val_range_255_loss_and_gradient(shape, win):
    what = f"{_sid(shape)} w{win} val_range 255"
    ref = _ref("noisy", shape, win, 0.0, 1.0, 255.0)
    # a kernel that dropped val_range (C1, C2 of range 1 on these images) would be visibly off
    assert abs(ref.ssim_mean - LU.loss_and_grad64(*_pair("noisy", shape, 255.0), 0.0, 1.0, win, SIGMA, 1.0).ssim_mean) > 10 * 5e-6
    run = Run(*_pair("noisy", shape, 255.0), win, val_range=255.0)
    sums, cf = run.forward()
    _check_sums(sums, ref, shape, what)
    _check_finalize(run.finalize(sums, 0.0, 1.0), ref, what, 0.0, 1.0)
    _grad_ratio(run.backward(cf, sums, 0.0, 1.0), ref.grad, what + " (0, 1)")


@pytest.mark.parametrize("win", LU.WINDOWS)
@pytest.mark.parametrize("shape", [(2, 3, 5), (1, 31, 33)], ids=_sid)
def test_coefficient_planes_directly(shape, win):
    """The three planes the forward leaves for the backward, against the header formulas in float64: the one check that
    places an error in the forward kernel when both kernels change together."""
    a, b = _pair("noisy", shape)
    want = LU.coef64(a, b, win, SIGMA).numpy()
    _, cf = Run(a, b, win).forward()
    got = cf.t.cpu().double().numpy()
    for q, name in enumerate(("dS/dmu1", "dS/dE[x^2]", "dS/dE[xy]")):
        err = np.abs(got[q] - want[q]).max() / np.abs(want[q]).max()
        _report(f"loss.hip coef {_sid(shape)} w{win} {name}: err / max {err:.2e} (bar 1e-4)")
        assert err <= 1e-4, name


# ------------------------------------------------------------------------------------------------ the clamp gate
@pytest.mark.parametrize("shape", LU.ANTI_SHAPES, ids=_sid)
def test_closed_gate_leaves_only_the_l1_gradient(shape):
    a, b = _pair("anti", shape)
    ne = (a != b)
    for win in LU.WINDOWS:
        ref = _ref("anti", shape, win, 0.6, 0.4)
        assert ref.ssim_mean < -0.3                        # (asserted for every window in test_loss_ref_host.py as well)
        run = Run(a, b, win)
        sums, cf = run.forward()
        _check_sums(sums, ref, shape, f"anti {_sid(shape)} w{win}")
        out = run.finalize(sums, 0.6, 0.4)
        _check_finalize(out, ref, f"anti {_sid(shape)} w{win}", 0.6, 0.4)
        assert out[2] < -0.3 and abs(out[0] - (0.6 * ref.l1_mean + 0.4)) <= 1e-5          # the total clamps, the mean does not
        got = run.backward(cf, sums, 0.6, 0.4)
        assert torch.equal(got, run.backward(cf, sums, 0.6, 0.0)), f"w{win}: the SSIM term leaks through the closed gate"
        assert torch.equal(got, run.backward(None, sums, 0.6, 0.0))
        mag = got.double()[ne].abs().numpy()
        assert np.allclose(mag, 0.6 / a.numel(), rtol=1e-6, atol=0)
        assert torch.equal(torch.sign(got)[ne], torch.sign(a - b)[ne])
        _grad_ratio(got, ref.grad, f"anti {_sid(shape)} w{win} (0.6, 0.4)")
        # without sums there is no gate: the bare ssim() gradient of the same pair is NOT zero
        _grad_ratio(run.backward(cf, None, 0.0, -1.0), _ref("anti", shape, win, 0.0, -1.0, clamp=False).grad,
                    f"anti {_sid(shape)} w{win} (0, -1) sums=NULL")


@pytest.mark.parametrize("win", LU.WINDOWS)
def test_gate_is_on_the_batch_mean_and_planes_stay_apart(win):
    shape = LU.MIXED_SHAPE
    ref = _ref("mixed", shape, win, 0.0, 1.0)
    assert ref.ssim_planes[0] < -0.5 and ref.ssim_planes[1] > 0.99 and 0.05 < ref.ssim_mean < 0.5
    run = Run(*_pair("mixed", shape), win)
    sums, cf = run.forward()
    _check_sums(sums, ref, shape, f"mixed w{win}")
    out = run.finalize(sums, 0.0, 1.0)
    _check_finalize(out, ref, f"mixed w{win}", 0.0, 1.0)
    assert np.abs(out[3:] - ref.ssim_planes).max() <= 5e-6          # a swapped or shared plane index is off by more than 1
    got = run.backward(cf, sums, 0.0, 1.0)
    _grad_ratio(got, ref.grad, f"mixed w{win} (0, 1)")
    assert got[0].abs().max() > 0.1 * got.abs().max(), "plane 0 (SSIM < 0) is gated on its own: the gate is on the batch mean"
    for p in range(2):                                              # each plane against its own reference maximum
        _grad_ratio(got[p], ref.grad[p], f"mixed w{win} (0, 1) plane {p}")


def test_l1_ties_have_gradient_zero():
    shape = (2, 9, 33)
    a, b, tie = LU.tie_pair(shape)
    run = Run(a, b, 11)
    sums, cf = run.forward()
    got = run.backward(None, sums, 1.0, 0.0)
    assert (got[tie] == 0.0).all(), "sign(0) must be 0, as torch.sign and nn.L1Loss's backward have it"
    assert np.allclose(got[~tie].double().numpy(), (torch.sign(a - b)[~tie].double() / a.numel()).numpy(), rtol=1e-6, atol=0)
    # with the SSIM term on, a tie carries the SSIM part alone
    ref = LU.loss_and_grad64(a, b, 0.6, 0.4, 11, SIGMA)
    _grad_ratio(run.backward(cf, sums, 0.6, 0.4), ref.grad, "ties 2x9x33 w11 (0.6, 0.4)")
    assert abs(sums.t.cpu().numpy()[:, 0] - ref.l1_sums).max() <= 1e-6 * ref.l1_sums.max()


# ------------------------------------------------------------------------------------------------ image metrics
def _metrics(a, b, win, val_range=1.0):
    n, h, w = a.shape
    ad, bd = a.contiguous().to(U.DEV), b.contiguous().to(U.DEV)
    sums = U.Guarded(torch.zeros(n, 3, dtype=torch.float64))
    out = U.Guarded(torch.full((n, 5), float("nan"), dtype=torch.float64))
    L.call("mrisr_image_metrics", ad.data_ptr(), bd.data_ptr(), sums.data_ptr(), n, h, w, val_range, SIGMA, win, U.stream())
    L.call("mrisr_metrics_finalize", sums.data_ptr(), n, h, w, val_range, out.data_ptr(), U.stream())
    torch.cuda.synchronize()
    sums.check("image_metrics: sums")
    out.check("metrics_finalize: out")
    return out.t.cpu().numpy()


def _check_metrics(got, want, what):
    for i in range(got.shape[0]):
        s, mse, rmse, mae, psnr = got[i]
        _report(f"loss.hip metrics {what}[{i}]: ssim err {abs(s - want[i, 0]):.2e} (bar 5e-6), mse rel {abs(mse - want[i, 1]) / want[i, 1]:.2e}, "
                f"mae rel {abs(mae - want[i, 3]) / want[i, 3]:.2e} (bars 1e-6), psnr err {abs(psnr - want[i, 4]):.2e} (bar 1e-5)")
        assert abs(s - want[i, 0]) <= 5e-6
        assert abs(mse - want[i, 1]) <= 1e-6 * want[i, 1] and abs(mae - want[i, 3]) <= 1e-6 * want[i, 3]
        assert rmse == np.sqrt(mse)
        assert abs(psnr - want[i, 4]) <= 1e-5


@pytest.mark.parametrize("win", [5, 9, 13])
@pytest.mark.parametrize("shape", [(2, 3, 5), (1, 31, 33), (3, 7, 65)], ids=_sid)
def test_image_metrics_against_float64(shape, win):
    a, b = _pair("noisy", shape)
    _check_metrics(_metrics(a, b, win), LU.metrics64(a, b, win, SIGMA), f"{_sid(shape)} w{win}")
    a255, b255 = _pair("noisy", shape, 255.0)
    _check_metrics(_metrics(a255, b255, win, 255.0), LU.metrics64(a255, b255, win, SIGMA, 255.0), f"{_sid(shape)} w{win} val_range 255")
    same = _metrics(a, a, win)
    assert (same[:, 4] == 100.0).all() and (same[:, 1] == 0.0).all() and (same[:, 3] == 0.0).all()
    assert np.abs(same[:, 0] - LU.metrics64(a, a, win, SIGMA)[:, 0]).max() <= 5e-6


def test_psnr_guard_sits_at_1e_minus_10():
    """One pixel of a 31 x 33 image off by 2^-11: mse = 2.33e-10, just above the guard - the logarithm; by 2^-12: 5.8e-11 - 100."""
    a = LU.noisy_pair((1, 31, 33))[0]
    a[0, 15, 16] = 0.5
    for step, guarded in ((2.0 ** -11, False), (2.0 ** -12, True)):
        b = a.clone()
        b[0, 15, 16] = 0.5 + step
        want = LU.metrics64(a, b, 9, SIGMA)
        assert (want[0, 1] < 1e-10) == guarded and 5e-11 < want[0, 1] < 2.5e-10
        got = _metrics(a, b, 9)
        _check_metrics(got, want, f"guard step {step:g}")
        if guarded:
            assert got[0, 4] == 100.0
        else:
            assert 96.0 < got[0, 4] < 96.6


# ------------------------------------------------------------------------------------------------ refusals
def test_windows_outside_the_instantiated_set_are_refused():
    lib = L.load()
    a, b = (t.to(U.DEV) for t in LU.noisy_pair((1, 8, 8)))
    sums2, sums3 = torch.zeros(2, dtype=torch.float64, device=U.DEV), torch.zeros(3, dtype=torch.float64, device=U.DEV)
    coef = torch.zeros(3 * 64, device=U.DEV)
    da = torch.full((64,), 7.0, device=U.DEV)
    for win in (-3, 0, 1, 2, 4, 6, 8, 10, 12, 14, 16, 17, 19):
        assert lib.mrisr_ssim_l1_forward_win(a.data_ptr(), b.data_ptr(), sums2.data_ptr(), coef.data_ptr(), 1, 8, 8, 1.0, SIGMA, win,
                                             U.stream()) == E_UNSUPPORTED, win
        assert b"window_size" in lib.mrisr_last_error()
        assert lib.mrisr_image_metrics(a.data_ptr(), b.data_ptr(), sums3.data_ptr(), 1, 8, 8, 1.0, SIGMA, win, U.stream()) == E_UNSUPPORTED, win
        assert lib.mrisr_ssim_l1_backward_win(a.data_ptr(), b.data_ptr(), coef.data_ptr(), sums2.data_ptr(), None, 0.6, 0.4, da.data_ptr(),
                                              1, 8, 8, SIGMA, win, U.stream()) == E_UNSUPPORTED, win
    # an SSIM term without the coefficient planes
    for ssim_w in (0.4, -1.0):
        assert lib.mrisr_ssim_l1_backward_win(a.data_ptr(), b.data_ptr(), None, sums2.data_ptr(), None, 0.6, ssim_w, da.data_ptr(), 1, 8, 8,
                                              SIGMA, 11, U.stream()) == E_ARG
        assert b"coef" in lib.mrisr_last_error()
    torch.cuda.synchronize()
    assert (sums2 == 0).all() and (sums3 == 0).all() and (da == 7.0).all()          # nothing was launched
