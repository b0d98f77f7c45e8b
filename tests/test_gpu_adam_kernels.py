"""csrc/optim.hip through its C entry points against lossutil.adam64 (torch.optim.Adam in float64 with the Python doubles
0.9 / 0.999; pinned on the CPU by test_loss_ref_host.py): p, m AND v after every step of mrisr_adam_step and
mrisr_adam_step_amp.

Bars: p absolute 2e-6 at lr = 1e-3 (the bar test_gpu_kernels.test_adam_matches_reference holds), m and v 1e-5 of the largest
magnitude of each.  Every buffer carries 64 floats of a sentinel on both sides, which no launch may touch.

What is run: n in {1, 3, 4, 5, 1027, 2048 * 256 * 4 + 4099} (scalar tail only, vector body only, body + tail, several blocks,
a grid-stride loop that wraps); weight_decay 0.5 on |p| ~ 1, where AdamW is > 100 bars away (asserted on the CPU);
grad_scale; a step count of 1000; zero and 1e-10 gradients; the refusals; the GradScaler form: device loss scale, skipped
steps, device step counter, NaN in found_inf, null forms, grad_mul.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mri_superresolution_amd import _lib as L          # noqa: E402
import hiputil as U                                    # noqa: E402
import lossutil as LU                                  # noqa: E402

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
TOL_P, TOL_MV = 2e-6, 1e-5
PAD, SENTINEL = 64, -7.5
E_ARG = -1


def _report(line):
    """The measured figure behind an assertion, in the test's captured output (pytest -rA or -s shows it)."""
    print(line)


class Buf:
    """n floats on a 16-byte boundary with PAD sentinel floats on both sides."""

    def __init__(self, init: torch.Tensor):
        n = init.numel()
        self.n = n
        self.raw = torch.full((2 * PAD + n,), SENTINEL, dtype=torch.float32, device=U.DEV)
        self.t = self.raw[PAD:PAD + n]
        self.t.copy_(init)
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what):
        assert bool((self.raw[:PAD] == SENTINEL).all()) and bool((self.raw[PAD + self.n:] == SENTINEL).all()), f"{what}: padding overwritten"

    def cpu(self):
        return self.t.cpu()


class State:
    def __init__(self, p0):
        self.n = p0.numel()
        self.p, self.m, self.v = Buf(p0), Buf(torch.zeros(self.n)), Buf(torch.zeros(self.n))

    def step(self, g, step, wd=0.0, grad_scale=1.0):
        gb = Buf(g)
        L.call("mrisr_adam_step", self.p.ptr(), gb.ptr(), self.m.ptr(), self.v.ptr(), self.n, LR, B1, B2, EPS, wd, step, grad_scale,
               U.stream())
        torch.cuda.synchronize()
        self._after(gb, g, "adam_step")

    def step_amp(self, g, step_dev, wd=0.0, grad_mul=1.0, loss_scale=None, found_inf=None):
        gb = Buf(g)
        L.call("mrisr_adam_step_amp", self.p.ptr(), gb.ptr(), self.m.ptr(), self.v.ptr(), self.n, LR, B1, B2, EPS, wd, step_dev.data_ptr(),
               grad_mul, L.ptr(loss_scale), L.ptr(found_inf), U.stream())
        torch.cuda.synchronize()
        self._after(gb, g, "adam_step_amp")

    def _after(self, gb, g, what):
        for name, b in (("p", self.p), ("m", self.m), ("v", self.v), ("g", gb)):
            b.check(f"{what} n={self.n}: {name}")
        assert torch.equal(gb.cpu().view(torch.int32), g.view(torch.int32)), f"{what}: the gradient was written"

    def snapshot(self):
        return [b.cpu().clone() for b in (self.p, self.m, self.v)]

    def compare(self, ref, what):
        """(p, m, v) against one entry of adam64; returns the three errors (p absolute, m and v relative to their maxima)."""
        p, m, v = (t.double().numpy() for t in self.snapshot())
        assert np.isfinite(p).all() and np.isfinite(m).all() and np.isfinite(v).all(), what
        ep = np.abs(p - ref[0]).max()
        em = np.abs(m - ref[1]).max() / max(np.abs(ref[1]).max(), 1e-300)
        ev = np.abs(v - ref[2]).max() / max(np.abs(ref[2]).max(), 1e-300)
        _report(f"optim.hip {what}: p abs err {ep:.2e} (bar {TOL_P:.0e}), m rel err {em:.2e}, v rel err {ev:.2e} (bars {TOL_MV:.0e})")
        assert ep <= TOL_P and em <= TOL_MV and ev <= TOL_MV, what
        return ep, em, ev


@pytest.mark.parametrize("n", LU.ADAM_SIZES)
def test_adam_p_m_v_every_size_with_weight_decay(n):
    steps = 2 if n == LU.ADAM_WRAP else 5
    p0, grads = LU.adam_inputs(n, steps)
    ref = LU.adam64(p0, grads, LR, (B1, B2), EPS, wd=0.5)
    if n == 1027:       # the inputs test_loss_ref_host.test_weight_decay_case_tells_adam_from_adamw is about
        aw = LU.adam64(p0, grads, LR, (B1, B2), EPS, wd=0.5, decoupled=True)
        assert all(np.abs(aw[k][0] - ref[k][0]).max() > 100 * TOL_P for k in range(steps))
    st = State(p0)
    for k, g in enumerate(grads):
        st.step(g, k + 1, wd=0.5)
        st.compare(ref[k], f"adam_step n={n} wd=0.5 step {k + 1}")


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
def test_adam_grad_scale_and_late_step_count(grad_scale):
    p0, grads = LU.adam_inputs(1027, 4, seed=8)
    ref = LU.adam64(p0, grads[:3], LR, (B1, B2), EPS, wd=0.0, grad_scale=grad_scale)
    if grad_scale != 1.0:
        plain = LU.adam64(p0, grads[:3], LR, (B1, B2), EPS, wd=0.0)
        assert np.abs(plain[0][1] - ref[0][1]).max() > 100 * TOL_MV * np.abs(ref[0][1]).max()       # an ignored grad_scale shows in m
    st = State(p0)
    for k in range(3):
        st.step(grads[k], k + 1, grad_scale=grad_scale)
        st.compare(ref[k], f"adam_step grad_scale={grad_scale} step {k + 1}")
    # step 1000 on the state left by step 3: the bias corrections are 1 - 0.9^1000 = 1 and 1 - 0.999^1000 = 0.632
    late = LU.adam64(ref[2][0], grads[3:], LR, (B1, B2), EPS, wd=0.0, grad_scale=grad_scale, m0=ref[2][1], v0=ref[2][2], step0=999)
    early = LU.adam64(ref[2][0], grads[3:], LR, (B1, B2), EPS, wd=0.0, grad_scale=grad_scale, m0=ref[2][1], v0=ref[2][2], step0=3)
    assert np.abs(late[0][0] - early[0][0]).max() > 100 * TOL_P
    st.step(grads[3], 1000, grad_scale=grad_scale)
    # (p carries the error of the three steps before: compare the step itself on top of the device's own state as well)
    st.compare(late[0], f"adam_step grad_scale={grad_scale} step 1000")
    fresh = State(p0)
    fresh.step(grads[0], 1000, grad_scale=grad_scale)
    fresh.compare(LU.adam64(p0, grads[:1], LR, (B1, B2), EPS, wd=0.0, grad_scale=grad_scale, step0=999)[0],
                  f"adam_step grad_scale={grad_scale} step 1000 from zero state")


def test_adam_zero_and_tiny_gradients():
    n = 1027
    st = State(torch.zeros(n))
    for k in range(2):
        st.step(torch.zeros(n), k + 1, wd=0.5)
        assert all(bool((t == 0).all()) for t in st.snapshot())          # 0 / (0 + eps): exactly zero, no NaN
    # |g| ~ 1e-10 << eps: the update is lr m / eps-dominated, about 1e-5 a step; p starts at 0 so that the update is all of p
    gen = torch.Generator().manual_seed(12)
    grads = [1e-10 * (1.0 + torch.rand(n, generator=gen)) * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0) for _ in range(3)]
    ref = LU.adam64(torch.zeros(n), grads, LR, (B1, B2), EPS, wd=0.0)
    no_eps = LU.adam64(torch.zeros(n), grads, LR, (B1, B2), 0.0, wd=0.0)
    assert np.abs(no_eps[0][0] - ref[0][0]).max() > 100 * TOL_P
    st = State(torch.zeros(n))
    for k, g in enumerate(grads):
        st.step(g, k + 1)
        st.compare(ref[k], f"adam_step |g| ~ 1e-10 step {k + 1}")
        p = st.p.cpu().double().numpy()
        assert np.abs(p - ref[k][0]).max() <= TOL_MV * np.abs(ref[k][0]).max()       # p is ~ 1e-5 here: held to the relative bar too


def test_adam_refusals():
    lib = L.load()
    n = 64
    bufs = [Buf(torch.ones(n)) for _ in range(4)]
    step_dev = torch.zeros(1, dtype=torch.int32, device=U.DEV)
    ptrs = [b.ptr() for b in bufs]
    for step in (0, -1):
        assert lib.mrisr_adam_step(*ptrs, n - 4, LR, B1, B2, EPS, 0.0, step, 1.0, U.stream()) == E_ARG
        assert b"step" in lib.mrisr_last_error()
    for k in range(4):            # 4 bytes past a 16-byte boundary, each buffer in turn
        off = list(ptrs)
        off[k] += 4
        assert lib.mrisr_adam_step(*off, n - 4, LR, B1, B2, EPS, 0.0, 1, 1.0, U.stream()) == E_ARG
        assert b"aligned" in lib.mrisr_last_error()
        assert lib.mrisr_adam_step_amp(*off, n - 4, LR, B1, B2, EPS, 0.0, step_dev.data_ptr(), 1.0, None, None, U.stream()) == E_ARG
        assert b"aligned" in lib.mrisr_last_error()
    assert lib.mrisr_adam_step_amp(*ptrs, n, LR, B1, B2, EPS, 0.0, None, 1.0, None, None, U.stream()) == E_ARG
    torch.cuda.synchronize()
    assert all(bool((b.raw[PAD:PAD + n] == 1.0).all()) for b in bufs) and int(step_dev.item()) == 0       # nothing was launched


# ------------------------------------------------------------------------------------------------ GradScaler form
def _dev_f32(v):
    return torch.tensor([v], dtype=torch.float32, device=U.DEV)


@pytest.mark.parametrize("n", [5, 1027])
def test_adam_amp_unscale_skip_and_device_step_count(n):
    scale = 1024.0
    p0, grads = LU.adam_inputs(n, 6, seed=9)
    skip = [False, True, False, False, True, False]
    ref = LU.adam64(p0, grads, LR, (B1, B2), EPS, wd=0.5, skip_mask=skip)
    unscaled_dropped = LU.adam64(p0, [g * scale for g in grads], LR, (B1, B2), EPS, wd=0.5, skip_mask=skip)
    assert np.abs(unscaled_dropped[0][1] - ref[0][1]).max() > 100 * TOL_MV * np.abs(ref[0][1]).max()
    st = State(p0)
    step_dev = torch.zeros(1, dtype=torch.int32, device=U.DEV)
    ls = _dev_f32(scale)
    for k, g in enumerate(grads):
        gk = g * scale
        if skip[k]:
            gk[0], gk[-1] = float("inf"), float("nan")
        before, count = st.snapshot(), int(step_dev.item())
        st.step_amp(gk, step_dev, wd=0.5, loss_scale=ls, found_inf=_dev_f32(1.0 if skip[k] else 0.0))
        if skip[k]:
            after = st.snapshot()
            assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(before, after)), f"step {k + 1}: a skipped step wrote"
            assert int(step_dev.item()) == count
        else:
            assert int(step_dev.item()) == count + 1
        assert int(step_dev.item()) == ref[k][3]
        st.compare(ref[k], f"adam_step_amp n={n} loss_scale 1024 step {k + 1}{' (skipped)' if skip[k] else ''}")
    assert int(step_dev.item()) == 4
    # NaN in found_inf counts as set
    before = st.snapshot()
    st.step_amp(grads[0] * scale, step_dev, wd=0.5, loss_scale=ls, found_inf=_dev_f32(float("nan")))
    assert all(torch.equal(x, y) for x, y in zip(before, st.snapshot())) and int(step_dev.item()) == 4


@pytest.mark.parametrize("n", [5, 1027, LU.ADAM_WRAP])
def test_adam_amp_null_forms_and_grad_mul_match_the_plain_kernel(n):
    steps = 2 if n == LU.ADAM_WRAP else 4
    p0, grads = LU.adam_inputs(n, steps, seed=10)
    ref = LU.adam64(p0, grads, LR, (B1, B2), EPS, wd=0.5, grad_scale=0.5)
    plain, forms = State(p0), {"null": State(p0), "found_inf only": State(p0), "loss_scale only": State(p0)}
    counters = {k: torch.zeros(1, dtype=torch.int32, device=U.DEV) for k in forms}
    zero, one = _dev_f32(0.0), _dev_f32(1.0)
    for k, g in enumerate(grads):
        plain.step(g, k + 1, wd=0.5, grad_scale=0.5)
        plain.compare(ref[k], f"adam_step n={n} grad_scale 0.5 step {k + 1}")
        forms["null"].step_amp(g, counters["null"], wd=0.5, grad_mul=0.5)
        forms["found_inf only"].step_amp(g, counters["found_inf only"], wd=0.5, grad_mul=0.5, found_inf=zero)
        forms["loss_scale only"].step_amp(g, counters["loss_scale only"], wd=0.5, grad_mul=0.5, loss_scale=one)
        want = [t.double().numpy() for t in plain.snapshot()]
        for name, st in forms.items():
            st.compare(ref[k], f"adam_step_amp n={n} {name} grad_mul 0.5 step {k + 1}")
            st.compare(want, f"adam_step_amp n={n} {name} grad_mul 0.5 step {k + 1} against adam_step")
            assert int(counters[name].item()) == k + 1


def test_adam_amp_bias_correction_follows_the_device_counter():
    """The counter at 999: the kernel forms 1 - 0.9^1000 and 1 - 0.999^1000 in float32 from it."""
    p0, grads = LU.adam_inputs(1027, 1, seed=11)
    late = LU.adam64(p0, grads, LR, (B1, B2), EPS, wd=0.0, step0=999)
    first = LU.adam64(p0, grads, LR, (B1, B2), EPS, wd=0.0)
    assert np.abs(late[0][0] - first[0][0]).max() > 100 * TOL_P
    st = State(p0)
    step_dev = torch.full((1,), 999, dtype=torch.int32, device=U.DEV)
    st.step_amp(grads[0], step_dev)
    st.compare(late[0], "adam_step_amp counter 999 -> step 1000")
    assert int(step_dev.item()) == 1000
