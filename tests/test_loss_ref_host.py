"""Pins tests/lossutil.py - the float64 specification test_gpu_loss_kernels.py and test_gpu_adam_kernels.py hold the kernels
of csrc/loss.hip and csrc/optim.hip to - on the CPU: against the float32 oracle (oracle/losses_ref, oracle/train_ref), the
reference project's recorded values (tests/golden/ssim.npz, ssim_windows.npz) and torch.optim.Adam, and asserts that the
seeded inputs do what the GPU tests use them for (closed clamp gate, planes of opposite SSIM sign, decay that tells Adam from
AdamW).  Bars against the float32 oracle: the project's 5e-6 per-sample SSIM, 1e-5 loss, 2e-4 of the gradient's maximum (the
oracle itself stays within 2e-7, 8e-7 and 5e-6 of float64 on these shapes).
"""
import math
import os

import numpy as np
import pytest
import torch

import lossutil as LU
from oracle import losses_ref
from oracle.train_ref import AdamRef


def _oracle32(a, b, l1_w, ssim_w, win, val_range):
    x = a.unsqueeze(1).clone().requires_grad_(True)
    y = b.unsqueeze(1)
    m = losses_ref.ssim_map(x, y, win, 1.5, val_range)
    total = l1_w * (x - y).abs().mean() + ssim_w * (1 - torch.clamp(m.mean(), 0.0, 1.0))
    total.backward()
    return m.detach().squeeze(1), total.item(), x.grad.squeeze(1).numpy()


@pytest.mark.parametrize("val_range", [1.0, 255.0])
@pytest.mark.parametrize("shape", LU.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_float64_reference_agrees_with_the_float32_oracle(shape, val_range):
    for win in LU.WINDOWS:
        a, b = LU.noisy_pair(shape)
        a, b = a * val_range, b * val_range
        l1_w = 0.6 if val_range == 1.0 else 0.0          # (with an L1 term at 255 the sign dominates and hides the SSIM part)
        ssim_w = 0.4 if val_range == 1.0 else 1.0
        ref = LU.loss_and_grad64(a, b, l1_w, ssim_w, win, 1.5, val_range)
        m32, total32, grad32 = _oracle32(a, b, l1_w, ssim_w, win, val_range)
        m64 = LU.ssim_map64(a, b, win, 1.5, val_range)
        assert m64.dtype == torch.float64 and m64.shape == a.shape
        assert np.abs(m32.double().mean((1, 2)).numpy() - ref.ssim_planes).max() <= 5e-6
        assert abs(float(m64.mean()) - ref.ssim_mean) <= 1e-12
        assert abs(total32 - ref.total) <= 1e-5
        assert np.abs(grad32 - ref.grad).max() <= 2e-4 * np.abs(ref.grad).max()
        # the clamp gate of every loss / gradient comparison on these inputs is open, with room for float32 sums
        assert 0.5 < ref.ssim_mean < 1.0 - 1e-3, (shape, win, ref.ssim_mean)
        assert np.abs(ref.grad).max() > 0


def test_float64_reference_agrees_with_the_recorded_reference_values(golden_dir):
    g = np.load(os.path.join(golden_dir, "ssim.npz"))
    for i in range(5):
        a, b = torch.from_numpy(g[f"a{i}"])[:, 0], torch.from_numpy(g[f"b{i}"])[:, 0]
        ref = LU.loss_and_grad64(a, b, 0.6, 0.4)
        assert abs(ref.ssim_mean - float(g[f"ssim{i}"])) <= 1e-5
        assert np.abs(ref.ssim_planes - g[f"ssim_ps{i}"]).max() <= 5e-6
        assert abs(float(LU.ssim_map64(a, a).mean()) - float(g[f"ssim_self{i}"])) <= 2e-6
        assert abs(ref.total - float(g[f"closs{i}"])) <= 1e-5
        want = g[f"cgrad{i}"][:, 0]
        assert np.abs(ref.grad - want).max() <= 2e-4 * np.abs(want).max()
    g = np.load(os.path.join(golden_dir, "ssim_windows.npz"))
    a, b = torch.from_numpy(g["a"])[:, 0], torch.from_numpy(g["b"])[:, 0]
    for ws in (3, 7, 11, 15):
        ref = LU.loss_and_grad64(a, b, 0.6, 0.4, ws)
        assert abs(ref.ssim_mean - float(g[f"ssim_w{ws}"])) <= 1e-5
        assert np.abs(ref.ssim_planes - g[f"ssim_ps_w{ws}"]).max() <= 5e-6
        assert abs(ref.total - float(g[f"closs_w{ws}"])) <= 1e-5
        for first, second, key in ((a, b, "cga"), (b, a, "cgb")):         # both are symmetric: swap for the second image
            want = g[f"{key}_w{ws}"][:, 0]
            assert np.abs(LU.loss_and_grad64(first, second, 0.6, 0.4, ws).grad - want).max() <= 2e-4 * np.abs(want).max()
        bare = LU.loss_and_grad64(a, b, 0.0, -1.0, ws, clamp=False).grad        # d(mean SSIM), the ssim() form
        want = g[f"ga_w{ws}"][:, 0]
        assert np.abs(bare - want).max() <= 2e-4 * np.abs(want).max()


def test_coefficient_planes_are_the_derivatives_of_the_ssim_term():
    """coef64 restates the header formulas of loss.hip; d(sum S)/dx = G(c0) + 2 x G(c1) + y G(c2) must equal autograd."""
    for shape, win in (((2, 3, 5), 5), ((1, 31, 33), 11), ((3, 7, 65), 13)):
        a, b = LU.noisy_pair(shape)
        c = LU.coef64(a, b, win).unsqueeze(2)
        w = LU.window64(win, 1.5)
        blur = lambda t: torch.nn.functional.conv2d(t, w, padding=win // 2)      # noqa: E731
        x, y = a.double().unsqueeze(1), b.double().unsqueeze(1)
        got = (blur(c[0]) + 2 * x * blur(c[1]) + y * blur(c[2])).squeeze(1).numpy()
        want = LU.loss_and_grad64(a, b, 0.0, -1.0, win, clamp=False, upstream=float(a.numel())).grad
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()


def test_gate_inputs_close_and_open_the_clamp_gate():
    for shape in LU.ANTI_SHAPES:
        for win in LU.WINDOWS:
            a, b = LU.anti_pair(shape)
            ref = LU.loss_and_grad64(a, b, 0.6, 0.4, win)
            assert ref.ssim_mean < -0.3, (shape, win, ref.ssim_mean)
            l1_only = LU.loss_and_grad64(a, b, 0.6, 0.0, win)
            assert np.array_equal(ref.grad, l1_only.grad)                  # closed gate: nothing but the L1 sign
            ne = (a != b).numpy()
            assert ne.mean() > 0.99 and np.allclose(np.abs(ref.grad[ne]), 0.6 / a.numel(), rtol=1e-12)
            # ... and an open gate WOULD show: the SSIM part alone is as large as the L1 part
            ungated = LU.loss_and_grad64(a, b, 0.0, -0.4, win, clamp=False)
            assert np.abs(ungated.grad).max() > 0.5 * 0.6 / a.numel()
    for win in LU.WINDOWS:
        a, b = LU.mixed_batch()
        ref = LU.loss_and_grad64(a, b, 0.0, 1.0, win)
        assert ref.ssim_planes[0] < -0.5 and ref.ssim_planes[1] > 0.99          # a swapped plane index is off by > 1
        assert 0.05 < ref.ssim_mean < 0.5
        assert np.abs(ref.grad[0]).max() > 0.1 * np.abs(ref.grad).max()         # a per-plane gate would zero plane 0
    a, b = LU.anti_pair(LU.ANTI_SHAPES[0])
    assert abs(LU.loss_and_grad64(a, b, 0.6, 0.4).ssim_mean - (-0.64)) < 0.05
    a, b = LU.anti_pair(LU.ANTI_SHAPES[1])
    assert abs(LU.loss_and_grad64(a, b, 0.6, 0.4).ssim_mean - (-0.44)) < 0.05


def test_tie_pair_and_metrics_reference():
    a, b, tie = LU.tie_pair((2, 9, 33))
    assert 0.4 < tie.float().mean() < 0.6
    ref = LU.loss_and_grad64(a, b, 1.0, 0.0)
    assert (ref.grad[tie.numpy()] == 0.0).all() and np.allclose(np.abs(ref.grad[~tie.numpy()]), 1.0 / a.numel(), rtol=1e-12)
    a, b = LU.noisy_pair((2, 20, 24))
    m = LU.metrics64(a, b, 9)
    assert m.shape == (2, 5)
    for i in range(2):
        assert abs(m[i, 0] - float(losses_ref.ssim(a[i][None, None], b[i][None, None], 9))) <= 5e-6
        assert abs(m[i, 4] - losses_ref.psnr(a[i], b[i])) <= 1e-9 and m[i, 2] == math.sqrt(m[i, 1])
    assert LU.metrics64(a, a)[0, 4] == 100.0
    assert LU.metrics64(a * 255, b * 255, 9, val_range=255.0)[0, 4] == pytest.approx(m[0, 4], abs=1e-4)


ADAM_TOL_P = 2e-6


def test_adam64_equals_the_oracle_and_torch_adam():
    p0, grads = LU.adam_inputs()
    skip = [False, True, False, False, True]
    for wd, gs in ((0.5, 1.0), (0.0, 0.125), (1e-2, 0.5)):
        ref = LU.adam64(p0, grads, lr=1e-3, wd=wd, grad_scale=gs)
        sd = {"p": p0.clone()}
        opt32 = AdamRef(sd, lr=1e-3, weight_decay=wd)
        p64 = p0.double().clone().requires_grad_(True)
        opt64 = torch.optim.Adam([p64], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
        for k, g in enumerate(grads):
            opt32.step(sd, {"p": g * gs})
            p64.grad = g.double() * gs
            opt64.step()
            p, m, v, t = ref[k]
            assert t == k + 1
            assert np.abs(sd["p"].numpy() - p).max() <= ADAM_TOL_P
            assert np.abs(opt32.m["p"].numpy() - m).max() <= 1e-5 * np.abs(m).max()
            assert np.abs(opt32.v["p"].numpy() - v).max() <= 1e-5 * np.abs(v).max()
            st = opt64.state[p64]
            assert np.abs(p64.detach().numpy() - p).max() <= 1e-12
            assert np.abs(st["exp_avg"].numpy() - m).max() <= 1e-12 * np.abs(m).max()
            assert np.abs(st["exp_avg_sq"].numpy() - v).max() <= 1e-12 * np.abs(v).max()
        # skipped steps leave everything as it was, the count included; the others are the steps of the shorter list
        sk = LU.adam64(p0, grads, lr=1e-3, wd=wd, grad_scale=gs, skip_mask=skip)
        short = LU.adam64(p0, [g for g, s in zip(grads, skip) if not s], lr=1e-3, wd=wd, grad_scale=gs)
        assert [r[3] for r in sk] == [1, 1, 2, 3, 3]
        for got, want in ((sk[1], sk[0]), (sk[4], sk[3]), (sk[4], short[2])):
            assert all(np.array_equal(x, y) for x, y in zip(got[:3], want[:3]))
    # a late step count, handed over as the state before the step
    late = LU.adam64(p0, grads[:1], wd=0.0, step0=999)[0]
    assert late[3] == 1000 and np.allclose(late[1], 0.1 * grads[0].double().numpy(), rtol=1e-12)


def test_weight_decay_case_tells_adam_from_adamw():
    """|p| ~ 1 and weight_decay 0.5: the decoupled (AdamW) result is more than 100 tolerances away from the L2 one."""
    p0, grads = LU.adam_inputs()
    l2 = LU.adam64(p0, grads, lr=1e-3, wd=0.5)
    aw = LU.adam64(p0, grads, lr=1e-3, wd=0.5, decoupled=True)
    for k in range(len(grads)):
        assert np.abs(l2[k][0] - aw[k][0]).max() > 100 * ADAM_TOL_P
        assert np.abs(l2[k][1] - aw[k][1]).max() > 100 * 1e-5 * np.abs(l2[k][1]).max()
