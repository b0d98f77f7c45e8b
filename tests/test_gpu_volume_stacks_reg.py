"""GPU tests of the regularised update of the reconstruction from orthogonal stacks (``mrisr_f32_volume_stack_update_reg`` of
csrc/volume_stacks.hip through mri_superresolution_amd/volume_stacks.py): the kernel and the whole loop against the numpy
specification, bit for bit."""
import functools
import math

import numpy as np
import pytest
import torch

import stackregutil as R
import stackutil as U
from mri_superresolution_amd import _lib
from mri_superresolution_amd import volume_stacks as S

pytestmark = pytest.mark.gpu

OUT = R.OUT


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                # a copy: the shared cases are read-only


@functools.lru_cache(maxsize=None)
def residuals(K):
    return [(y - np.float32(450)).astype(np.float32) for y in R.case(K)[1]]


@pytest.mark.parametrize("coeffs", [(1.0, 1.0, 1.0), (1.0, 0.25, 0.64)], ids=["iso", "aniso"])
@pytest.mark.parametrize("delta", [math.inf, 40.0])
@pytest.mark.parametrize("clamp", [0.0, None])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_the_regularised_update_is_bit_equal_to_the_specification(K, clamp, delta, coeffs):
    x, _, geometries = R.case(K)
    res = residuals(K)
    want, cnt_want = S.stack_update_np(x, res, geometries, 0.75, clamp, reg_lambda=0.05, reg_delta=delta, reg_coeffs=coeffs)
    if K == 1:                                                # the oblique stack leaves the grid: the neighbour-skip rule is exercised
        assert (cnt_want > 0).sum() == 2681 and R.uncovered_faces(cnt_want) == 990
    d = np.concatenate([np.diff(x, axis=a).reshape(-1) for a in range(3)])
    assert (d > 40.0).any() and (d < -40.0).any() and (np.abs(d) < 40.0).any()      # both branches of the clip and the middle
    xd, rd = dev(x), [dev(r) for r in res]
    got, cnt = S.stack_update(xd, rd, geometries, 0.75, clamp, cover=True, reg_lambda=0.05, reg_delta=delta, reg_coeffs=coeffs)
    assert got is not xd and U.same_bits(got.cpu().numpy(), want) and np.array_equal(cnt.cpu().numpy(), cnt_want)
    assert U.same_bits(xd.cpu().numpy(), x)                                           # the estimate is read only
    out = torch.empty_like(xd)
    again, none = S.stack_update(xd, rd, geometries, 0.75, clamp, out=out, reg_lambda=0.05, reg_delta=delta, reg_coeffs=coeffs, coverage=cnt)
    assert again is out and none is None and U.same_bits(out.cpu().numpy(), want)


@pytest.mark.parametrize("shape", [(1, 1, 1), (8, 8, 32), (1, 11, 70)], ids=str)
def test_tile_edges(shape):
    rng = np.random.default_rng(7)
    x = rng.uniform(0.0, 900.0, shape).astype(np.float32)
    r = rng.uniform(-200.0, 200.0, shape).astype(np.float32)
    a = np.eye(4)
    a[:3, 3] = [0.0, 0.0, 0.0] if shape == (1, 1, 1) else [0.0, -0.25, -0.75]         # off the centres; the last plane along z is not covered
    g = S.stack_geometry(a, np.eye(4), 2, samples=1)
    want, cnt_want = S.stack_update_np(x, [r], [g], 1.0, 0.0, reg_lambda=0.1, reg_delta=40.0)
    got, cnt = S.stack_update(dev(x), [dev(r)], [g], 1.0, 0.0, cover=True, reg_lambda=0.1, reg_delta=40.0)
    assert cnt_want.any() and U.same_bits(got.cpu().numpy(), want) and np.array_equal(cnt.cpu().numpy(), cnt_want)


@functools.lru_cache(maxsize=None)
def reference(K, iterations):
    _, stacks, geometries = R.case(K)
    return S.combine_stacks_np(stacks, geometries, OUT, iterations=iterations, step=1.0, clamp=0.0, fill=-5.0, reg_lambda=0.03)


def same_result(got, want):
    assert U.same_bits(got.volume.cpu().numpy(), want.volume) and U.same_bits(got.initial.cpu().numpy(), want.initial)
    assert np.array_equal(got.counts, want.counts) and np.array_equal(got.coverage, want.coverage)
    # a sum within one spacing (2^-52 relative), then a rounded quotient and a rounded root: below 4 x 2^-53 < 1e-15
    assert got.rms.shape == want.rms.shape and np.allclose(got.rms, want.rms, rtol=1e-15, atol=0.0)


@pytest.mark.parametrize("iterations", [2, 3])
@pytest.mark.parametrize("K", [1, 3])
def test_regularised_combine_stacks_is_bit_equal_to_the_specification(K, iterations):
    _, stacks, geometries = R.case(K)
    got = S.combine_stacks([dev(y) for y in stacks], geometries, OUT, iterations=iterations, fill=-5.0, check=True, reg_lambda=0.03)
    same_result(got, reference(K, iterations))
    plain = S.combine_stacks_np(stacks, geometries, OUT, iterations=1, fill=-5.0)
    assert not U.same_bits(plain.volume, S.combine_stacks_np(stacks, geometries, OUT, iterations=1, fill=-5.0, reg_lambda=0.03).volume)


def test_two_runs_and_a_captured_loop_give_the_same_bits(monkeypatch):
    _, stacks, geometries = R.case(3)
    ys = [dev(y) for y in stacks]
    ws = S.StackWorkspace(OUT, [y.shape for y in stacks], "cuda", iterations=3, regularised=True)
    reads = []
    for name in ("cpu", "item", "tolist"):
        real = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _real=real, _name=name, **k: (reads.append(_name), _real(self, *a, **k))[1])
    eager = S.combine_stacks(ys, geometries, OUT, iterations=3, fill=-5.0, workspace=ws, reg_lambda=0.03)
    assert reads == ["cpu"]                                                  # the one device-to-host read, after the loop
    second = S.combine_stacks(ys, geometries, OUT, iterations=3, fill=-5.0, workspace=ws, reg_lambda=0.03)
    captured = S.combine_stacks(ys, geometries, OUT, iterations=3, fill=-5.0, workspace=ws, graph=True, check=True, reg_lambda=0.03)
    assert reads == ["cpu"] * 3                # a captured loop cannot read the device: a synchronisation would end the capture
    monkeypatch.undo()
    for other in (second, captured):
        assert U.same_bits(other.volume.cpu().numpy(), eager.volume.cpu().numpy())
        assert np.array_equal(other.rms.view(np.uint64), eager.rms.view(np.uint64)) and np.array_equal(other.counts, eager.counts)
    same_result(captured, reference(3, 3))


def test_lambda_zero_on_a_regularised_workspace_is_the_plain_loop():
    _, stacks, geometries = R.case(3)
    ys = [dev(y) for y in stacks]
    ws = S.StackWorkspace(OUT, [y.shape for y in stacks], "cuda", iterations=3, regularised=True)
    plain = S.combine_stacks(ys, geometries, OUT, iterations=3, fill=-5.0)
    got = S.combine_stacks(ys, geometries, OUT, iterations=3, fill=-5.0, workspace=ws, reg_lambda=0.0, reg_delta=40.0)
    assert U.same_bits(got.volume.cpu().numpy(), plain.volume.cpu().numpy()) and U.same_bits(got.initial.cpu().numpy(), plain.initial.cpu().numpy())
    assert np.array_equal(got.rms.view(np.uint64), plain.rms.view(np.uint64)) and np.array_equal(got.coverage, plain.coverage)


def test_a_nan_voxel_spreads_as_in_the_specification():
    x, _, geometries = R.case(3)
    x = x.copy()
    x[4, 5, 33] = np.nan                                       # next to the boundary of two tiles along z
    res = residuals(3)
    want = S.stack_update_np(x, res, geometries, 0.75, 0.0, reg_lambda=0.05, reg_delta=40.0)[0]
    got = S.stack_update(dev(x), [dev(r) for r in res], geometries, 0.75, 0.0, reg_lambda=0.05, reg_delta=40.0)[0].cpu().numpy()
    nan = np.isnan(want)
    assert nan.sum() == 7 and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def test_wrappers_refuse_what_they_cannot_run():
    x, stacks, geometries = R.case(3)
    xd, ys = dev(x), [dev(y) for y in stacks]
    with pytest.raises(ValueError, match="out must be another tensor"):
        S.stack_update(xd, ys, geometries, out=xd, reg_lambda=0.05)
    with pytest.raises(ValueError, match="regularised=True"):
        S.combine_stacks(ys, geometries, OUT, iterations=3, reg_lambda=0.03,
                         workspace=S.StackWorkspace(OUT, [y.shape for y in ys], "cuda", iterations=3))
    for bad in (dict(reg_lambda=-1.0), dict(reg_lambda=math.nan), dict(reg_lambda=0.05, reg_delta=0.0), dict(reg_lambda=0.05, reg_delta=math.nan),
                dict(reg_lambda=0.05, reg_coeffs=(1.0, 0.0, 1.0)), dict(reg_lambda=0.05, reg_coeffs=(1.0, 1.0))):
        with pytest.raises(ValueError, match="reg_"):
            S.stack_update(xd, ys, geometries, **bad)
        with pytest.raises(ValueError, match="reg_"):
            S.combine_stacks(ys, geometries, OUT, iterations=1, **bad)
    with pytest.raises(ValueError, match="stability bound"):
        S.stack_update(xd, ys, geometries, reg_lambda=0.17)
    with pytest.raises(ValueError, match="stability bound"):
        S.combine_stacks(ys, geometries, OUT, iterations=1, step=2.0, reg_lambda=0.1)
    cover = torch.ones(OUT, dtype=torch.uint8, device="cuda")
    for bad in (cover.float(), cover[:8], cover.cpu(), cover.transpose(0, 1), np.ones(OUT, dtype=np.uint8)):
        with pytest.raises(ValueError, match="coverage"):
            S.stack_update(xd, ys, geometries, reg_lambda=0.05, coverage=bad)


def test_the_entry_point_refuses_before_any_launch():
    lib = _lib.load()
    x, stacks, geometries = R.case(3)
    xd, yd = dev(x), dev(stacks[0])
    out = torch.full_like(xd, 7.0)
    cover_in = torch.ones(OUT, dtype=torch.uint8, device="cuda")
    cover = torch.full(OUT, 9, dtype=torch.uint8, device="cuda")
    slots = torch.empty(lib.mrisr_f32_volume_stack_workspace_bytes(3) // 8, dtype=torch.int64, device="cuda")
    views = S._views_arg([yd], geometries[:1])
    st = torch.cuda.current_stream().cuda_stream
    C = _lib.C
    ARG, SHAPE = -1, -2

    def update(views=views, K=1, step=1.0, use=1, lo=0.0, lam=0.05, delta=40.0, c=(1.0, 1.0, 1.0), cin=cover_in.data_ptr(), o=out.data_ptr(),
               cov=cover.data_ptr(), ws=None, rows=None, shape=OUT):
        return lib.mrisr_f32_volume_stack_update_reg(xd.data_ptr(), *shape, views, K, step, use, lo, lam, delta,
                                                     None if c is None else (C.c_float * 3)(*c), cin, o, cov, ws, rows, st)

    assert update(views=None) == ARG and update(o=None) == ARG and update(cin=None) == ARG and update(c=None) == ARG
    assert update(K=0) == ARG and update(K=9) == ARG and update(o=out.data_ptr() + 2) == ARG
    assert update(step=float("nan")) == ARG and update(lo=float("-inf")) == ARG and update(use=-1) == ARG
    assert update(o=xd.data_ptr()) == ARG and update(o=yd.data_ptr()) == ARG
    assert update(cin=xd.data_ptr()) == ARG and update(cin=out.data_ptr()) == ARG
    assert update(cov=yd.data_ptr()) == ARG and update(cov=xd.data_ptr()) == ARG and update(cov=cover_in.data_ptr()) == ARG
    assert update(lam=-0.5) == ARG and update(lam=math.nan) == ARG and update(delta=0.0) == ARG and update(delta=math.nan) == ARG
    assert update(c=(1.0, -1.0, 1.0)) == ARG and update(c=(math.inf, 1.0, 1.0)) == ARG
    assert update(lam=0.17) == ARG and update(lam=0.1, step=2.0) == ARG and update(lam=0.1, c=(2.0, 2.0, 2.0)) == ARG
    assert update(ws=slots.data_ptr()) == ARG and update(rows=slots.data_ptr()) == ARG and update(shape=(9, 0, 70)) == SHAPE
    torch.cuda.synchronize()
    assert (out == 7.0).all().item() and (cover == 9).all().item()           # nothing was launched
