"""Slice-to-volume motion correction on the device against its numpy specification: the per-slice residual and update bit for bit
(slice axes 0, 1, 2, an oblique stack, T = 1 and 4, poses that open a gap, overlap two slices and push one out of the volume, K = 1
and 3, extents that are no multiple of a brick), the slice cost (counts equal, sums within 1e-12, the same bits on every run), the
search on the moved phantom stacks, the graph replay of the motion rounds, and the per-slice residual with the stack's own matrix
repeated against the plain residual kernel (one shared body: the same bits)."""
import functools

import numpy as np
import pytest
import torch

import sliceutil as U
from mri_superresolution_amd import volume_slices as V
from mri_superresolution_amd import volume_stacks as S
from stackutil import oblique_affine, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _estimate():
    rng = np.random.default_rng(5)
    x = rng.uniform(0.0, 900.0, U.SMALL_OUT).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _case(axis, slices, oblique=False, samples=None):
    """-> ``(y, g, to_output_s, from_output_s)`` of a small stack under the hand-made poses."""
    y, g, a = U.small_stack(axis, slices, oblique)
    if samples is not None:
        g = S.stack_geometry(a, np.eye(4), axis, "box", samples=samples)
    M, N = V.slice_geometries(a, np.eye(4), y.shape, axis, U.hand_poses(slices, axis, float(S.voxel_sizes(a)[axis])))
    return y, g, M, N


CASES = [(0, 5, False, None), (1, 7, False, None), (2, 5, False, 1), (2, 7, True, 4), (1, 1, False, None), (0, 5, True, 4)]


@pytest.mark.parametrize("axis,slices,oblique,samples", CASES)
def test_residual_slices_bit_equal(axis, slices, oblique, samples):
    y, g, M, _ = _case(axis, slices, oblique, samples)
    x = _estimate()
    r_np, (s_np, n_np) = V.stack_residual_slices_np(x, y, g, M)
    r, s, n = V.stack_residual_slices(_dev(x), _dev(y), g, M)
    assert same_bits(r.cpu().numpy(), r_np) and int(n) == n_np
    assert abs(float(s) - s_np) <= np.spacing(s_np)
    if slices >= 5:                                                   # the slice pushed out of the volume holds no residual
        assert not np.take(r_np, slices - 1, axis=axis).any() and 0 < n_np < y.size


@pytest.mark.parametrize("cases", [[CASES[0]], [CASES[2]], [CASES[4]], [CASES[0], CASES[1], CASES[3]], [CASES[5], CASES[2], CASES[4]]])
def test_update_slices_bit_equal(cases):
    x = _estimate()
    stacks = [_case(*c) for c in cases]
    res = [V.stack_residual_slices_np(x, y, g, M)[0] for y, g, M, _ in stacks]
    geometries, tables = [c[1] for c in stacks], [c[3] for c in stacks]
    for step, clamp in ((1.0, 0.0), (0.7, None)):
        want, cnt_np = V.stack_update_slices_np(x, res, geometries, tables, step, clamp)
        got, cnt = V.stack_update_slices(_dev(x), [_dev(r) for r in res], geometries, tables, step, clamp, cover=True)
        assert np.array_equal(cnt.cpu().numpy(), cnt_np) and same_bits(got.cpu().numpy(), want)
    assert 0 < int((cnt_np > 0).sum()) < cnt_np.size                  # gaps and the grid's rim stay uncovered
    # in place, with tables that lie on the device already
    xd = _dev(x)
    out, none = V.stack_update_slices(xd, [_dev(r) for r in res], geometries, [_dev(t.reshape(-1, 12)) for t in tables], 0.7, None, out=xd)
    assert out is xd and none is None and same_bits(xd.cpu().numpy(), want)


def test_slices_reject_cpu_tensors_and_regulariser():
    y, g, M, N = _case(0, 5)
    x = _estimate()
    with pytest.raises(ValueError, match="no CPU fallback"):
        V.stack_residual_slices(torch.from_numpy(x.copy()), torch.from_numpy(y), g, M)
    with pytest.raises(ValueError, match="no CPU fallback"):
        V.stack_update_slices(torch.from_numpy(x.copy()), [torch.from_numpy(y)], [g], [N])
    with pytest.raises(ValueError, match="no CPU fallback"):
        V.slice_cost(torch.from_numpy(x.copy()), torch.from_numpy(y), g, M[:, None])
    with pytest.raises(NotImplementedError, match="not built"):
        V.stack_update_slices(_dev(x), [_dev(y)], [g], [N], reg_lambda=0.05)
    with pytest.raises(ValueError):
        V.stack_residual_slices(_dev(x), _dev(y), g, M[:4])


def _candidates(axis, slices, oblique, C, seed):
    y, g, a = U.small_stack(axis, slices, oblique)
    rng = np.random.default_rng(seed)
    base = U.hand_poses(slices, axis, float(S.voxel_sizes(a)[axis]))
    cands = base[:, None, :] + rng.uniform(-1.0, 1.0, (slices, C, 6)) * ([1.0] * 3 + [3.0] * 3)
    return y, g, np.stack([V.slice_geometries(a, np.eye(4), y.shape, axis, cands[:, c])[0] for c in range(C)], axis=1)


@pytest.mark.parametrize("axis,slices,oblique,C,stride", [(2, 7, True, 13, 1), (0, 5, False, 13, 2), (1, 7, False, 1, 2), (1, 1, False, 1, 1)])
def test_slice_cost(axis, slices, oblique, C, stride):
    y, g, cand = _candidates(axis, slices, oblique, C, 11)
    x = _estimate()
    want = V.slice_cost_np(x, y, g, cand, stride)
    xd, yd = _dev(x), _dev(y)
    ws = V.SliceCostWorkspace(DEV, slices, C)
    first = V.slice_cost(xd, yd, g, cand, stride, ws).cpu().numpy().copy()
    for buf in (ws.slots, ws.out, ws.cand):                           # garbage in the workspace in between
        buf.view(torch.int64).fill_(0x7FF8DEADBEEF0000)
    second = V.slice_cost(xd, yd, g, cand, stride, ws).cpu().numpy()
    assert np.array_equal(first.view(np.uint64), second.view(np.uint64))
    assert first.shape == want.shape == (slices, C, 6) and np.array_equal(first[..., 0], want[..., 0])
    assert np.abs(first - want).max() <= 1e-12 * np.abs(want).max() and (np.abs(first - want) <= 1e-12 * np.abs(want)).all()
    if slices >= 5:
        assert not want[slices - 1].any() and want[..., 0].max() > 0.5 * V.strided_slice_count(y.shape, axis, stride)


@functools.lru_cache(maxsize=None)
def _moved():
    truth = U.structured_phantom()
    return (truth,) + U.moved_stacks(truth, 2, seed=0)


def test_register_slices_recovers_poses():
    """Against the true volume as the target, where the CPU specification leaves 0.7665 of the injected RMS corner displacement
    (1.834 of 2.392 mm: sliceutil, stack 2, limits 3 mm / 6 degrees; measured with register_slices_np - the through-plane part of a
    thick slice's pose is weakly determined): the bound is that plus a quarter of the gap to 1."""
    truth, stacks, geometries, affines, params = _moved()
    k = 2
    m = V.register_slices(_dev(truth), _dev(stacks[k]), geometries[k], affines[k], np.eye(4), limits=(3.0, 6.0))
    left = U.rms_corner_displacement([m.params], [params[k]], [affines[k]], [stacks[k].shape], [geometries[k]], [m.active])
    injected = U.rms_corner_displacement([params[k]], [np.zeros_like(params[k])], [affines[k]], [stacks[k].shape], [geometries[k]], [m.active])
    print(f"left {left:.4f} mm of {injected:.4f} mm injected, {int(m.active.sum())} of {m.active.size} slices active")
    assert m.active.sum() >= m.active.size - 3 and np.abs(m.params[:, :3]).max() <= 3.0 and np.abs(m.params[:, 3:]).max() <= 6.0
    assert np.array_equal(m.params[~m.active], np.zeros((int((~m.active).sum()), 6)))
    assert left / injected <= REGISTER_RATIO + 0.25 * (1 - REGISTER_RATIO)


REGISTER_RATIO = 0.7665


def test_combine_stacks_motion_graph_equals_eager():
    truth, stacks, geometries, affines, params = _moved()
    ys = [_dev(y) for y in stacks]
    motion = U.motion_options(affines, rounds=1, limit_mm=3.0, limit_deg=6.0, levels=tuple([(2, (1.0,) * 3 + (2.0,) * 3, 0.5)] for _ in stacks))
    ws = S.StackWorkspace(truth.shape, [y.shape for y in stacks], DEV, 2, motion=True)
    eager = S.combine_stacks(ys, geometries, truth.shape, 2, workspace=ws, motion=motion)
    graph = S.combine_stacks(ys, geometries, truth.shape, 2, workspace=ws, motion=motion, graph=True)
    assert same_bits(eager.volume.cpu().numpy(), graph.volume.cpu().numpy()) and same_bits(eager.initial.cpu().numpy(), graph.initial.cpu().numpy())
    assert all(np.array_equal(a, b) for a, b in zip(eager.motion, graph.motion)) and np.array_equal(eager.counts, graph.counts)
    assert np.array_equal(eager.rms.view(np.uint64), graph.rms.view(np.uint64)) and np.array_equal(eager.coverage, graph.coverage)
    assert eager.motion_cost.shape == (1, 3, 2) and any(np.abs(p).max() > 0 for p in eager.motion)
    # the rebuild is the specification's on the poses the device found
    tables = [V.slice_geometries(a, np.eye(4), y.shape, g.slice_axis, p) for a, y, g, p in zip(affines, stacks, geometries, eager.motion)]
    want = S._reconstruct_np(stacks, truth.shape, 2, 0.0,
                             *V._slice_steps_np(stacks, geometries, [t[0] for t in tables], [t[1] for t in tables], 1.0, 0.0))
    assert same_bits(eager.volume.cpu().numpy(), want[0]) and same_bits(eager.initial.cpu().numpy(), want[1])
    # without the keyword nothing changes
    plain = S.combine_stacks(ys, geometries, truth.shape, 2)
    assert plain.motion is None and same_bits(plain.volume.cpu().numpy(), S.combine_stacks_np(stacks, geometries, truth.shape, 2).volume)
    with pytest.raises(NotImplementedError, match="not built"):
        S.combine_stacks(ys, geometries, truth.shape, 2, reg_lambda=0.03, motion=motion)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_residual_repeated_tables_bit_equal_on_device(axis):
    """The device twin of ``test_residual_repeated_tables_bit_equal``: the stack's own matrix S times gives the bits of the plain
    kernel - ``r``, the sum and the count.  Both kernels run one shared body; the test guards against the two drifting apart."""
    rng = np.random.default_rng(40 + axis)
    shape_out, shape = (12, 10, 9), [7, 9, 11]
    shape[axis] = 5
    voxel = [1.0, 1.0, 1.0]
    voxel[axis] = (shape_out[axis] - 2.0) / 5
    a = oblique_affine(shape_out, shape, voxel, (6.0, -8.0, 11.0), (0.3, -0.2, 0.4))
    g = S.stack_geometry(a, np.eye(4), axis, "gaussian", samples=3)
    x, y = _dev(rng.uniform(0.0, 900.0, shape_out).astype(np.float32)), _dev(rng.uniform(0.0, 900.0, shape).astype(np.float32))
    table = np.repeat(g.to_output[None], 5, axis=0)
    r0, s0, n0 = S.stack_residual(x, y, g)
    r1, s1, n1 = V.stack_residual_slices(x, y, g, table)
    assert same_bits(r0.cpu().numpy(), r1.cpu().numpy()) and r0.cpu().numpy().any()
    assert int(s0.view(torch.int64)) == int(s1.view(torch.int64)) and int(n0) == int(n1) and 0 < int(n0) <= y.numel()
