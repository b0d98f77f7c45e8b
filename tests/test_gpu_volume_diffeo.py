"""GPU tests of the diffeomorphic variant of the deformable registration (csrc/volume_deform.hip through
mri_superresolution_amd/volume_deform.py): the composition, the update-only force, the exponential, the one interpolation through
matrix and field and the registration against the numpy specification, bit for bit."""
import functools

import numpy as np
import pytest
import torch

from deformutil import messy_field, messy_volume, on_device, phantom, same_bits, smooth_field
from mri_superresolution_amd import volume_deform as D

pytestmark = pytest.mark.gpu

# (5, 7, 70) and (3, 4, 130): odd extents, more than one 2 x 2 x 64 brick on every axis, no multiple of the smoothing tiles;
# (1, 6, 9): an axis of extent 1; (24, 28, 32): the phantom's grid
SHAPES = [(5, 7, 70), (3, 4, 130), (1, 6, 9), (24, 28, 32)]


def seed_of(shape):
    return shape[0] * 10007 + shape[1] * 101 + shape[2]


def past_every_face(shape):
    """A smooth field whose displacements leave the grid through all six faces: -+ (n + 1.25) at the two ends of every axis."""
    u = smooth_field(shape, seed_of(shape) + 5)
    for a, n in enumerate(shape):
        if n == 1:                                   # one plane cannot leave through both faces and stay a test of anything else
            continue
        index = [slice(None)] * 3
        index[a] = 0
        u[a][tuple(index)] = -(n + 1.25)
        index[a] = n - 1
        u[a][tuple(index)] = n + 1.25
    return u


def field_of(shape, kind):
    return {"messy": lambda: messy_field(shape, seed_of(shape)), "smooth": lambda: smooth_field(shape, seed_of(shape)),
            "past": lambda: past_every_face(shape)}[kind]()


KINDS = ("messy", "smooth", "past")


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_compose_is_bit_equal_to_the_specification(shape, offset):
    for ku in ("smooth", "messy"):
        u = field_of(shape, ku)
        for kv in KINDS:
            v = field_of(shape, kv) if kv != ku else field_of(shape, kv)[::-1].copy()
            want = D.compose_np(u, v)
            got = D.compose(on_device(u, offset), on_device(v, offset))
            assert same_bits(got.cpu().numpy(), want), (ku, kv)
    out = on_device(np.zeros_like(u), offset)
    assert D.compose(on_device(u), on_device(v), out=out) is out and same_bits(out.cpu().numpy(), want)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_compose_squares_a_field_given_twice(shape):
    for kind in KINDS:
        w = field_of(shape, kind)
        t = on_device(w)
        got = D.compose(t, t)                                        # one pointer for both inputs
        assert same_bits(got.cpu().numpy(), D.compose_np(w, w)), kind
        assert same_bits(t.cpu().numpy(), w)


def test_compose_refuses_an_aliased_output_and_other_shapes():
    u, v = (on_device(smooth_field((4, 5, 6), s)) for s in (1, 2))
    for bad in (u, v):
        with pytest.raises(ValueError, match="out must be another"):
            D.compose(u, v, out=bad)
    with pytest.raises(ValueError):
        D.compose(u, v[:, :3].contiguous())
    with pytest.raises(ValueError):
        D.compose(u, v, out=torch.empty_like(u, dtype=torch.float64))
    with pytest.raises(ValueError, match="out must be another"):
        D.demons_update(u[0], u[1], v, out=v)
    with pytest.raises(ValueError, match="out must be another"):
        D.warp_matrix(u[0], np.eye(4)[:3], v, out=u[0])


@pytest.mark.parametrize("scale", [1.0, 0.25])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_demons_update_is_bit_equal_to_the_specification(shape, scale):
    rng = np.random.default_rng(seed_of(shape))
    for kind, specials in (("messy", True), ("smooth", False)):
        fixed, moving = messy_volume(shape, seed_of(shape) + 1, specials), messy_volume(shape, seed_of(shape) + 2, specials)
        if kind == "smooth":
            moving = (fixed + rng.normal(0, 30, shape)).astype(np.float32)          # differences of the size of the gradients
        u = field_of(shape, kind)
        want, (s_want, n_want) = D.demons_update_np(fixed, moving, u, max_step=0.4, fill=2.0, scale=scale)
        args = (on_device(fixed, 1), on_device(moving), on_device(u, 1))
        got, s, n = D.demons_update(*args, max_step=0.4, fill=2.0, scale=scale)
        assert same_bits(got.cpu().numpy(), want), kind
        assert int(n) == n_want and abs(float(s) - s_want) <= np.spacing(s_want), (kind, float(s), s_want)
        out = on_device(np.zeros_like(u))
        again, s2, n2 = D.demons_update(*args, max_step=0.4, fill=2.0, scale=scale, out=out)
        assert again is out and same_bits(out.cpu().numpy(), want)
        assert np.float64(float(s2)).view(np.uint64) == np.float64(float(s)).view(np.uint64) and int(n2) == int(n)      # the same bits
        # the additive entry shares the kernel: its bits are those of its own specification still
        v, sv, nv = D.demons_force(*args, max_step=0.4, fill=2.0)
        assert same_bits(v.cpu().numpy(), D.demons_force_np(fixed, moving, u, max_step=0.4, fill=2.0)[0])
        assert np.float64(float(sv)).view(np.uint64) == np.float64(float(s)).view(np.uint64) and int(nv) == int(n)


@pytest.mark.parametrize("steps", [0, 1, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_exp_field_is_bit_equal_to_the_specification(shape, steps):
    for kind in KINDS:
        w = field_of(shape, kind)
        t = on_device(w, 1)
        want = D.exp_field_np(w, steps)
        assert same_bits(D.exp_field(t, steps).cpu().numpy(), want), kind
        assert same_bits(t.cpu().numpy(), w)
    out = on_device(np.zeros_like(w))
    assert D.exp_field(t, steps, out=out) is out and same_bits(out.cpu().numpy(), want)


ROTATED = np.array([[0.9 * 0.8, -0.6 * 1.3, 0.0, 1.7], [0.9 * 0.6, 0.8 * 1.3, 0.05, -2.2], [0.02, 0.0, 0.5, 0.3]])


@pytest.mark.parametrize("method", ["linear", "cubic"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_warp_matrix_is_bit_equal_to_the_specification(shape, method):
    src_shape = (9, 7, 11)
    src = messy_volume(src_shape, seed_of(shape) + 3)
    spread = np.diag([(s - 1) / max(n - 1, 1) for s, n in zip(src_shape, shape)])       # the grid spread over the source
    matrices = [ROTATED, np.hstack([spread, np.array([[0.25], [-0.125], [0.5]])])]
    for kind in ("messy", "past", "smooth"):
        u = field_of(shape, kind)
        for m in matrices:
            want = D.warp_matrix_np(src, m, u, method, fill=-3.5)
            got = D.warp_matrix(on_device(src, 1), m, on_device(u), method, fill=-3.5)
            assert same_bits(got.cpu().numpy(), want), kind
    assert (want != np.float32(-3.5)).sum() > want.size // 4                            # the smooth field stays inside the source mostly
    out = on_device(np.zeros(shape, dtype=np.float32), 1)
    assert D.warp_matrix(on_device(src), m, on_device(u), method, fill=-3.5, out=out) is out and same_bits(out.cpu().numpy(), want)
    # by construction: the reslice for a zero field, the warp for the identity matrix
    from mri_superresolution_amd.volume_reslice import reslice
    zero = torch.zeros((3,) + shape, device="cuda")
    assert same_bits(D.warp_matrix(on_device(src), ROTATED, zero, method, 1.5).cpu().numpy(),
                     reslice(on_device(src), ROTATED, shape, method, 1.5).cpu().numpy())
    own = messy_volume(shape, seed_of(shape) + 4)
    assert same_bits(D.warp_matrix(on_device(own), np.eye(4)[:3], on_device(u), method, 1.5).cpu().numpy(),
                     D.warp(on_device(own), on_device(u), method, 1.5).cpu().numpy())


# ---------------------------------------------------------------- the whole registration

SCHEDULE = dict(levels=2, iterations=(4, 3), sigma_vox=1.5)


@functools.lru_cache(maxsize=None)
def reference(method="linear", exp_steps=2):
    fixed, moving = phantom()[:2]
    return D.register_diffeomorphic_np(fixed, moving, method=method, exp_steps=exp_steps, **SCHEDULE)


def scans():
    return tuple(torch.from_numpy(v.copy()).cuda() for v in phantom()[:2])


def same_result(got, want):
    assert same_bits(got.field.cpu().numpy(), want.field)
    assert same_bits(got.warped.cpu().numpy(), want.warped)
    assert [n for _, n in got.stats] == [n for _, n in want.stats]
    for (s, _), (s_want, _) in zip(got.stats, want.stats):
        assert abs(s - s_want) <= np.spacing(s_want)
    assert got.jacobian == want.jacobian and got.schedule == want.schedule


@pytest.mark.parametrize("method, exp_steps", [("linear", 2), ("cubic", 2), ("linear", 0), ("linear", 3)])
def test_register_diffeomorphic_is_bit_equal_to_the_specification(method, exp_steps):
    fixed, moving = scans()
    got = D.register_diffeomorphic(fixed, moving, method=method, exp_steps=exp_steps, **SCHEDULE)
    same_result(got, reference(method, exp_steps))
    again = D.register_diffeomorphic(fixed, moving, method=method, exp_steps=exp_steps, **SCHEDULE)
    assert again.stats == got.stats and again.jacobian == got.jacobian             # the same bits on a second run
    assert same_bits(again.field.cpu().numpy(), got.field.cpu().numpy())


def test_a_captured_iteration_loop_equals_the_eager_one():
    fixed, moving = scans()
    ws = D.DiffeoWorkspace(fixed.shape, fixed.device, exp_steps=2, **SCHEDULE)
    eager = D.register_diffeomorphic(fixed, moving, workspace=ws, **SCHEDULE)
    captured = D.register_diffeomorphic(fixed, moving, workspace=ws, graph=True, **SCHEDULE)
    assert same_bits(captured.field.cpu().numpy(), eager.field.cpu().numpy())
    assert same_bits(captured.warped.cpu().numpy(), eager.warped.cpu().numpy())
    assert captured.stats == eager.stats and captured.jacobian == eager.jacobian
    same_result(captured, reference())


def test_a_workspace_of_another_schedule_is_refused():
    fixed, moving = scans()
    for ws in (D.DiffeoWorkspace(fixed.shape, fixed.device, levels=2, iterations=(4, 2), sigma_vox=1.5, exp_steps=2),
               D.DiffeoWorkspace(fixed.shape, fixed.device, exp_steps=3, **SCHEDULE),
               D.DiffeoWorkspace(fixed.shape, fixed.device, levels=2, iterations=(4, 3), sigma_vox=1.0, exp_steps=2),
               D.DeformWorkspace(fixed.shape, fixed.device, **SCHEDULE)):
        with pytest.raises(ValueError, match="workspace"):
            D.register_diffeomorphic(fixed, moving, workspace=ws, **SCHEDULE)
    with pytest.raises(ValueError, match="workspace"):
        D.register_deformable(fixed, moving, workspace=D.DiffeoWorkspace(fixed.shape, fixed.device, exp_steps=2, **SCHEDULE), **SCHEDULE)


def test_identical_scans_leave_the_field_exactly_zero():
    fixed = torch.from_numpy(phantom()[0].copy()).cuda()
    r = D.register_diffeomorphic(fixed, fixed.clone(), **SCHEDULE)
    assert not r.field.any().item() and r.jacobian == (1.0, 0)
    assert same_bits(r.warped.cpu().numpy(), phantom()[0])
    assert r.stats == [(0.0, 12 * 14 * 16)] * 4 + [(0.0, 24 * 28 * 32)] * 3
