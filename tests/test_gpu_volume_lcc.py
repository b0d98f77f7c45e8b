"""GPU tests of the force across contrasts (csrc/volume_lcc.hip through mri_superresolution_amd/volume_deform.py): the fused force
and the registrations that use it against the numpy specification, bit for bit."""
import numpy as np
import pytest
import torch

import lccutil
from deformutil import messy_field, messy_volume, on_device, same_bits, smooth_field
from mri_superresolution_amd import volume_deform as D

pytestmark = pytest.mark.gpu

# extents below the radius, extents of 1, tiles (32 x 8 x 32) that do not divide, more than one tile on axes 1 and 2
SHAPES = [(1, 1, 1), (1, 5, 70), (3, 2, 2), (2, 9, 3), (9, 10, 67), (17, 18, 33)]


def seed_of(shape):
    return shape[0] * 10007 + shape[1] * 101 + shape[2]


def same_double(a, b):
    return np.float64(float(a)).view(np.uint64) == np.float64(float(b)).view(np.uint64)


def pair(shape, kind):
    """(fixed, moving, field): messy volumes with specials under a messy field, or a noisy other contrast under a smooth one."""
    seed = seed_of(shape)
    if kind == "messy":
        return messy_volume(shape, seed + 1, True), messy_volume(shape, seed + 2, True), messy_field(shape, seed)
    fixed = messy_volume(shape, seed + 1, False)
    rng = np.random.default_rng(seed)
    moving = (500.0 - 0.6 * fixed + rng.normal(0, 30, shape)).astype(np.float32)
    return fixed, moving, smooth_field(shape, seed)


@pytest.mark.parametrize("radius", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_lcc_force_and_update_are_bit_equal_to_the_specification(shape, radius):
    for offset, kind in enumerate(("messy", "smooth", "messy", "smooth")):          # base pointers 0..3 floats past 16 bytes
        fixed, moving, u = pair(shape, kind)
        args = (on_device(fixed, offset), on_device(moving, (offset + 1) % 4), on_device(u, (offset + 2) % 4))
        want, (s_want, n_want) = D.lcc_force_np(fixed, moving, u, radius, max_step=0.4)
        got, s, n = D.lcc_force(*args, radius=radius, max_step=0.4)
        assert same_bits(got.cpu().numpy(), want), (kind, offset)
        assert int(n) == n_want and abs(float(s) - s_want) <= np.spacing(s_want), (kind, float(s), s_want)
        for scale in (1.0, 0.25):
            want_w, row = D.lcc_update_np(fixed, moving, u, radius, max_step=0.4, scale=scale)
            out = on_device(np.zeros_like(u), (offset + 3) % 4)
            w, sw, nw = D.lcc_update(*args, radius=radius, max_step=0.4, scale=scale, out=out)
            assert w is out and same_bits(w.cpu().numpy(), want_w), (kind, offset, scale)
            assert row == (s_want, n_want) and same_double(sw, s) and int(nw) == int(n)
        for t, a in zip(args, (fixed, moving, u)):
            assert same_bits(t.cpu().numpy(), a)                                    # the inputs are only read
    if min(shape) > 1:
        assert n_want > 0


def test_two_runs_give_the_same_bits():
    shape = (17, 18, 33)
    fixed, moving, u = pair(shape, "messy")
    args = (on_device(fixed), on_device(moving), on_device(u))
    a, sa, na = D.lcc_force(*args, radius=2)
    b, sb, nb = D.lcc_force(*args, radius=2)
    assert same_bits(a.cpu().numpy(), b.cpu().numpy()) and same_double(sa, sb) and int(na) == int(nb) and int(na) > 0


def test_the_neighbours_of_the_output_are_left_alone():
    shape = (9, 10, 67)
    fixed, moving, u = pair(shape, "smooth")
    n = 3 * int(np.prod(shape))
    for update in (False, True):
        buf = torch.full((n + 64,), -7.25, dtype=torch.float32, device="cuda")
        out = buf[32:32 + n].view(3, *shape)
        fn = D.lcc_update if update else D.lcc_force
        got, _, _ = fn(on_device(fixed), on_device(moving), on_device(u), radius=3, out=out)
        host = buf.cpu().numpy()
        assert (host[:32] == -7.25).all() and (host[32 + n:] == -7.25).all()
        want = (D.lcc_update_np if update else D.lcc_force_np)(fixed, moving, u, 3)[0]
        assert same_bits(host[32:32 + n].reshape(want.shape), want)


def test_bad_arguments_are_refused_on_the_device_too():
    shape = (4, 5, 6)
    fixed, moving, u = (on_device(a) for a in pair(shape, "smooth"))
    for radius in (0, 5, 2.5):
        with pytest.raises(ValueError, match="lcc_radius"):
            D.lcc_force(fixed, moving, u, radius=radius)
    with pytest.raises(ValueError, match="out must be another"):
        D.lcc_force(fixed, moving, u, out=u)
    with pytest.raises(ValueError):
        D.lcc_force(fixed, moving[:3].contiguous(), u)
    with pytest.raises(ValueError):
        D.lcc_update(fixed.double(), moving, u)


# ---------------------------------------------------------------- the whole registration

def scans():
    return tuple(torch.from_numpy(v.copy()).cuda() for v in lccutil.contrast_phantom()[:2])


def same_result(got, want):
    assert same_bits(got.field.cpu().numpy(), want.field)
    assert same_bits(got.warped.cpu().numpy(), want.warped)
    assert [n for _, n in got.stats] == [n for _, n in want.stats]
    for (s, _), (s_want, _) in zip(got.stats, want.stats):
        assert abs(s - s_want) <= np.spacing(s_want)
    assert got.jacobian == want.jacobian and got.schedule == want.schedule


@pytest.mark.parametrize("kind", ["deformable", "diffeomorphic"])
def test_the_registration_is_bit_equal_to_the_specification_eager_and_captured(kind):
    fixed, moving = scans()
    fn, ws_type = (D.register_deformable, D.DeformWorkspace) if kind == "deformable" else (D.register_diffeomorphic, D.DiffeoWorkspace)
    want = lccutil.reference(kind, "lcc")
    ws = ws_type(fixed.shape, fixed.device, force="lcc", lcc_radius=2, **lccutil.SCHEDULE)
    eager = fn(fixed, moving, force="lcc", lcc_radius=2, workspace=ws, **lccutil.SCHEDULE)
    same_result(eager, want)
    captured = fn(fixed, moving, force="lcc", lcc_radius=2, workspace=ws, graph=True, **lccutil.SCHEDULE)
    assert same_bits(captured.field.cpu().numpy(), eager.field.cpu().numpy())
    assert same_bits(captured.warped.cpu().numpy(), eager.warped.cpu().numpy())
    assert captured.stats == eager.stats and captured.jacobian == eager.jacobian
    # a workspace made for the other force, or another radius, is refused - both ways
    for other in (ws_type(fixed.shape, fixed.device, **lccutil.SCHEDULE),
                  ws_type(fixed.shape, fixed.device, force="lcc", lcc_radius=3, **lccutil.SCHEDULE)):
        with pytest.raises(ValueError, match="workspace"):
            fn(fixed, moving, force="lcc", lcc_radius=2, workspace=other, **lccutil.SCHEDULE)
    with pytest.raises(ValueError, match="workspace"):
        fn(fixed, moving, workspace=ws, **lccutil.SCHEDULE)
