"""CPU-only tests of the force across contrasts (mri_superresolution_amd/volume_deform.py, numpy part): the specification against an
independent restatement, what an affine contrast change does to it (nothing), the argument checks, the unchanged default and the
quality on the phantom seen in another contrast."""
import numpy as np
import pytest
import torch

import deformutil as du
import lccutil
from mri_superresolution_amd import volume_deform as D


def smooth_volume(shape):
    """A noise-free smooth volume with a gradient everywhere."""
    x, y, z = np.meshgrid(*(np.linspace(0.0, 1.0, n) for n in shape), indexing="ij")
    return (400.0 + 250.0 * np.sin(2.2 * x + 0.3) * np.cos(1.7 * y) + 180.0 * z * z + 90.0 * x * y).astype(np.float32)


@pytest.mark.parametrize("radius", [1, 2])
def test_the_specification_equals_an_independent_restatement(radius):
    shape = (5, 4, 7)
    for specials, field in ((False, du.smooth_field(shape, 3)), (True, du.messy_field(shape, 4))):
        fixed, moving = du.messy_volume(shape, 11, specials), du.messy_volume(shape, 12, specials)
        want, (s_want, n_want) = lccutil.slow_lcc_force(fixed, moving, field, radius, max_step=0.4)
        got, (s, n) = D.lcc_force_np(fixed, moving, field, radius, max_step=0.4)
        assert du.same_bits(got, want)
        assert n == n_want and s == s_want
        assert n > 0 and not du.same_bits(got, field + np.float32(0))          # the force did something
        upd, row = D.lcc_update_np(fixed, moving, field, radius, max_step=0.4, scale=0.25)
        assert row == (s, n) and not np.isnan(upd).any()                        # an update is never NaN, whatever the field holds
        with np.errstate(all="ignore"):
            clean = np.where(np.isfinite(field), field, 0).astype(np.float32)
        # on a finite field the additive form is u + upd / scale (0.25 is a power of two: exact)
        got_clean = D.lcc_force_np(fixed, moving, clean, radius, max_step=0.4)[0]
        upd_clean = D.lcc_update_np(fixed, moving, clean, radius, max_step=0.4, scale=0.25)[0]
        assert du.same_bits(got_clean, clean + upd_clean * np.float32(4))


@pytest.mark.parametrize("b", [-0.7, 1.3])
def test_an_affine_contrast_change_produces_no_force(b):
    fixed = smooth_volume((12, 10, 14))
    moving = (150.0 + b * fixed.astype(np.float64)).astype(np.float32)
    zero = np.zeros((3,) + fixed.shape, dtype=np.float32)
    upd, (s, n) = D.lcc_update_np(fixed, moving, zero, radius=2)
    assert n == fixed.size
    assert np.abs(upd).max() <= 1e-3
    assert s / n >= 0.999
    # the intensity difference does see a force in the same pair: ten times that bound and more
    assert np.abs(D.demons_update_np(fixed, moving, zero)[0]).max() > 1e-2


def test_bad_inputs_raise():
    shape = (4, 5, 6)
    f, m = du.messy_volume(shape, 1, False), du.messy_volume(shape, 2, False)
    u = np.zeros((3,) + shape, dtype=np.float32)
    for radius in (0, 5, 2.5, True):
        with pytest.raises(ValueError, match="lcc_radius"):
            D.lcc_force_np(f, m, u, radius)
        with pytest.raises(ValueError, match="lcc_radius"):
            D.lcc_update_np(f, m, u, radius)
        with pytest.raises(ValueError, match="lcc_radius"):
            D.register_deformable_np(f, m, levels=1, iterations=1, force="lcc", lcc_radius=radius)
    with pytest.raises(ValueError):
        D.lcc_force_np(f.astype(np.float64), m, u)
    with pytest.raises(ValueError, match="share a grid"):
        D.lcc_force_np(f, m[:3], u)
    with pytest.raises(ValueError):
        D.lcc_force_np(f, m, u[:2])
    with pytest.raises(ValueError, match="Unknown force"):
        D.register_deformable_np(f, m, levels=1, iterations=1, force="mi")
    with pytest.raises(ValueError, match="Unknown force"):
        D.register_diffeomorphic_np(f, m, levels=1, iterations=1, force="mi")
    with pytest.raises(ValueError, match="scale"):
        D.lcc_update_np(f, m, u, scale=0.0)
    cpu = [torch.from_numpy(a) for a in (f, m, u)]
    for fn in (D.lcc_force, D.lcc_update):
        with pytest.raises(ValueError):
            fn(*cpu)
    for fn in (D.register_deformable, D.register_diffeomorphic):
        with pytest.raises(ValueError):
            fn(cpu[0], cpu[1], levels=1, iterations=1, force="lcc")


def test_the_default_force_computes_what_it_did():
    shape = (16, 12, 20)
    f, m = du.messy_volume(shape, 5, False), du.messy_volume(shape, 6, False)
    for fn in (D.register_deformable_np, D.register_diffeomorphic_np):
        a = fn(f, m, levels=1, iterations=3)
        b = fn(f, m, levels=1, iterations=3, force="ssd")
        c = fn(f, m, levels=1, iterations=3, force="ssd", lcc_radius=4)
        for r in (b, c):
            assert du.same_bits(r.field, a.field) and du.same_bits(r.warped, a.warped)
            assert r.stats == a.stats and r.jacobian == a.jacobian
    # and the row of the default force is still the sum of squared differences of demons_force_np
    u = np.zeros((3,) + shape, dtype=np.float32)
    assert a.stats[0][1] == D.demons_update_np(f, m, u)[1][1]


@pytest.mark.parametrize("noise", [0.0, 10.0])
def test_the_force_improves_another_contrast_where_the_difference_worsens_it(noise):
    """End-point error over the RMS of the true field inside the object, two levels, 15 + 10 iterations, sigma 1.5, r = 2: the
    specification gives 0.833 with the correlation force (minimum determinant 0.721) and 1.826 with the intensity difference at
    noise 0; 0.831 (0.734) and 1.826 at noise 10.  The thresholds are the boundary between improving and worsening the field."""
    fixed, moving, truth, mask = lccutil.contrast_phantom(noise)
    lcc = du.quality(fixed, moving, truth, mask, lccutil.reference("deformable", "lcc", noise))
    ssd = du.quality(fixed, moving, truth, mask, lccutil.reference("deformable", "ssd", noise))
    print(f"noise {noise}: lcc end-point ratio {lcc[1]:.4f}, min det {lcc[2]:.4f}; ssd end-point ratio {ssd[1]:.4f}")
    assert lcc[1] < 1.0
    assert ssd[1] > 1.0
    assert lcc[2] > 0.0
    rows = lccutil.reference("deformable", "lcc", noise).stats
    assert len(rows) == 25 and all(0 < s <= n for s, n in rows)             # (sum of confidences, count): a mean in (0, 1]
