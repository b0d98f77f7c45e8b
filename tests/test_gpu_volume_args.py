"""The shared argument checks of the volume tools (``_volume_args``) on CUDA tensors: what the device entry points refuse - with the
``what`` prefix, before anything is launched - and what they go on accepting: ``volume_eval``'s lenient entries take a volume
that is not contiguous and a bool mask (they copy), the strict entries take a bool mask as a uint8 view (no copy).  Volumes of
(5, 6, 7): the smallest shape that keeps the three axes distinct.
"""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

pytestmark = pytest.mark.gpu

from mri_superresolution_amd import _lib as L              # noqa: E402
import mri_superresolution_amd.volume_bias as B            # noqa: E402
import mri_superresolution_amd.volume_deform as D          # noqa: E402
import mri_superresolution_amd.volume_denoise as N         # noqa: E402
import mri_superresolution_amd.volume_eval as V            # noqa: E402
import mri_superresolution_amd.volume_intensity as I       # noqa: E402
import mri_superresolution_amd.volume_register as G        # noqa: E402
import mri_superresolution_amd.volume_reslice as R         # noqa: E402
import mri_superresolution_amd.volume_sharpness as E       # noqa: E402
import mri_superresolution_amd.volume_stacks as K          # noqa: E402
import mri_superresolution_amd.volume_surface as S         # noqa: E402
import mri_superresolution_amd.volume_tissue as T          # noqa: E402

SHAPE = (5, 6, 7)
EYE = np.eye(4)[:3]
GEO = K.StackGeometry(EYE, EYE, 2, np.zeros(1), np.ones(1, dtype=np.float32))
RANGE = (0.0, 100.0)


@pytest.fixture(scope="module")
def vol():
    rng = np.random.default_rng(11)
    return torch.from_numpy((rng.random(SHAPE) * 100).astype(np.float32)).cuda()


@pytest.fixture(scope="module")
def mask():
    rng = np.random.default_rng(12)
    return torch.from_numpy((rng.random(SHAPE) < 0.6).astype(np.uint8)).cuda()


@pytest.fixture(scope="module")
def labels():
    rng = np.random.default_rng(13)
    return torch.from_numpy(rng.integers(0, 4, SHAPE).astype(np.uint8)).cuda()


@pytest.fixture
def no_launch(monkeypatch):
    def refuse(name, *args, **kwargs):
        raise AssertionError(f"{name} was launched after a bad argument")
    monkeypatch.setattr(L, "call", refuse)


# Every device entry point whose volume check moved, as (what, call of one volume): the other arguments are good ones.
def volume_entries(vol, mask, labels):
    field = torch.zeros((3,) + SHAPE, dtype=torch.float32, device="cuda")
    sdist = torch.zeros((2,) + SHAPE, dtype=torch.float32, device="cuda")
    return [
        ("reslice", lambda v: R.reslice(v, EYE, SHAPE)),
        ("masked_percentiles", lambda v: I.masked_percentiles(v, mask)),
        ("piecewise_map", lambda v: I.piecewise_map(v, vol[0, 0, :3].contiguous(), vol[0, 0, :3].contiguous())),
        ("match_intensity", lambda v: I.match_intensity(v, vol)),
        ("smooth_masked", lambda v: B.smooth_masked(v, mask, (1, 1, 1))),
        ("match_bias", lambda v: B.match_bias(v, vol, mask, mask, (1, 1, 1))),
        ("correct_bias", lambda v: B.correct_bias(v, mask, (1, 1, 1))),
        ("denoise", lambda v: N.denoise(v, N.noise_params(5.0))),
        ("estimate_noise", lambda v: N.estimate_noise(v, mask)),
        ("background_mask", lambda v: N.background_mask(v)),
        ("denoise_volume", lambda v: N.denoise_volume(v)),
        ("warp", lambda v: D.warp(v, field)),
        ("demons_force", lambda v: D.demons_force(v, vol, field)),
        ("demons_update", lambda v: D.demons_update(vol, v, field)),
        ("lcc_force", lambda v: D.lcc_force(v, vol, field)),
        ("warp_matrix", lambda v: D.warp_matrix(v, EYE, field)),
        ("register_deformable", lambda v: D.register_deformable(v, vol)),
        ("register_diffeomorphic", lambda v: D.register_diffeomorphic(vol, v)),
        ("stack_residual", lambda v: K.stack_residual(v, vol, GEO)),
        ("stack_update", lambda v: K.stack_update(v, [vol], [GEO])),
        ("combine_stacks: stack 0", lambda v: K.combine_stacks([v], [GEO], SHAPE)),
        ("joint_histogram", lambda v: G.joint_histogram(v, vol, EYE, 32, 1, RANGE, RANGE)),
        ("register_rigid", lambda v: G.register_rigid(v, np.eye(4), vol, np.eye(4))),
        ("segment_tissue", lambda v: T.segment_tissue(v, mask)),
        ("edge_profile", lambda v: E.edge_profile(v, sdist)),
    ]


# ... and of one uint8 label volume or mask.
def label_entries(labels):
    return [
        ("reslice_mask", lambda t: R.reslice_mask(t, EYE, SHAPE)),
        ("mask_moments", lambda t: G.mask_moments(t)),
        ("label_confusion", lambda t: T.label_confusion(t, labels)),
        ("label_boundary", lambda t: S.label_boundary(t)),
        ("distance_transform_sq", lambda t: S.distance_transform_sq(t, 1)),
        ("surface_distances", lambda t: S.surface_distances(t, labels)),
        ("interface_sides", lambda t: E.interface_sides(t, 1)),
        ("signed_distance", lambda t: E.signed_distance(t, 1)),
        ("signed_distances", lambda t: E.signed_distances(t)),
    ]


def test_bad_volumes_are_refused(vol, mask, labels, no_launch):
    entries = volume_entries(vol, mask, labels)
    bad = {"transposed": vol.permute(0, 2, 1).contiguous().permute(0, 2, 1),       # the shape of vol, not contiguous
           "float64": vol.double(),
           "empty": vol[:0]}
    assert bad["transposed"].shape == vol.shape and not bad["transposed"].is_contiguous()
    for what, call in entries:
        for kind, v in bad.items():
            with pytest.raises(ValueError, match="^" + what):
                call(v)


def test_bad_labels_are_refused(labels, no_launch):
    bad = {"transposed": labels.permute(0, 2, 1).contiguous().permute(0, 2, 1),
           "float64": labels.double(),
           "empty": labels[:0]}
    for what, call in label_entries(labels):
        for kind, t in bad.items():
            with pytest.raises(ValueError, match="^" + what):
                call(t)


def test_masks_of_the_wrong_shape_are_refused(vol, mask, labels, no_launch):
    wrong = torch.ones((5, 6, 8), dtype=torch.uint8, device="cuda")
    for what, call in [
            ("masked_percentiles", lambda m: I.masked_percentiles(vol, m)),
            ("masked_percentiles", lambda m: I.match_intensity(vol, vol, source_mask=m)),      # the entry that checks it
            ("smooth_masked", lambda m: B.smooth_masked(vol, m, (1, 1, 1))),
            ("match_bias", lambda m: B.match_bias(vol, vol, mask, m, (1, 1, 1))),
            ("correct_bias", lambda m: B.correct_bias(vol, m, (1, 1, 1))),
            ("estimate_noise", lambda m: N.estimate_noise(vol, m)),
            ("joint_histogram", lambda m: G.joint_histogram(vol, vol, EYE, 32, 1, RANGE, RANGE, fixed_mask=m)),
            ("segment_tissue", lambda m: T.segment_tissue(vol, m)),
            ("label_confusion", lambda m: T.label_confusion(labels, labels, m)),
            ("surface_distances", lambda m: S.surface_distances(labels, m)),
            ("volume_metrics", lambda m: V.volume_metrics(vol, vol, 100.0, 3, mask=m))]:
        with pytest.raises(ValueError, match="^" + what):
            call(wrong)
        with pytest.raises(ValueError, match="^" + what):
            call(mask.to(torch.int32))


def test_register_rigid_refuses_bad_masks(vol, mask):
    """``register_rigid`` reads the ranges of its volumes before it looks at the masks, as it always has: no ``no_launch`` here."""
    wrong = torch.ones((5, 6, 8), dtype=torch.uint8, device="cuda")
    for bad in (wrong, mask.to(torch.int32), mask.bool(), mask.permute(0, 2, 1).contiguous().permute(0, 2, 1)):
        with pytest.raises(ValueError, match="^register_rigid: the mask must be"):
            G.register_rigid(vol, np.eye(4), vol, np.eye(4), fixed_mask=bad)
        with pytest.raises(ValueError, match="^register_rigid: the mask must be"):
            G.register_rigid(vol, np.eye(4), vol, np.eye(4), init="global", fixed_mask=mask, moving_mask=bad)


def test_bad_out_of_the_other_entries_is_refused(vol, labels, no_launch):
    """The entries whose ``out`` goes through ``cuda_tensor``: another shape, not contiguous, another dtype."""
    lm = vol[0, 0, :3].contiguous()
    for what, call, dtype in [
            ("(piecewise_map|out must have the shape)", lambda out: I.piecewise_map(vol, lm, lm, out=out), torch.float32),
            ("signed_distance: out must be", lambda out: E.signed_distance(labels, 1, out=out), torch.float32),
            (r"interface_sides \(out\)", lambda out: E.interface_sides(labels, 1, out=out), torch.uint8),
            (r"label_boundary \(out\)", lambda out: S.label_boundary(labels, out=out), torch.uint8)]:
        other = torch.float64 if dtype == torch.float32 else torch.int32
        for out in (torch.empty((5, 6, 8), dtype=dtype, device="cuda"),
                    torch.empty((5, 7, 6), dtype=dtype, device="cuda").transpose(1, 2),
                    torch.empty(SHAPE, dtype=other, device="cuda")):
            with pytest.raises(ValueError, match="^" + what):
                call(out)


def test_bad_out_is_refused(vol, no_launch):
    field = torch.zeros((3,) + SHAPE, dtype=torch.float32, device="cuda")
    for what, call, alias, like in [
            ("warp", lambda out: D.warp(vol, field, out=out), vol, vol),
            ("demons_force", lambda out: D.demons_force(vol, vol, field, out=out), field, field),
            ("smooth_field", lambda out: D.smooth_field(field, (1, 1, 1), out=out), field, field),
            ("compose", lambda out: D.compose(field, field, out=out), field, field),
            ("demons_update", lambda out: D.demons_update(vol, vol, field, out=out), field, field),
            ("exp_field", lambda out: D.exp_field(field, 2, out=out), field, field),
            ("warp_matrix", lambda out: D.warp_matrix(vol, EYE, field, out=out), vol, vol),
            ("stack_residual", lambda out: K.stack_residual(vol, vol, GEO, out=out), vol, vol),
            ("stack_update", lambda out: K.stack_update(vol, [vol], [GEO], out=out), None, vol),
            ("denoise", lambda out: N.denoise(vol, N.noise_params(5.0), out=out), vol, vol)]:
        bad = [torch.empty(like.shape[:-1] + (like.shape[-1] + 1,), dtype=torch.float32, device="cuda"),        # another shape
               torch.empty(like.shape[:-2] + like.shape[:-3:-1], dtype=torch.float32, device="cuda").transpose(-1, -2)]
        assert bad[1].shape == like.shape and not bad[1].is_contiguous()
        if alias is not None:
            bad.append(alias)
        for out in bad:
            with pytest.raises(ValueError, match="^" + what + ": out must be another"):
                call(out)


def same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if not isinstance(a, torch.Tensor):
        return a == b
    return a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))      # bit for bit, NaN too


def test_volume_eval_stays_lenient(vol, mask):
    """``volume_eval``'s entries copy what they need: a volume that is not contiguous and a bool mask give the bits of the
    contiguous float32 / uint8 form."""
    even = vol[:4, :6, :6].contiguous()
    view = even.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert not view.is_contiguous()
    assert same(V.downsample2(view), V.downsample2(even))
    assert same(V.upscale2(view, "cubic"), V.upscale2(even, "cubic"))
    assert same(V.otsu_mask(view), V.otsu_mask(even))
    assert same(V.foreground_mask(view, 1), V.foreground_mask(even, 1))
    assert same(V.volume_metrics(view, even * 0.5, 100.0, 3), V.volume_metrics(even, even * 0.5, 100.0, 3))
    flipped = mask.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    for m in (mask.bool(), flipped, flipped.bool()):
        assert same(V.binary_dilate(m, 1), V.binary_dilate(mask, 1))
        assert same(V.binary_erode(m, 1), V.binary_erode(mask, 1))
        assert same(V.binary_close(m, 1), V.binary_close(mask, 1))
        assert same(V.label_components(m), V.label_components(mask))
        assert same(V.largest_component(m), V.largest_component(mask))
        assert same(V.fill_holes(m), V.fill_holes(mask))
        assert same(V.volume_metrics(vol, vol * 0.5, 100.0, 3, mask=m), V.volume_metrics(vol, vol * 0.5, 100.0, 3, mask=mask))


def test_bool_masks_are_taken_as_views(vol, mask, labels):
    """The strict entries read a bool mask through ``.view(torch.uint8)``: the bits of the uint8 mask's result."""
    b = mask.bool()
    assert same(I.masked_percentiles(vol, b), I.masked_percentiles(vol, mask))
    assert same(B.smooth_masked(vol, b, (1, 1, 1)), B.smooth_masked(vol, mask, (1, 1, 1)))
    assert same(B.correct_bias(vol, b, (1, 1, 1)), B.correct_bias(vol, mask, (1, 1, 1)))
    assert same(N.estimate_noise(vol, b), N.estimate_noise(vol, mask))
    assert same(R.reslice_mask(b, EYE, SHAPE), R.reslice_mask(mask, EYE, SHAPE))
    assert same(T.segment_tissue(vol, b).labels, T.segment_tissue(vol, mask).labels)
    assert np.array_equal(T.label_confusion(labels, labels, b), T.label_confusion(labels, labels, mask))
