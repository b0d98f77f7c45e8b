"""Pins tests/lowfieldutil.py on the CPU: at every shape, kind and crop factor test_gpu_lowfield_shapes.py runs, a float32 numpy
emulation of the kernels' circulant form stays within F32_BAR / 10 of the float64 restatement, the tie band excuses at most 5 %
of an image's pixels, and the emulation stays inside the derived impulse bar - so the GPU file's bars can be met by correct
arithmetic.  Also the impulse expectation against the float64 FFT form, the extrema images, and the geometry the shape list
relies on (columns per thread, column trips, LDS bytes, the size rule's limit).  The library is loaded for its table helpers; no
GPU."""
import numpy as np
import pytest

import lowfieldutil as LU
from mri_superresolution_amd.utils import lowfield as LF

PIPE_CASES = [("u8", c) for c in LU.cases(LU.U8_SHAPES)] + [("f32", c) for c in LU.cases(LU.F32_SHAPES)]
EXTREMA_CASES = [("u8", c) for c in LU.cases(LU.U8_SHAPES + (LU.EXTREMA_EXTRA,))] + \
                [("f32", c) for c in LU.cases(LU.F32_SHAPES + (LU.EXTREMA_EXTRA,))]
_id = lambda pc: f"{pc[0]}-{LU.case_id(pc[1])}"      # noqa: E731


def _emulation_against_host(pipe, kind, h, w, f):
    images, knoise = LU.batch(pipe, kind, h, w, f)
    n_re, n_im = LU.image_noise_planes(knoise)
    refs = []
    for k in range(LU.BATCH):
        ref = LU.host_reference(pipe, images[k], f, knoise[k])
        emu = LU.emulate_f32(pipe, images[k], f, (n_re[k], n_im[k]))
        merr = np.abs(emu["magnitude"] - ref["magnitude"]).max()
        perr = np.abs(emu["plane"] - ref["plane"]).max()
        assert merr <= LU.F32_BAR / 10 and perr <= LU.F32_BAR / 10, (kind, k, merr, perr)
        if pipe == "u8":
            LU.check_u8(emu["lr_u8"], emu["plane"], ref)          # the band's share among them: the seeds' condition
        refs.append(ref)
    return images, refs


@pytest.mark.parametrize("pc", PIPE_CASES, ids=_id)
def test_emulation_within_a_tenth_of_the_bar_and_tie_band_share(pc):
    pipe, (h, w, f) = pc
    for kind in LU.KINDS:
        _emulation_against_host(pipe, kind, h, w, f)


@pytest.mark.parametrize("pc", EXTREMA_CASES, ids=_id)
def test_extrema_images_and_what_a_lost_extremum_costs(pc):
    pipe, (h, w, f) = pc
    images, refs = _emulation_against_host(pipe, "extrema", h, w, f)
    lo, hi = LU.extrema_positions(h, w)
    assert hi[1] < w and lo != hi
    if LU.columns(w) > 1:
        assert hi[1] == LU.threads(w)              # j = 1 of lane 0
    # the minimum's column group is ragged, except at an instantiation's upper edge
    assert w % (LU.threads(w) * LU.columns(w)) != 0 or (h, w) in ((6, 256), (10, 512), LU.EXTREMA_EXTRA)
    scale = 255.0 if pipe == "u8" else 1.0
    for k in range(LU.BATCH):
        x = images[k].astype(np.float64) / scale
        assert (x == x.min()).sum() == 1 and (x == x.max()).sum() == 1
        assert np.unravel_index(x.argmin(), x.shape) == lo and np.unravel_index(x.argmax(), x.shape) == hi
        rest = np.delete(x.ravel(), [x.argmin(), x.argmax()])
        bg = (40 / 255, 200 / 255) if pipe == "u8" else (0.2, 0.8)
        assert bg[0] - 1e-6 <= rest.min() and rest.max() <= bg[1] + 1e-6
        mag = refs[k]["magnitude"]
        assert np.abs(LU.renormalise64(mag, x.min(), x.max(), pipe == "u8") - refs[k]["plane"]).max() <= 1e-12
        for lost in ((rest.min(), x.max()), (x.min(), rest.max())):          # pass 1 misses the minimum / the maximum
            moved = np.abs(LU.renormalise64(mag, lost[0], lost[1], pipe == "u8") - refs[k]["plane"]).max()
            assert moved > 1e-2, (k, lost, moved)


@pytest.mark.parametrize("pc", PIPE_CASES, ids=_id)
def test_impulse_expectation_and_emulation_inside_the_bar(pc):
    pipe, (h, w, f) = pc
    x = LU.impulse_images(pipe, h, w)
    assert len(set(LU.impulse_positions(h, w))) == (3 if (h, w) == (2, 129) else 4)       # (H - 1, W - 1) is (H / 2, kLT) there
    for k, (m0, n0) in enumerate(LU.impulse_positions(h, w)):
        assert x[k].sum() == x[k, m0, n0] == (255 if pipe == "u8" else 1)
        exp = LU.impulse_expectation(pipe, h, w, f, m0, n0)
        # the expectation is the reference's own answer up to the float32 rounding of the two table entries
        host = LU.host_reference(pipe, x[k], f)["magnitude"]
        assert (np.abs(host - exp) <= 4 * 2.0 ** -24 * exp + 1e-15).all(), (k, np.abs(host - exp).max())
        emu = LU.emulate_f32(pipe, x[k], f)["magnitude"].astype(np.float64)
        ratio = (np.abs(emu - exp) / LU.impulse_bar(exp)).max()
        assert ratio <= 1.0, (k, ratio)


def test_impulse_floor_correction_is_needed():
    """The 1e-30 floor first proposed for the impulse bar does not hold for correct float32 arithmetic: where a table entry is
    rounding residue the squares of |Y| are subnormal.  The emulation exceeds that bar here and stays inside the derived one
    (lowfieldutil's docstring)."""
    h, w, f = 12, 2050, 0.3
    m0, n0 = LU.impulse_positions(h, w)[2]
    exp = LU.impulse_expectation("u8", h, w, f, m0, n0)
    err = np.abs(LU.emulate_f32("u8", LU.impulse_images("u8", h, w)[2], f)["magnitude"].astype(np.float64) - exp)
    assert (err > LU.IMPULSE_ULPS * 2.0 ** -24 * exp + 1e-30).any() and (err <= LU.impulse_bar(exp)).all()
    residue = exp < 1e-12
    assert residue.any() and exp[residue].max() < 1e-16 and exp[~residue].min() > 1e-8 > 1e6 * LU.IMPULSE_FLOOR


def test_shapes_reach_every_instantiation_trip_and_the_lds_limit():
    want = {(4, 130): (2, 128, 1), (6, 256): (2, 128, 1), (24, 258): (2, 256, 1), (10, 512): (2, 256, 1), (8, 514): (4, 256, 1),
            (8, 1026): (4, 256, 2), (12, 2050): (4, 256, 3), (8, 2272): (4, 256, 3),
            (2, 129): (2, 128, 1), (5, 129): (2, 128, 1), (3, 257): (2, 256, 1), (4, 257): (2, 256, 1), (7, 513): (4, 256, 1),
            (9, 1025): (4, 256, 2), (5, 2049): (4, 256, 3)}
    assert set(want) == set(LU.U8_SHAPES) | set(LU.F32_SHAPES)
    for (h, w), (kk, klt, trips) in want.items():
        assert (LU.columns(w), LU.threads(w), -(-w // (kk * klt))) == (kk, klt, trips), (h, w)
        assert (LU.lds_bytes(h, w) > 64 * 1024) == (w >= 1025) and LU.lds_bytes(h, w) <= LU.LDS_LIMIT
    assert LU.columns(LU.EXTREMA_EXTRA[1]) == 1
    assert all(h % 2 == 0 and w % 2 == 0 and h >= 4 for h, w in LU.U8_SHAPES)
    assert {h for h, _ in LU.F32_SHAPES if h < 8} and any(w % 4 for _, w in LU.F32_SHAPES)       # H < 8; noise rows off 16 bytes
    # the size rule: (8, 2272) needs 163 776 of the 163 840 bytes, (7, 2273) all of them
    assert LU.lds_bytes(8, 2272) == 163776 and LU.lds_bytes(8, 2274) == 163920 > LU.LDS_LIMIT
    assert LU.widest(8, even=True) == 2272 and LU.widest(7, even=False) == 2273 and LU.lds_bytes(7, 2273) == LU.LDS_LIMIT
    assert LU.lds_bytes(7, 2274) > LU.LDS_LIMIT


def test_crop_factors():
    """0.5 everywhere it keeps a frequency; the library refuses it at H = 2 and H = 3 (int(n f) // 2 == 0), which run at 1.0 and
    0.75; 0.3 wherever int(n f) // 2 >= 1 on both axes."""
    assert LU.crops(2, 129) == (1.0,) and LU.crops(3, 257) == (0.75,)
    for n in (2, 3):
        with pytest.raises(RuntimeError, match="keeps nothing"):
            LF.dirichlet_table_any(n, 0.5)
    for h, w in LU.U8_SHAPES + LU.F32_SHAPES:
        cs = LU.crops(h, w)
        assert (cs[0] == 0.5) == (h >= 4) and ((0.3 in cs) == (int(h * 0.3) // 2 >= 1 and int(w * 0.3) // 2 >= 1))
        for f in cs:
            assert LU.half_width(h, f) >= 1 and LU.half_width(w, f) >= 1
            LU.table("f32", h, f), LU.table("f32", w, f)          # the library accepts them
    assert sum(0.3 in LU.crops(h, w) for h, w in LU.U8_SHAPES) == 6 and sum(0.3 in LU.crops(h, w) for h, w in LU.F32_SHAPES) == 2
