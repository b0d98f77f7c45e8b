"""Low-field simulation (csrc/lowfield.hip) at every pass-1 launch shape: the shapes, seeded inputs, float32 emulation, tie band and
impulse expectation of test_lowfield_ref_host.py (which proves on the CPU that the bars can be met by correct arithmetic) and
test_gpu_lowfield_shapes.py.  Host code only: nothing here touches the GPU; the library is loaded for its table helpers.

Bars
  F32_BAR     5e-5 absolute, the project's float32 bar (tests/test_gpu_lowfield.py), for the magnitude plane and the output plane
              against the float64 restatements of utils/lowfield.py.
  tie band    the uint8 image is the truncation of lr * 255, discontinuous at the integers: a pixel may differ from the host's
              (by one grey level) only where the host's v = lr * 255 lies within 255 * F32_BAR of an integer, and that band may
              hold at most TIE_SHARE of an image's pixels - a condition the seeds are chosen to meet (seed_of), asserted on the
              host reference alone in test_lowfield_ref_host.py.
  impulse     one pixel of 255 (uint8) or 1.0 (float) at (m0, n0), no noise:
                  magnitude[r][c] = |p_r[(r - m0) mod H]| |p_c[(c - n0) mod W]|,
              p the float32 tables the kernel reads, taken to float64.  Every sum of pass 1 then has ONE non-zero term, so the
              error is the rounding of that term alone, u = 2^-24, first order:
                  U = fl(fl(255 p) fl(1 / 255))             3 u of each component, so |dU| <= 3 u |U|       (float input: 0)
                  Y = U q, a component is fma(a, b, fl(c d))  2 u (|ab| + |cd|) <= 2 u |U| |q| per component (Cauchy-Schwarz:
                                                            relative to |Y|, not to the component, which may cancel), so
                                                            |dY| <= 2 sqrt(2) u |Y| < 3 u |Y|
                  m = sqrt(fma(re, re, fl(im im)))          2 u of the sum, halved by the root, and the root's own: 2 u
              about 8 u in all; IMPULSE_ULPS = 16 covers the second-order terms and an emulation that rounds every product
              (numpy: 3 u per component of Y, 3 u for the sum of squares - about 10 u).
              CORRECTION of the floor.  The issue's 1e-30 is wrong and test_lowfield_ref_host.py shows it: the tables hold
              rounding residue of the double sums (1e-19 where the exact entry is 0), so |Y| reaches 1e-20 .. 1e-24, its squares
              are float32 subnormals (quantum 2^-149) and the relative bound above no longer holds.  With s = re^2 + im^2 off by
              at most d = 3 * 2^-150 (two squares and the sum, half a quantum each), |sqrt(s + d) - sqrt(s)| <= sqrt(d) < 2^-74.
              The floor is therefore IMPULSE_FLOOR = 2^-74 (5.3e-23): derived from the format, below every entry that is not
              residue (the smallest genuine |p_r| |p_c| of these shapes is above 1e-8, the largest residue below 1e-16).
"""
from __future__ import annotations

import functools
import math

import numpy as np

from mri_superresolution_amd.utils import lowfield as LF

F32_BAR = 5e-5
TIE_SHARE = 0.05
IMPULSE_ULPS = 16
IMPULSE_FLOOR = 2.0 ** -74
NOISE_STD = (5.0, 2.0, 9.0)                 # per batch entry, as tests/test_gpu_lowfield.py
BATCH = 3
KINDS = ("uniform", "binary", "ramp")
LDS_LIMIT = 160 * 1024

# (H, W) of the uint8 pipeline (even, >= 4) and of the float pipeline (any size >= 2); what each reaches is listed next to the
# dispatch table in test_gpu_lowfield_shapes.py
U8_SHAPES = ((4, 130), (6, 256), (24, 258), (10, 512), (8, 514), (8, 1026), (12, 2050), (8, 2272))
F32_SHAPES = ((2, 129), (3, 257), (7, 513), (9, 1025), (5, 2049), (5, 129), (4, 257))
EXTREMA_EXTRA = (8, 128)                    # the <1,128> instantiation, for the extrema placement only
WIDE_SEEDED = ((8, 514), (8, 1026))


def threads(w):
    """kLT of lowfield_pass1's dispatch for an image of width w."""
    return 128 if w <= 256 else 256


def columns(w):
    """kK of lowfield_pass1's dispatch."""
    return 1 if w <= 128 else 2 if w <= 512 else 4


def half_width(n, f):
    return int(n * f) // 2


def crops(h, w):
    """Crop factors of a shape: 0.5, and 0.3 where it keeps a frequency on both axes.  int(n 0.5) // 2 is 0 for n = 2 and n = 3 -
    the library refuses those (the reference's mask would be empty) - so the two shortest float shapes run at the smallest of
    0.75 and 1.0 that keeps one instead."""
    first = next(f for f in (0.5, 0.75, 1.0) if half_width(h, f) >= 1 and half_width(w, f) >= 1)
    return (first, 0.3) if half_width(h, 0.3) >= 1 and half_width(w, 0.3) >= 1 else (first,)


def lds_bytes(h, w):
    """lowfield_lds_bytes of csrc/lowfield.hip: two float2 tables (H + 16 and W entries, rounded up to even) and U [W][16] float."""
    return ((h + 16 + w + 1) & ~1) * 8 + w * 16 * 4


def widest(h, even):
    """The widest image of height h the size rule accepts (the uint8 entry takes even widths only)."""
    return max(w for w in range(4, 4096) if lds_bytes(h, w) <= LDS_LIMIT and not (even and w & 1))


def cases(shapes):
    return [(h, w, f) for h, w in shapes for f in crops(h, w)]


def case_id(c):
    return f"{c[0]}x{c[1]}-f{c[2]}"


# ------------------------------------------------------------------------------------------------ seeded inputs
# seeds whose host reference puts more than TIE_SHARE of an image's pixels into the tie band are moved on (the LR image of
# (4, 130) has 130 pixels: 7 in the band are too many); test_lowfield_ref_host.py asserts the condition for every case
SEED_BUMP = {("u8", "ramp", 4, 130, 0.5): 1}


def seed_of(pipe, kind, h, w, f):
    key = (pipe, kind, h, w, f)
    return [("u8", "f32").index(pipe), ("uniform", "binary", "ramp", "extrema").index(kind), h, w, int(f * 100), SEED_BUMP.get(key, 0)]


def _ramp(h, w, k):
    yy, xx = np.mgrid[0:h, 0:w]
    return (yy * (k + 1) + xx * 3) / float((h - 1) * (k + 1) + (w - 1) * 3)


def image(rng, pipe, kind, h, w, k):
    """One (H,W) image: uint8 as tests/test_gpu_lowfield.py makes it, or float32 in [0,1] (batch entry 1 keeps its extrema away
    from 0 and 1, as the extraction's slices do not)."""
    if kind == "uniform":
        v = rng.integers(0, 256, (h, w)) if pipe == "u8" else rng.random((h, w))
    elif kind == "binary":
        v = rng.integers(0, 2, (h, w)) * (255 if pipe == "u8" else 1)
    else:
        v = _ramp(h, w, k) * (255.0 if pipe == "u8" else 1.0)
    if pipe == "u8":
        return v.astype(np.uint8)
    v = v.astype(np.float32)
    return np.float32(0.2) + np.float32(0.5) * v if k == 1 else v


def kspace_noise(rng, h, w, noise_std):
    s = (noise_std / 255.0) * math.sqrt(h * w) / 10            # preprocessing.py:274
    return rng.normal(0, s, (h, w)), rng.normal(0, s, (h, w))


def batch(pipe, kind, h, w, f):
    """(images [3][H][W], k-space noise [(re, im)] * 3): a different image and different noise per batch entry."""
    rng = np.random.default_rng(seed_of(pipe, kind, h, w, f))
    if kind == "extrema":
        images = [extrema_image(rng, pipe, h, w, k) for k in range(BATCH)]
    else:
        images = [image(rng, pipe, kind, h, w, k) for k in range(BATCH)]
    return np.stack(images), [kspace_noise(rng, h, w, NOISE_STD[k]) for k in range(BATCH)]


def image_noise_planes(knoise):
    """float32 (re, im) [B][H][W] image-space planes of the k-space draws: what the device is handed."""
    n = np.stack([LF.image_noise_from_kspace(a, b) for a, b in knoise])
    return np.ascontiguousarray(n.real, dtype=np.float32), np.ascontiguousarray(n.imag, dtype=np.float32)


def extrema_positions(h, w):
    """((row, col) of the single minimum, of the single maximum): the last pixel (ragged last column group, last row block) and
    the first pixel of a lane's second column - for one column per thread, that lane-127 pixel (0, 127)."""
    return (h - 1, w - 1), (0, threads(w) if columns(w) > 1 else 127)


EXTREMA_U8 = ((7, 251), (0, 255), (19, 233))             # (minimum, maximum) per batch entry; background in [40, 200]
EXTREMA_F32 = ((0.03, 0.97), (0.0, 1.0), (0.11, 0.9))    # background in [0.2, 0.8]


def extrema_image(rng, pipe, h, w, k):
    lo, hi = extrema_positions(h, w)
    if pipe == "u8":
        x = rng.integers(40, 201, (h, w)).astype(np.uint8)
        x[lo], x[hi] = EXTREMA_U8[k]
    else:
        x = (0.2 + 0.6 * rng.random((h, w))).astype(np.float32)
        x[lo], x[hi] = EXTREMA_F32[k]
    return x


def impulse_positions(h, w):
    return ((0, 0), (h - 1, w - 1), (h // 2, threads(w)), (1, w - 2))


def impulse_images(pipe, h, w):
    """[4][H][W]: all zero except one pixel of 255 / 1.0, one position of impulse_positions per batch entry."""
    x = np.zeros((4, h, w), dtype=np.uint8 if pipe == "u8" else np.float32)
    for k, (m0, n0) in enumerate(impulse_positions(h, w)):
        x[k, m0, n0] = 255 if pipe == "u8" else 1.0
    return x


# ------------------------------------------------------------------------------------------------ references
@functools.lru_cache(maxsize=None)
def table(pipe, n, f):
    """complex64 Dirichlet row of an axis, the float32 values the kernel reads."""
    re, im = (LF.dirichlet_table if pipe == "u8" else LF.dirichlet_table_any)(n, f)
    return (re + 1j * im).astype(np.complex64)


def impulse_expectation(pipe, h, w, f, m0, n0):
    """float64 [H][W]: |p_r[(r - m0) mod H]| |p_c[(c - n0) mod W]|."""
    pr, pc = np.abs(table(pipe, h, f).astype(np.complex128)), np.abs(table(pipe, w, f).astype(np.complex128))
    return np.outer(pr[(np.arange(h) - m0) % h], pc[(np.arange(w) - n0) % w])


def impulse_bar(expected):
    return IMPULSE_ULPS * 2.0 ** -24 * expected + IMPULSE_FLOOR


@functools.lru_cache(maxsize=4)
def _circulant(pipe, n, f):
    """(re, im) float32 [n][n]: P[i][j] = p[(i - j) mod n]."""
    p = table(pipe, n, f)
    d = np.arange(n)
    m = p[(d[:, None] - d[None, :]) % n]
    return np.ascontiguousarray(m.real), np.ascontiguousarray(m.imag)


def host_reference(pipe, x, f, kspace_noise=None):
    """The float64 restatement of either pipeline with one key, ``plane``, for the output plane (``lr`` / ``clipped``)."""
    if pipe == "u8":
        ref = LF.simulate_low_field_host(x, f, noise_std=0.0, kspace_noise=kspace_noise)
        ref["plane"] = ref["lr"]
    else:
        ref = LF.simulate_low_field_f32_host(np.asarray(x, dtype=np.float64), f, noise_std=0.0, kspace_noise=kspace_noise)
        ref["plane"] = ref["clipped"]
    return ref


def emulate_f32(pipe, x, f, noise=None):
    """float32 numpy emulation of the kernels' circulant form for one (H,W) image: every value and every operation in float32
    (the sums in numpy's order, not the kernel's), pass 2 operation by operation.  ``noise``: float32 (re, im) image-space
    planes.  Returns ``magnitude``, ``plane`` and, for the uint8 pipeline, ``lr_u8``."""
    f32 = np.float32
    h, w = x.shape
    rr, ri = _circulant(pipe, h, f)
    cr, ci = _circulant(pipe, w, f)
    xv = x.astype(f32)
    ure, uim = rr @ xv, ri @ xv
    if pipe == "u8":
        ure, uim = ure * (f32(1) / f32(255)), uim * (f32(1) / f32(255))
    yre = ure @ cr.T - uim @ ci.T
    yim = ure @ ci.T + uim @ cr.T
    if noise is not None:
        yre, yim = yre + noise[0], yim + noise[1]
    mag = np.sqrt(yre * yre + yim * yim)
    assert mag.dtype == f32
    mn, mx = mag.min(), mag.max()
    omin, omax = (f32(x.min()) / f32(255), f32(x.max()) / f32(255)) if pipe == "u8" else (x.min(), x.max())
    s = (mag - mn) / (mx - mn) * (omax - omin) + omin if mx > mn else np.full_like(mag, omin)
    s = np.clip(s, f32(0), f32(1))
    if pipe != "u8":
        return {"magnitude": mag, "plane": s}
    q = s.reshape(h // 2, 2, w // 2, 2)
    lr = (((q[:, 0, :, 0] + q[:, 0, :, 1]) + q[:, 1, :, 0]) + q[:, 1, :, 1]) * f32(0.25)
    assert lr.dtype == f32
    return {"magnitude": mag, "plane": lr, "lr_u8": np.clip(lr * f32(255), 0, 255).astype(np.uint8)}


def renormalise64(magnitude, x_min, x_max, pool):
    """float64 pass 2 from a magnitude plane and the input's extrema (uint8 extrema already divided by 255): what the output
    becomes when pass 1 reports other extrema than the image has."""
    s = (magnitude - magnitude.min()) / (magnitude.max() - magnitude.min()) * (x_max - x_min) + x_min
    s = np.clip(s, 0, 1)
    return s.reshape(s.shape[0] // 2, 2, s.shape[1] // 2, 2).mean((1, 3)) if pool else s


# ------------------------------------------------------------------------------------------------ uint8 rules
def tie_band(lr_host):
    """Pixels whose host value lr * 255 lies within 255 * F32_BAR of an integer: where a truncation may land on the other side."""
    v = np.asarray(lr_host, dtype=np.float64) * 255.0
    return np.abs(v - np.rint(v)) <= 255.0 * F32_BAR


def check_u8(got_u8, got_plane, ref):
    """The uint8 rules for one image against the host dict ``ref``; returns (differing pixels, share of the band)."""
    assert np.array_equal(got_u8, np.clip(got_plane * np.float32(255), 0, 255).astype(np.uint8)), "not the truncation of the plane"
    d = np.abs(got_u8.astype(int) - ref["lr_u8"].astype(int))
    band = tie_band(ref["lr"])
    assert d.max() <= 1, f"{int(d.max())} grey levels from the host image"
    assert not (d > 0)[~band].any(), f"{int((d > 0)[~band].sum())} differing pixel(s) outside the tie band"
    assert band.mean() <= TIE_SHARE, f"the tie band excuses {band.mean():.3f} of the image"
    return int((d > 0).sum()), float(band.mean())
