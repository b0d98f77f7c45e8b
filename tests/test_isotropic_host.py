"""Host side of the isotropic x2 volume: volume.combine_planes_np - the specification the blend kernel
is tested against - pinned to torch's CPU linear interpolation, its edge cases, the NIfTI geometry of three doubled axes and
the --isotropic flag.  No GPU needed."""
import os
import struct
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from mri_superresolution_amd.utils.nifti import read_nifti, write_nifti      # noqa: E402
from mri_superresolution_amd.volume import combine_planes_np                 # noqa: E402


def plane_of(vol, axis):
    """A stand-in for enhance_volume(axis): axis kept, the two others doubled (nearest neighbour: any values will do)."""
    for a in range(3):
        if a != axis:
            vol = np.repeat(vol, 2, axis=a)
    return np.ascontiguousarray(vol, dtype=np.float32)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_single_plane_equals_torch_linear_interpolation(axis):
    """rtol 1e-6 of the largest magnitude: two float32 roundings either side are about 2.4e-7, and torch may fuse the
    multiply-add."""
    rng = np.random.default_rng(axis)
    e = plane_of(rng.uniform(-3000, 3000, (5, 7, 6)), axis)
    got = combine_planes_np({axis: e})
    assert got.dtype == np.float32 and got.shape == (10, 14, 12)
    t = torch.from_numpy(np.moveaxis(e, axis, 2).copy())                      # interpolate the last axis of (N, C, L)
    want = torch.nn.functional.interpolate(t, scale_factor=2, mode="linear", align_corners=False).numpy()
    want = np.moveaxis(want, 2, axis)
    err = np.abs(got - want).max()
    print(f"axis {axis}: max abs difference {err:.3e} at magnitude {np.abs(want).max():.1f}")
    assert err <= 1e-6 * np.abs(want).max()


def test_one_and_two_slices():
    rng = np.random.default_rng(7)
    for axis in (0, 1, 2):
        shape = [4, 6, 8]
        shape[axis] = 1
        e = rng.uniform(-3000, 3000, shape).astype(np.float32)
        u = combine_planes_np({axis: e})
        both = np.moveaxis(u, axis, 0)
        # 0.75 e + 0.25 e: each product and the sum within half an ulp - one rounding of the result at most
        assert both.shape[0] == 2 and np.array_equal(both[0], both[1])
        assert np.abs(both[0] - np.moveaxis(e, axis, 0)[0]).max() <= np.spacing(np.float32(3000))
        shape[axis] = 2
        e = rng.uniform(-3000, 3000, shape).astype(np.float32)
        a, b = np.moveaxis(e, axis, 0)
        f = np.float32
        want = np.stack([f(0.75) * a + f(0.25) * a, f(0.75) * a + f(0.25) * b, f(0.75) * b + f(0.25) * a, f(0.75) * b + f(0.25) * b])
        assert np.array_equal(np.moveaxis(combine_planes_np({axis: e}), axis, 0), want)


def test_mean_of_three_equal_constants_is_the_constant():
    """Exactly, where float32 can: for v of at most 22 significant bits 0.75 v, 0.25 v, their sum, v + v, 3 v and 3 v / 3 are all
    exact (scanner intensities are such values).  Any other v comes back within the roundings of the chain: the sum of two rounded
    products (1 ulp), two additions and the division (half an ulp each, relative to the result) - below 4 ulp."""
    shapes = ((0, (3, 8, 10)), (1, (6, 4, 10)), (2, (6, 8, 5)))
    for value in (1234.0, 0.0, -7.5, 3000.0, 4095.0, 65535.0):
        out = combine_planes_np({a: np.full(s, value, dtype=np.float32) for a, s in shapes})
        assert out.shape == (6, 8, 10) and (out == np.float32(value)).all(), value
    for value in (-0.1, 3.0e-5, 2999.7):
        out = combine_planes_np({a: np.full(s, value, dtype=np.float32) for a, s in shapes})
        assert np.abs(out - np.float32(value)).max() <= 4 * np.spacing(np.float32(abs(value))), value
    two = combine_planes_np({0: np.full((3, 8, 10), 7.0, dtype=np.float32), 2: np.full((6, 8, 5), 9.0, dtype=np.float32)})
    assert (two == 8.0).all()


def test_int16_rounds_half_to_even_and_saturates():
    # a (1, 1, 9) volume whose values change along axis 2 only, planes 0 and 1: both interpolate a constant, 0.75 v + 0.25 v is
    # exact for these values and so is (v + v) / 2 - the float32 mean is v itself, a tie or past the int16 range
    values = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 40000.0, -40000.0, 32767.5, -32768.5], dtype=np.float32)
    doubled = np.repeat(values, 2)
    planes = {0: np.ascontiguousarray(np.broadcast_to(doubled, (1, 2, 18))), 1: np.ascontiguousarray(np.broadcast_to(doubled, (2, 1, 18)))}
    assert (combine_planes_np(planes) == doubled).all()
    out = combine_planes_np(planes, np.int16)
    assert out.dtype == np.int16 and out.shape == (2, 2, 18)
    want = np.repeat(np.array([0, 2, 2, 0, -2, 32767, -32768, 32767, -32768], dtype=np.int16), 2)
    assert (out == want).all()
    with pytest.raises(ValueError):
        combine_planes_np({})
    with pytest.raises(ValueError):
        combine_planes_np({3: planes[0]})
    with pytest.raises(ValueError):
        combine_planes_np({0: planes[0].astype(np.float64)})
    with pytest.raises(ValueError):
        combine_planes_np({0: planes[0], 1: planes[1][:, :, :1]})


# ---- NIfTI geometry of three doubled axes: the headers of tests/test_nifti_host.py, built again here

OBLIQUE = [[1.1, -0.2, 0.3, -90.0], [0.15, 0.9, -0.25, 120.5], [-0.3, 0.2, 2.8, -7.25]]


def pack_header(shape, pixdim, qform_code=0, sform_code=0, quatern=(0.0, 0.0, 0.0), qoffset=(0.0, 0.0, 0.0), srows=None):
    """348 bytes of a little-endian float32 NIfTI-1 header, every field of nifti1.h in its order."""
    dim = [len(shape)] + list(shape) + [1] * (7 - len(shape))
    pix = list(pixdim) + [0.0] * (8 - len(pixdim))
    srows = srows if srows is not None else [[0.0] * 4] * 3
    raw = b"".join([
        struct.pack("<i", 348), struct.pack("<10s18s", b"", b""), struct.pack("<ihcB", 0, 0, b"r", 0), struct.pack("<8h", *dim),
        struct.pack("<3f", 0.0, 0.0, 0.0), struct.pack("<4h", 0, 16, 32, 0), struct.pack("<8f", *pix),
        struct.pack("<3f", 352.0, 0.0, 0.0), struct.pack("<hBB", 0, 0, 10), struct.pack("<4f", 0.0, 0.0, 0.0, 0.0),
        struct.pack("<2i", 0, 0), struct.pack("<80s24s", b"packed by the test", b""), struct.pack("<2h", qform_code, sform_code),
        struct.pack("<6f", *quatern, *qoffset), struct.pack("<12f", *[v for r in srows for v in r]),
        struct.pack("<16s4s", b"", b"n+1\0")])
    assert len(raw) == 348
    return raw


def quaternion_affine(b, c, d, pix, qfac, off):
    """nifti1.h, method 2."""
    a = np.sqrt(1.0 - (b * b + c * c + d * d))
    r = np.array([[a * a + b * b - c * c - d * d, 2 * b * c - 2 * a * d, 2 * b * d + 2 * a * c],
                  [2 * b * c + 2 * a * d, a * a + c * c - b * b - d * d, 2 * c * d - 2 * a * b],
                  [2 * b * d - 2 * a * c, 2 * c * d + 2 * a * b, a * a + d * d - c * c - b * b]])
    aff = np.eye(4)
    aff[:3, :3] = r * np.array([pix[0], pix[1], pix[2] * qfac])
    aff[:3, 3] = off
    return aff


@pytest.mark.parametrize("form", ["sform", "qform"])
def test_three_doubled_axes_keep_the_volume_in_place(tmp_path, form):
    shape, pix = (4, 6, 3), (0.9, 1.1, 3.0)
    if form == "sform":
        raw = pack_header(shape, (1.0,) + pix, sform_code=2, srows=OBLIQUE)
        affine_in = np.array(OBLIQUE + [[0, 0, 0, 1]], dtype=np.float64)
    else:
        quat, off, qfac = (0.1, -0.2, 0.3), (-80.5, 100.25, -12.0), -1.0
        raw = pack_header(shape, (qfac,) + pix, qform_code=1, quatern=quat, qoffset=off)
        affine_in = quaternion_affine(*quat, pix, qfac, off)
    src = tmp_path / "in.nii"
    src.write_bytes(raw + b"\0" * 4 + np.arange(72, dtype="<f4").tobytes())
    _, hdr = read_nifti(str(src))
    assert np.allclose(hdr.affine(), affine_in, rtol=1e-6, atol=1e-5)
    out_shape = (8, 12, 6)
    path = tmp_path / "out.nii"
    write_nifti(str(path), np.zeros(out_shape, dtype=np.float32), hdr, (0, 1, 2))
    _, h2 = read_nifti(str(path))
    assert h2.shape == out_shape and h2.get("dim")[:4] == [3, 8, 12, 6]
    assert h2.get("pixdim")[1:4] == pytest.approx([p / 2 for p in pix])
    assert h2.get("pixdim")[0] == hdr.get("pixdim")[0]
    if form == "qform":
        names = ("quatern_b", "quatern_c", "quatern_d")
        assert [h2.get(k) for k in names] == [hdr.get(k) for k in names]
        affine_out = quaternion_affine(*(h2.get(k) for k in names), h2.get("pixdim")[1:4], -1.0 if h2.get("pixdim")[0] < 0 else 1.0,
                                       [h2.get(k) for k in ("qoffset_x", "qoffset_y", "qoffset_z")])
    else:
        affine_out = np.array([h2.get("srow_x"), h2.get("srow_y"), h2.get("srow_z"), [0, 0, 0, 1]], dtype=np.float64)
    assert np.allclose(h2.affine(), affine_out, rtol=1e-6, atol=1e-5)
    # the centre of the volume: input (1.5, 2.5, 1.0), output (3.5, 5.5, 2.5)
    centre_in = affine_in @ np.array([(s - 1) / 2 for s in shape] + [1.0])
    centre_out = affine_out @ np.array([(s - 1) / 2 for s in out_shape] + [1.0])
    assert np.allclose(centre_out, centre_in, rtol=0, atol=2e-4)          # header floats are float32: ~1e-5 at |x| ~ 100
    last = [s - 1 for s in out_shape]
    corners = [(i, j, k) for i in (0, last[0]) for j in (0, last[1]) for k in (0, last[2])]
    for o in corners + [(1, 2, 1), (3, 5, 2)]:
        want = affine_in @ np.array([v / 2 - 0.25 for v in o] + [1.0])
        got = affine_out @ np.array(list(o) + [1.0])
        assert np.allclose(got, want, rtol=0, atol=2e-4), (form, o, got, want)
    with pytest.raises(ValueError):
        write_nifti(str(path), np.zeros((8, 12, 3), dtype=np.float32), hdr, (0, 1, 2))      # shape does not fit three axes
    with pytest.raises(ValueError):
        write_nifti(str(path), np.zeros(out_shape, dtype=np.float32), hdr, (0, 1, 1))


def test_isotropic_flag_parses_and_defaults_are_unchanged():
    from scripts import infer_volume
    base = ["--input", "a.nii", "--output", "b.nii"]
    plain = vars(infer_volume.parse_args(base))
    assert plain.pop("isotropic") is False
    assert plain == {"input": "a.nii", "output": "b.nii", "checkpoint_dir": "./checkpoints", "checkpoint_path": None, "model_type": "unet",
                     "base_filters": 64, "cpu": False, "use_amp": False, "axis": 2, "batch_size": 16, "no_graph": False,
                     "output_dtype": "float32"}
    iso = vars(infer_volume.parse_args(base + ["--isotropic", "--output_dtype", "int16", "--no_graph", "--use_amp"]))
    assert iso["isotropic"] is True and iso["output_dtype"] == "int16" and iso["no_graph"] and iso["use_amp"] and iso["axis"] == 2
