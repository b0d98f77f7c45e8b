"""utils/nifti.py against NIfTI-1 files packed here, field by field from the nifti1.h layout, with ``struct``: reading
(byte orders, gzip, datatypes, scaling, 3-D / 4-D), refusals, the write -> read round trip, and the geometry of the x2 output
(world position of output voxel o = input affine at o / 2 - 1 / 4 along the upscaled axes).  No GPU needed."""
import gzip
import struct

import numpy as np
import pytest

from mri_superresolution_amd.utils.nifti import read_nifti, write_nifti

NP_OF = {2: "u1", 4: "i2", 8: "i4", 16: "f4", 64: "f8", 256: "i1", 512: "u2", 768: "u4"}


def pack_header(shape, datatype, endian="<", slope=0.0, inter=0.0, pixdim=(1.0, 1.0, 1.0, 1.0, 1.0), qform_code=0, sform_code=0,
                quatern=(0.0, 0.0, 0.0), qoffset=(0.0, 0.0, 0.0), srows=None, magic=b"n+1\0", sizeof_hdr=348, vox_offset=352.0,
                bitpix=None):
    """348 bytes, every field of nifti1.h in its order."""
    e = endian
    dim = [len(shape)] + list(shape) + [1] * (7 - len(shape))
    pix = list(pixdim) + [0.0] * (8 - len(pixdim))
    srows = srows if srows is not None else [[0.0] * 4] * 3
    bitpix = np.dtype(NP_OF[datatype]).itemsize * 8 if bitpix is None else bitpix
    parts = [
        struct.pack(e + "i", sizeof_hdr),                   # sizeof_hdr
        struct.pack(e + "10s18s", b"", b""),                # data_type, db_name
        struct.pack(e + "ihcB", 0, 0, b"r", 0),             # extents, session_error, regular, dim_info
        struct.pack(e + "8h", *dim),                        # dim
        struct.pack(e + "3f", 0.0, 0.0, 0.0),               # intent_p1..3
        struct.pack(e + "4h", 0, datatype, bitpix, 0),      # intent_code, datatype, bitpix, slice_start
        struct.pack(e + "8f", *pix),                        # pixdim
        struct.pack(e + "3f", vox_offset, slope, inter),    # vox_offset, scl_slope, scl_inter
        struct.pack(e + "hBB", 0, 0, 10),                   # slice_end, slice_code, xyzt_units
        struct.pack(e + "4f", 0.0, 0.0, 0.0, 0.0),          # cal_max, cal_min, slice_duration, toffset
        struct.pack(e + "2i", 0, 0),                        # glmax, glmin
        struct.pack(e + "80s24s", b"packed by the test", b""),   # descrip, aux_file
        struct.pack(e + "2h", qform_code, sform_code),      # qform_code, sform_code
        struct.pack(e + "6f", *quatern, *qoffset),          # quatern_b/c/d, qoffset_x/y/z
        struct.pack(e + "12f", *[v for r in srows for v in r]),   # srow_x, srow_y, srow_z
        struct.pack(e + "16s4s", b"", magic),               # intent_name, magic
    ]
    raw = b"".join(parts)
    assert len(raw) == 348
    return raw


def write_file(path, raw_header, voxels, endian="<", pad=4):
    blob = raw_header + b"\0" * pad + voxels.astype(voxels.dtype.newbyteorder(endian)).tobytes(order="F")
    if str(path).endswith(".gz"):
        with gzip.open(path, "wb") as f:
            f.write(blob)
    else:
        path.write_bytes(blob)
    return blob


def ramp(shape, dtype, lo, hi):
    n = int(np.prod(shape))
    return np.linspace(lo, hi, n).astype(dtype).reshape(shape)      # C-order ramp: the Fortran order of the file matters


@pytest.mark.parametrize("endian", ["<", ">"])
@pytest.mark.parametrize("suffix", [".nii", ".nii.gz"])
def test_reads_packed_files(tmp_path, endian, suffix):
    cases = [((5, 7, 3), 4, ramp((5, 7, 3), np.int16, -3000, 3000), 0.5, -10.0),
             ((5, 7, 3), 4, ramp((5, 7, 3), np.int16, -3000, 3000), 0.0, 5.0),          # slope 0: unscaled
             ((4, 6, 2), 2, ramp((4, 6, 2), np.uint8, 0, 255), float("nan"), 0.0),      # slope NaN: unscaled
             ((4, 6, 2), 16, ramp((4, 6, 2), np.float32, -1.5, 2.5e4), 0.0, 0.0),
             ((3, 5, 2, 2), 16, ramp((3, 5, 2, 2), np.float32, 0, 4095), 1.0, 0.0),     # 4-D
             ((3, 4, 2), 512, ramp((3, 4, 2), np.uint16, 0, 65535), 2.0, 1.0),
             ((3, 4, 2), 64, ramp((3, 4, 2), np.float64, -1e3, 1e3), 0.0, 0.0),
             ((3, 4, 2), 8, ramp((3, 4, 2), np.int32, -100000, 100000), 0.0, 0.0),
             ((3, 4, 2), 256, ramp((3, 4, 2), np.int8, -128, 127), 0.0, 0.0),
             ((3, 4, 2), 768, ramp((3, 4, 2), np.uint32, 0, 4e9), 0.0, 0.0)]
    for i, (shape, code, vox, slope, inter) in enumerate(cases):
        path = tmp_path / f"case{i}{suffix}"
        write_file(path, pack_header(shape, code, endian, slope, inter, pixdim=(1.0, 0.9, 1.1, 3.0, 2.0)), vox, endian)
        data, hdr = read_nifti(str(path))
        scaled = slope != 0.0 and not np.isnan(slope)
        want = (vox.astype(np.float64) * slope + inter).astype(np.float32) if scaled else vox.astype(np.float32)
        assert data.dtype == np.float32 and data.shape == shape
        assert np.array_equal(data, want), (i, endian, suffix)
        assert hdr.endian == endian and hdr.shape == shape and hdr.get("datatype") == code
        assert hdr.get("pixdim")[1:4] == pytest.approx([0.9, 1.1, 3.0])


def test_non_finite_voxels_become_zero(tmp_path, caplog):
    vox = ramp((3, 4, 2), np.float32, 1, 24)
    vox[1, 2, 1], vox[0, 0, 0] = np.nan, np.inf
    path = tmp_path / "nan.nii"
    write_file(path, pack_header((3, 4, 2), 16), vox)
    with caplog.at_level("WARNING"):
        data, _ = read_nifti(str(path))
    want = vox.copy()
    want[1, 2, 1] = want[0, 0, 0] = 0
    assert np.array_equal(data, want)
    assert any("non-finite" in r.getMessage() for r in caplog.records)


def test_refusals_name_the_field(tmp_path):
    vox = ramp((3, 4, 2), np.int16, 0, 23)

    def refused(name, raw, voxels=vox, match=None, cut=None):
        path = tmp_path / name
        blob = write_file(path, raw, voxels)
        if cut is not None:
            path.write_bytes(blob[:cut])
        with pytest.raises(ValueError, match=match):
            read_nifti(str(path))

    refused("nifti2.nii", pack_header((3, 4, 2), 4, sizeof_hdr=540), match="sizeof_hdr")
    refused("nifti2_be.nii", pack_header((3, 4, 2), 4, endian=">", sizeof_hdr=540), match="sizeof_hdr")
    refused("garbage.nii", pack_header((3, 4, 2), 4, sizeof_hdr=123), match="sizeof_hdr")
    refused("twofile.nii", pack_header((3, 4, 2), 4, magic=b"ni1\0"), match="magic")
    refused("nomagic.nii", pack_header((3, 4, 2), 4, magic=b"\0\0\0\0"), match="magic")
    refused("five_d.nii", pack_header((3, 4, 2, 1, 1), 4), match="dim")
    refused("two_d.nii", pack_header((3, 8), 4), match="dim")
    for code, bitpix in ((32, 64), (1792, 128), (128, 24), (2304, 32), (1024, 64)):      # complex64 / 128, RGB24, RGBA32, int64
        refused(f"type{code}.nii", pack_header((3, 4, 2), code, bitpix=bitpix), match="datatype")
    refused("bitpix.nii", pack_header((3, 4, 2), 4, bitpix=32), match="bitpix")
    refused("short_data.nii", pack_header((3, 4, 2), 4), match="shorter", cut=352 + 2 * 23)
    refused("short_header.nii", pack_header((3, 4, 2), 4), match="shorter", cut=200)
    refused("offset.nii", pack_header((3, 4, 2), 4, vox_offset=100.0), match="vox_offset")


OBLIQUE = [[1.1, -0.2, 0.3, -90.0], [0.15, 0.9, -0.25, 120.5], [-0.3, 0.2, 2.8, -7.25]]


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


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
@pytest.mark.parametrize("suffix", [".nii", ".nii.gz"])
def test_write_read_round_trip(tmp_path, dtype, suffix):
    shape = (4, 6, 3)
    src = tmp_path / "in.nii"
    write_file(src, pack_header(shape, 4, ">", slope=2.0, inter=3.0, sform_code=1, srows=OBLIQUE), ramp(shape, np.int16, 0, 71), ">")
    _, hdr = read_nifti(str(src))
    out = ramp((8, 12, 3), dtype, -2000, 2000)
    path = tmp_path / f"out{suffix}"
    write_nifti(str(path), out, hdr, (0, 1))
    back, h2 = read_nifti(str(path))
    assert np.array_equal(back, out.astype(np.float32)) and back.shape == (8, 12, 3)
    assert h2.endian == ">" and h2.get("datatype") == (16 if dtype == np.float32 else 4) and h2.get("bitpix") == (32 if dtype == np.float32 else 16)
    assert h2.get("scl_slope") == 1.0 and h2.get("scl_inter") == 0.0 and h2.get("vox_offset") == 352.0
    assert h2.get("descrip").rstrip(b"\0") == b"packed by the test"      # the rest of the header is the input's
    assert hdr.get("dim")[1:4] == [4, 6, 3]                              # the caller's header is not modified
    # no upscaled axes: same geometry
    same = tmp_path / "same.nii"
    write_nifti(str(same), ramp(shape, dtype, 0, 71), hdr, ())
    _, h3 = read_nifti(str(same))
    assert np.allclose(h3.affine(), np.array(OBLIQUE + [[0, 0, 0, 1]]), rtol=1e-6) and h3.shape == shape
    with pytest.raises(ValueError):
        write_nifti(str(same), ramp((8, 12, 3), dtype, 0, 1), hdr, (0, 2))      # shape does not fit these axes
    with pytest.raises(ValueError):
        write_nifti(str(same), ramp(shape, np.float64, 0, 1), hdr, ())


@pytest.mark.parametrize("form", ["sform", "qform"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_output_geometry_keeps_the_volume_in_place(tmp_path, form, axis):
    shape = (4, 6, 3)
    pix = (0.9, 1.1, 3.0)
    if form == "sform":
        raw = pack_header(shape, 16, pixdim=(1.0,) + pix, sform_code=2, srows=OBLIQUE)
        affine_in = np.array(OBLIQUE + [[0, 0, 0, 1]], dtype=np.float64)
    else:
        quat, off, qfac = (0.1, -0.2, 0.3), (-80.5, 100.25, -12.0), -1.0
        raw = pack_header(shape, 16, pixdim=(qfac,) + pix, qform_code=1, quatern=quat, qoffset=off)
        affine_in = quaternion_affine(*quat, pix, qfac, off)
    src = tmp_path / "in.nii"
    write_file(src, raw, ramp(shape, np.float32, 0, 71))
    _, hdr = read_nifti(str(src))
    assert np.allclose(hdr.affine(), affine_in, rtol=1e-6, atol=1e-5)
    in_plane = tuple(a for a in (0, 1, 2) if a != axis)
    out_shape = tuple(s * (2 if a in in_plane else 1) for a, s in enumerate(shape))
    path = tmp_path / "out.nii"
    write_nifti(str(path), np.zeros(out_shape, dtype=np.float32), hdr, in_plane)
    _, h2 = read_nifti(str(path))
    assert h2.shape == out_shape
    assert h2.get("pixdim")[1:4] == pytest.approx([p / (2 if a in in_plane else 1) for a, p in enumerate(pix)])
    assert h2.get("pixdim")[0] == hdr.get("pixdim")[0]
    if form == "qform":
        assert [h2.get(k) for k in ("quatern_b", "quatern_c", "quatern_d")] == [hdr.get(k) for k in ("quatern_b", "quatern_c", "quatern_d")]
        affine_out = quaternion_affine(*(h2.get(k) for k in ("quatern_b", "quatern_c", "quatern_d")), h2.get("pixdim")[1:4],
                                       -1.0 if h2.get("pixdim")[0] < 0 else 1.0, [h2.get(k) for k in ("qoffset_x", "qoffset_y", "qoffset_z")])
    else:
        affine_out = np.array([h2.get("srow_x"), h2.get("srow_y"), h2.get("srow_z"), [0, 0, 0, 1]], dtype=np.float64)
    last = [s - 1 for s in out_shape]
    voxels = [(0, 0, 0), tuple(last), (last[0], 0, 0), (0, last[1], 0), (0, 0, last[2]), (last[0], last[1], 0), (1, 2, 1), (3, 5, 2)]
    for o in voxels:
        src_coord = [o[a] / 2 - 0.25 if a in in_plane else o[a] for a in range(3)]
        want = affine_in @ np.array(src_coord + [1.0])
        got = affine_out @ np.array(list(o) + [1.0])
        assert np.allclose(got, want, rtol=0, atol=2e-4), (form, axis, o, got, want)      # header floats are float32: ~1e-5 at |x| ~ 100
