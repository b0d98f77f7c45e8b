"""Single-file NIfTI-1 reading and writing for whole-volume inference (extension), host only:
numpy, ``struct`` and ``gzip`` - no nibabel.

``read_nifti(path)``                                  -> ``(float32 array in the file's index order, NiftiHeader)``
``write_nifti(path, data, header, upscaled_axes)``    the x2 output under the input's header, geometry moved with it
``frames(data)``, ``mask_frames(path, ...)``          a 3-D / 4-D array as 3-D timepoints; a mask file as one uint8 frame each
``grid_matrix``, ``downscaled_affine``, ``respaced_grid``, ``header_for_grid``    grid arithmetic for reslicing one scan onto
                                                      another's grid (``volume_reslice.py``), float64

What the reference sees of a volume is ``nib.load(path).get_fdata().astype(np.float32)`` (``utils/extraction_utils.py:118``):
the stored values, scaled by ``scl_slope`` / ``scl_inter`` in float64 when a slope is set, cast to float32.

Geometry of the output.  The model's x2 is a half-pixel-centred upsampling: output index ``o`` along an upscaled axis sits at
input coordinate ``o / 2 - 1 / 4``.  With the input affine's columns ``c_a`` of the upscaled axes and its translation ``t``,
the output affine has the columns ``c_a / 2`` and the translation ``t`` minus a quarter of the sum of those columns (two for
a slice pass across one axis, all three for the isotropic output): the volume stays where it was in world space.  Applied to the sform rows when ``sform_code > 0`` and to the qform (pixdim halved, offsets moved by the same
vector built from the qform's own axes, quaternion unchanged) when ``qform_code > 0``.
"""
from __future__ import annotations

import gzip
import logging
import struct
from typing import Sequence, Tuple

import numpy as np

logger = logging.getLogger("nifti")

HEADER_BYTES = 348
# name -> (byte offset, struct format) of the NIfTI-1 header (nifti1.h)
FIELDS = {
    "sizeof_hdr": (0, "i"), "dim_info": (39, "B"), "dim": (40, "8h"), "intent_p1": (56, "f"), "intent_p2": (60, "f"),
    "intent_p3": (64, "f"), "intent_code": (68, "h"), "datatype": (70, "h"), "bitpix": (72, "h"), "slice_start": (74, "h"),
    "pixdim": (76, "8f"), "vox_offset": (108, "f"), "scl_slope": (112, "f"), "scl_inter": (116, "f"), "slice_end": (120, "h"),
    "slice_code": (122, "B"), "xyzt_units": (123, "B"), "cal_max": (124, "f"), "cal_min": (128, "f"),
    "slice_duration": (132, "f"), "toffset": (136, "f"), "descrip": (148, "80s"), "aux_file": (228, "24s"),
    "qform_code": (252, "h"), "sform_code": (254, "h"), "quatern_b": (256, "f"), "quatern_c": (260, "f"),
    "quatern_d": (264, "f"), "qoffset_x": (268, "f"), "qoffset_y": (272, "f"), "qoffset_z": (276, "f"),
    "srow_x": (280, "4f"), "srow_y": (296, "4f"), "srow_z": (312, "4f"), "intent_name": (328, "16s"), "magic": (344, "4s"),
}
# datatype code -> (numpy kind and size, bitpix)
DATATYPES = {2: ("u1", 8), 4: ("i2", 16), 8: ("i4", 32), 16: ("f4", 32), 64: ("f8", 64), 256: ("i1", 8), 512: ("u2", 16),
             768: ("u4", 32)}
_REFUSED_TYPES = {0: "unknown", 1: "binary", 32: "complex64", 128: "RGB24", 1024: "int64", 1280: "uint64", 1536: "float128",
                  1792: "complex128", 2048: "complex256", 2304: "RGBA32"}


class NiftiHeader:
    """The 348 header bytes as read, their byte order, and field access by name (``FIELDS``)."""

    def __init__(self, raw: bytes, endian: str = "<"):
        if len(raw) != HEADER_BYTES or endian not in ("<", ">"):
            raise ValueError(f"a NIfTI-1 header is {HEADER_BYTES} bytes in '<' or '>' order, got {len(raw)} bytes, {endian!r}")
        self.raw = bytearray(raw)
        self.endian = endian

    @classmethod
    def new(cls, shape: Sequence[int], pixdim: Sequence[float] = (1.0, 1.0, 1.0), affine=None, endian: str = "<") -> "NiftiHeader":
        """A minimal float32 header for a 3-D / 4-D volume of ``shape``: voxel sizes in mm, ``affine`` (4x4) as the sform."""
        hdr = cls(bytes(HEADER_BYTES), endian)
        hdr.set("sizeof_hdr", HEADER_BYTES)
        hdr.set("dim", [len(shape)] + [int(d) for d in shape] + [1] * (7 - len(shape)))
        hdr.set("pixdim", [1.0] + [float(p) for p in pixdim] + [1.0] * (7 - len(pixdim)))
        hdr.set("datatype", 16)
        hdr.set("bitpix", 32)
        hdr.set("vox_offset", 352.0)
        hdr.set("scl_slope", 1.0)
        hdr.set("xyzt_units", 2)
        hdr.set("magic", b"n+1\0")
        if affine is not None:
            hdr.set("sform_code", 1)
            for row, name in enumerate(("srow_x", "srow_y", "srow_z")):
                hdr.set(name, [float(v) for v in np.asarray(affine)[row]])
        return hdr

    def get(self, name: str):
        off, fmt = FIELDS[name]
        v = struct.unpack_from(self.endian + fmt, self.raw, off)
        return v[0] if len(v) == 1 else list(v)

    def set(self, name: str, value):
        off, fmt = FIELDS[name]
        struct.pack_into(self.endian + fmt, self.raw, off, *(value if isinstance(value, (list, tuple)) else (value,)))

    def copy(self) -> "NiftiHeader":
        return NiftiHeader(bytes(self.raw), self.endian)

    @property
    def shape(self) -> Tuple[int, ...]:
        dim = self.get("dim")
        return tuple(dim[1:1 + dim[0]])

    def sform_affine(self) -> np.ndarray:
        return np.array([self.get("srow_x"), self.get("srow_y"), self.get("srow_z"), [0, 0, 0, 1]], dtype=np.float64)

    def qform_affine(self) -> np.ndarray:
        """nifti1.h's quaternion form: rotation of (b, c, d), columns scaled by pixdim[1..3], the third by qfac = pixdim[0]."""
        b, c, d = (float(self.get(k)) for k in ("quatern_b", "quatern_c", "quatern_d"))
        a = np.sqrt(max(0.0, 1.0 - (b * b + c * c + d * d)))
        rot = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                        [2 * (b * c + a * d), a * a + c * c - b * b - d * d, 2 * (c * d - a * b)],
                        [2 * (b * d - a * c), 2 * (c * d + a * b), a * a + d * d - b * b - c * c]])
        pix = self.get("pixdim")
        aff = np.eye(4)
        aff[:3, :3] = rot * np.array([pix[1], pix[2], pix[3] * (-1.0 if pix[0] < 0 else 1.0)])
        aff[:3, 3] = [self.get("qoffset_x"), self.get("qoffset_y"), self.get("qoffset_z")]
        return aff

    def affine(self) -> np.ndarray:
        """Index -> world: the sform when set, else the qform, else the pixdim scaling (nifti1.h's methods 3, 2, 1)."""
        if self.get("sform_code") > 0:
            return self.sform_affine()
        if self.get("qform_code") > 0:
            return self.qform_affine()
        pix = self.get("pixdim")
        return np.diag([pix[1], pix[2], pix[3], 1.0])


def _read_bytes(path: str) -> bytes:
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rb") as f:
        return f.read()


def read_nifti(path: str):
    """-> ``(data, header)``: float32 ndarray of shape ``dim[1..ndim]`` (3 or 4 axes; the file's Fortran order kept as the
    array's memory order) and the ``NiftiHeader``.  Values are ``raw * scl_slope + scl_inter`` in float64 cast to float32 when
    ``scl_slope`` is neither 0 nor NaN, else the raw values cast.  Non-finite voxels become 0 (logged).  ``ValueError`` names
    the offending field for everything that is not a 3-D / 4-D single-file NIfTI-1 of a real integer or float type."""
    blob = _read_bytes(path)
    if len(blob) < 4:
        raise ValueError(f"{path}: sizeof_hdr missing, file of {len(blob)} bytes")
    endian = None
    for e in ("<", ">"):
        size = struct.unpack_from(e + "i", blob, 0)[0]
        if size == HEADER_BYTES:
            endian = e
        elif size == 540:
            raise ValueError(f"{path}: sizeof_hdr 540 is NIfTI-2, only NIfTI-1 is read")
    if endian is None:
        raise ValueError(f"{path}: sizeof_hdr {struct.unpack_from('<i', blob, 0)[0]} is not 348 in either byte order")
    if len(blob) < HEADER_BYTES:
        raise ValueError(f"{path}: file of {len(blob)} bytes is shorter than the header (sizeof_hdr 348)")
    hdr = NiftiHeader(blob[:HEADER_BYTES], endian)
    magic = hdr.get("magic")
    if magic == b"ni1\0":
        raise ValueError(f"{path}: magic 'ni1' is the two-file form (.hdr / .img), only single-file 'n+1' is read")
    if magic != b"n+1\0":
        raise ValueError(f"{path}: magic {magic!r} is not 'n+1\\0'")
    dim = hdr.get("dim")
    if dim[0] not in (3, 4):
        raise ValueError(f"{path}: dim[0] = {dim[0]}, only 3-D and 4-D volumes are read")
    shape = tuple(dim[1:1 + dim[0]])
    if any(d < 1 for d in shape):
        raise ValueError(f"{path}: dim {dim} has an empty axis")
    code = hdr.get("datatype")
    if code not in DATATYPES:
        raise ValueError(f"{path}: datatype {code} ({_REFUSED_TYPES.get(code, 'unknown')}) is not a real integer or float type "
                         f"of {sorted(DATATYPES)}")
    kind, bitpix = DATATYPES[code]
    if hdr.get("bitpix") != bitpix:
        raise ValueError(f"{path}: bitpix {hdr.get('bitpix')} does not belong to datatype {code} ({bitpix})")
    offset = hdr.get("vox_offset")
    if not np.isfinite(offset) or offset < HEADER_BYTES or offset != int(offset):
        raise ValueError(f"{path}: vox_offset {offset} lies inside the header")
    offset, count = int(offset), int(np.prod(shape, dtype=np.int64))
    if len(blob) < offset + count * bitpix // 8:
        raise ValueError(f"{path}: file of {len(blob)} bytes is shorter than vox_offset {offset} + {count} voxels of "
                         f"{bitpix // 8} bytes (dim {list(shape)})")
    raw = np.frombuffer(blob, dtype=np.dtype(endian + kind), count=count, offset=offset).reshape(shape, order="F")
    slope, inter = hdr.get("scl_slope"), hdr.get("scl_inter")
    if slope != 0 and not np.isnan(slope):
        data = (raw.astype(np.float64) * float(slope) + float(inter)).astype(np.float32)
    else:
        data = raw.astype(np.float32)
    bad = ~np.isfinite(data)
    if bad.any():
        logger.warning(f"{path}: {int(bad.sum())} non-finite voxel(s) set to 0")
        data[bad] = 0
    return data, hdr


def frames(data: np.ndarray) -> list:
    """A 3-D array as ``[data]``, a 4-D array as the list of its timepoints ``data[..., t]`` (views)."""
    return [data] if data.ndim == 3 else [data[..., t] for t in range(data.shape[3])]


def mask_frames(path: str, spatial_shape, count: int, what: str = "mask"):
    """-> (``count`` contiguous uint8 arrays, 1 where the file is non-zero, one per timepoint of the scan the mask belongs to; the
    file's ``NiftiHeader``).  A 3-D mask serves every timepoint (one array, ``count`` times), a 4-D one needs ``count`` of its own.
    ``spatial_shape``: the three extents the mask must have, None for a mask that may lie on any grid.  ``what`` names the mask in
    the errors."""
    data, header = read_nifti(path)
    if spatial_shape is not None and tuple(data.shape[:3]) != tuple(spatial_shape):
        raise ValueError(f"{what} {path} has shape {tuple(data.shape)}, a scan of {tuple(spatial_shape)} voxels needs the same")
    out = [np.ascontiguousarray((f != 0).astype(np.uint8)) for f in frames(data)]
    if data.ndim == 4 and len(out) != count:
        raise ValueError(f"{what} {path} has {len(out)} timepoints, {count} are needed")
    return (out if data.ndim == 4 else out * count), header


def upscaled_affine(affine: np.ndarray, upscaled_axes: Sequence[int]) -> np.ndarray:
    """Affine of the x2 output: columns of the upscaled axes halved, translation moved by minus a quarter of their sum."""
    src = np.asarray(affine, dtype=np.float64)
    out = src.copy()
    for a in upscaled_axes:
        out[:3, 3] -= 0.25 * src[:3, a]
        out[:3, a] = 0.5 * src[:3, a]
    return out


def downscaled_affine(affine: np.ndarray, axes: Sequence[int]) -> np.ndarray:
    """The exact inverse of ``upscaled_affine``: columns of ``axes`` doubled, translation moved by plus a quarter of the NEW
    columns - the grid on which a x2 pass over ``axes`` expects its low-resolution input."""
    src = np.asarray(affine, dtype=np.float64)
    out = src.copy()
    for a in axes:
        out[:3, a] = 2.0 * src[:3, a]
        out[:3, 3] += 0.25 * out[:3, a]
    return out


def check_affine(affine, what) -> np.ndarray:
    a = np.asarray(affine, dtype=np.float64)
    if a.shape != (4, 4):
        raise ValueError(f"{what} must be a 4 x 4 index -> world affine, got shape {a.shape}")
    return a


def grid_matrix(src_affine: np.ndarray, dst_affine: np.ndarray) -> np.ndarray:
    """(3, 4) float64: the first three rows of ``inv(src_affine) @ dst_affine`` (``np.linalg.solve``) - a voxel index of the
    destination grid -> the continuous voxel index of the source grid.  A singular or non-finite ``src_affine`` (or a non-finite
    ``dst_affine``) is a ``ValueError``."""
    src, dst = check_affine(src_affine, "src_affine"), check_affine(dst_affine, "dst_affine")
    if not np.isfinite(src).all() or not np.isfinite(dst).all():
        raise ValueError("grid_matrix: an affine has an entry that is not finite")
    try:
        with np.errstate(all="ignore"):
            m = np.linalg.solve(src, dst)
    except np.linalg.LinAlgError as e:
        raise ValueError(f"grid_matrix: the source affine is singular ({e})") from None
    if not np.isfinite(m).all() or np.linalg.matrix_rank(src) < 4:
        raise ValueError("grid_matrix: the source affine is singular")
    return np.ascontiguousarray(m[:3])


def respaced_grid(affine: np.ndarray, shape: Sequence[int], spacing: Sequence[float]):
    """-> ``(affine', shape')``: the grid of ``(affine, shape)`` with the voxel size of axis ``a`` changed to ``spacing[a]`` (``None``
    or 0 keeps the axis).  Voxels are cells with their centres at the integer indices.  Per axis: ``s = |affine[:3, a]|``,
    ``n' = max(1, ceil(n s / s' - 1e-6))``, ``col' = col s' / s``; translation ``t' = t - sum(col) / 2 + sum(col') / 2``: the
    corner of the first cell stays where it was in world space.  Halving the spacing of two or three axes gives
    ``upscaled_affine`` and the doubled shape."""
    src = check_affine(affine, "affine")
    shape = tuple(int(d) for d in shape)
    if len(shape) != 3 or any(d < 1 for d in shape) or len(tuple(spacing)) != 3:
        raise ValueError(f"respaced_grid takes three positive extents and three spacings, got {shape} and {tuple(spacing)}")
    out, new_shape = src.copy(), list(shape)
    for a, want in enumerate(spacing):
        if want is None or want == 0:
            continue
        s = float(np.linalg.norm(src[:3, a]))
        if not (np.isfinite(want) and want > 0) or not (np.isfinite(s) and s > 0):
            raise ValueError(f"respaced_grid: spacing {want} for axis {a} of voxel size {s} (both must be positive and finite)")
        new_shape[a] = max(1, int(np.ceil(shape[a] * s / float(want) - 1e-6)))
        out[:3, a] = src[:3, a] * (float(want) / s)
    out[:3, 3] = src[:3, 3] - 0.5 * src[:3, :3].sum(axis=1) + 0.5 * out[:3, :3].sum(axis=1)
    return out, tuple(new_shape)


def header_for_grid(header: NiftiHeader, shape: Sequence[int], affine: np.ndarray) -> NiftiHeader:
    """A copy of ``header`` for a volume on the grid ``(affine, shape)``: ``dim[1..3]`` from ``shape``, ``pixdim[1..3]`` the
    column norms of ``affine``, ``srow_*`` its rows, ``sform_code`` kept when positive (else 1) and ``qform_code = 0`` - a
    general affine has no quaternion form, the sform alone then defines the grid.  ``dim[0]``, ``dim[4]``, the byte order and
    everything else are kept; ``write_nifti(path, data, that_header)`` takes it as it is."""
    aff = check_affine(affine, "affine")
    shape = tuple(int(d) for d in shape)
    if len(shape) != 3 or any(not 1 <= d <= 32767 for d in shape) or not np.isfinite(aff).all():
        raise ValueError(f"header_for_grid takes three extents in 1..32767 and a finite affine, got {shape}")
    hdr = header.copy()
    dim, pix = list(hdr.get("dim")), list(hdr.get("pixdim"))
    dim[1:4] = shape
    pix[1:4] = [float(np.linalg.norm(aff[:3, a])) for a in range(3)]
    hdr.set("dim", dim)
    hdr.set("pixdim", pix)
    for row, name in enumerate(("srow_x", "srow_y", "srow_z")):
        hdr.set(name, [float(v) for v in aff[row]])
    if hdr.get("sform_code") <= 0:
        hdr.set("sform_code", 1)
    hdr.set("qform_code", 0)
    return hdr


def write_nifti(path: str, data: np.ndarray, header: NiftiHeader, upscaled_axes: Sequence[int] = ()):
    """Writes float32, int16 or uint8 ``data`` (3-D or 4-D) as single-file NIfTI-1 under a copy of ``header`` (its byte order kept):
    ``dim`` from ``data.shape``, which must be the header's with the ``upscaled_axes`` (two or all three of 0, 1, 2, or none) doubled;
    their ``pixdim`` halved and the sform / qform moved as the module docstring says; ``datatype`` / ``bitpix`` set,
    ``scl_slope = 1``, ``scl_inter = 0``, ``vox_offset = 352``, magic ``n+1``.  gzip when the name ends in ``.gz``."""
    data = np.asarray(data)
    codes = {np.dtype(np.float32): 16, np.dtype(np.int16): 4, np.dtype(np.uint8): 2}
    if data.dtype not in codes:
        raise ValueError(f"write_nifti writes float32, int16 or uint8, not {data.dtype}")
    if data.ndim not in (3, 4):
        raise ValueError(f"write_nifti writes 3-D or 4-D volumes, not {data.shape}")
    axes = tuple(int(a) for a in upscaled_axes)
    if len(axes) not in (0, 2, 3) or len(set(axes)) != len(axes) or any(a not in (0, 1, 2) for a in axes):
        raise ValueError(f"upscaled_axes must be two or three different axes of 0, 1, 2 (or none), got {upscaled_axes}")
    hdr = header.copy()
    old_dim = hdr.get("dim")
    expect = tuple(old_dim[1 + a] * (2 if a in axes else 1) for a in range(data.ndim))
    if old_dim[0] != data.ndim or expect != data.shape:
        raise ValueError(f"data of shape {data.shape} does not fit header dim {old_dim} with axes {axes} doubled ({expect})")
    sform, qform = hdr.sform_affine(), hdr.qform_affine()
    dim, pix = list(old_dim), hdr.get("pixdim")
    for a in axes:
        dim[1 + a] = data.shape[a]
        pix[1 + a] = pix[1 + a] / 2
    hdr.set("dim", dim)
    hdr.set("pixdim", pix)
    if hdr.get("sform_code") > 0:
        new = upscaled_affine(sform, axes)
        for row, name in enumerate(("srow_x", "srow_y", "srow_z")):
            hdr.set(name, [float(v) for v in new[row]])
    if hdr.get("qform_code") > 0:
        new = upscaled_affine(qform, axes)
        for row, name in enumerate(("qoffset_x", "qoffset_y", "qoffset_z")):
            hdr.set(name, float(new[row, 3]))
    code = codes[data.dtype]
    hdr.set("datatype", code)
    hdr.set("bitpix", DATATYPES[code][1])
    hdr.set("scl_slope", 1.0)
    hdr.set("scl_inter", 0.0)
    hdr.set("vox_offset", 352.0)
    hdr.set("magic", b"n+1\0")
    payload = bytes(hdr.raw) + b"\0\0\0\0" + np.asarray(data, dtype=data.dtype.newbyteorder(hdr.endian)).tobytes(order="F")
    if str(path).endswith(".gz"):
        with gzip.open(path, "wb", compresslevel=1) as f:
            f.write(payload)
    else:
        with open(path, "wb") as f:
            f.write(payload)
    return hdr
