"""Edge sharpness across tissue interfaces on the device (extension): SSIM and PSNR reward smoothness, Dice and
the surface distances are taken on hard labels and are blind to the slope of an edge.  This module measures that slope: the signed
distance of every voxel to the interface between the tissue classes ``1..k`` and ``k+1..K``, the edge-spread function of a volume
across that interface (the mean intensity as a function of the signed distance) and its 10 % - 90 % width in millimetres.

``interface_sides_np``, ``signed_distance_np``, ``edge_profile_np``      the specification.
``edge_width``          host float64, shared by the specification and the device path: a profile -> width and contrast.
``interface_sides``, ``signed_distance``, ``signed_distances``, ``edge_profile``, ``edge_sharpness``, ``EdgeWorkspace``      the device
                        path (``csrc/volume_edge.hip``), equal to the specification bit for bit except the three float64 sums of a
                        profile, which are added in another order.  There is no CPU path: CPU tensors raise.

The signed distance is measured between voxel centres (``volume_surface.edt_sq_np``): ``+`` the distance to the nearest voxel of the
darker side on the brighter side, ``-`` the distance to the nearest voxel of the brighter side on the darker side.  The interface
itself lies between voxel centres, so no voxel has ``|s|`` below the smallest voxel size and the abscissa has a gap around 0.  This is
left as it is: the same ``s``, taken from the reference's labels, serves every method, so comparisons stay fair.

Device path: per interface 1 launch for the sides, 6 for the two transforms and 1 for the signed distance; per scored volume ONE
launch for the profiles of all interfaces (it reads the volume at most once and every signed distance once, writes no volume and
is HIP-graph capturable) and one that adds the fixed slots; one download of ``J * nb * 32`` bytes at the end.

Not built: a half-voxel correction of the abscissa, an erf fit / MTF, widths per region, a 2-D form for ``scripts/evaluate.py``.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from ._volume_args import NO_CPU, check_classes, check_extents, check_spacing, cuda_device, cuda_tensor, u8_np, volume_np
from .volume_surface import distance_transform_sq, edt_sq_np

MAX_INTERFACES = 5                   # K <= 6 tissue classes
MIN_BINS, MAX_BINS = 2, 64
WORDS = 4                            # per bin: the count (int64) and the float64 sums of v, s and v * v


class EdgeProfile(NamedTuple):
    count: np.ndarray                # (J, nb) int64
    sum_v: np.ndarray                # (J, nb) float64: the sum of the intensities
    sum_s: np.ndarray                # (J, nb) float64: the sum of the signed distances
    sum_vv: np.ndarray               # (J, nb) float64: the sum of the squared intensities


class EdgeSharpness(NamedTuple):
    width: np.ndarray                # (J,) float64: the 10 % - 90 % width of the edge, in the unit of ``spacing``; NaN where undefined
    contrast: np.ndarray             # (J,) float64: the difference of the two plateaus
    profile: EdgeProfile


# ---------------------------------------------------------------- checks shared by both paths

def _check_interface(k) -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= 254:
        raise ValueError(f"k must be an integer in 1..254 (the interface between the classes 1..k and k+1..K), got {k!r}")
    return int(k)


def check_bins(radius, bin_width):
    """-> (R, w, nb): the radius and the bin width as float32 and ``nb = ceil(2 radius / bin_width)`` of the numbers given."""
    try:
        r, w = float(radius), float(bin_width)
    except (TypeError, ValueError):
        r = w = float("nan")
    with np.errstate(over="ignore"):
        r32, w32 = np.float32(r), np.float32(w)
    if not (np.isfinite(r32) and r32 > 0 and np.isfinite(w32) and w32 > 0):
        raise ValueError(f"radius and bin_width are finite positive numbers (float32), got {radius!r} and {bin_width!r}")
    nb = math.ceil(2.0 * r / w)
    if not MIN_BINS <= nb <= MAX_BINS:
        raise ValueError(f"radius {r:g} and bin_width {w:g} give {nb} bins: {MIN_BINS}..{MAX_BINS} are supported")
    return r32, w32, int(nb)


def edge_width(profile, min_count=8):
    """profile: an ``EdgeProfile`` (or its four (J, nb) arrays) -> ``(width (J,), contrast (J,))`` in float64.

    Per interface the bins with ``count >= min_count`` are kept, in ascending order; ``n`` of them.  Abscissa ``x_b = sum_s / count``,
    mean ``m_b = sum_v / count``.  The plateaus ``L`` and ``H`` are the means of ``m_b`` over the outermost ``max(1, n // 8)`` kept bins
    on the dark and on the bright end, ``contrast = H - L`` and ``p_b = (m_b - L) / contrast``.  From the first kept bin with
    ``p >= 0.5`` the walk goes right to the first ``p >= 0.9`` and left to the first ``p <= 0.1``; each crossing is interpolated
    linearly between that bin and its neighbour on the side of the start.  ``width = x90 - x10``.  The width is NaN when a crossing is
    not reached or ``contrast <= 0``; width and contrast are NaN when fewer than 4 bins are kept."""
    if isinstance(min_count, bool) or not isinstance(min_count, (int, np.integer)) or min_count < 1:
        raise ValueError(f"min_count must be a positive integer, got {min_count!r}")
    count, sum_v, sum_s = (np.asarray(a) for a in profile[:3])
    if count.ndim != 2 or sum_v.shape != count.shape or sum_s.shape != count.shape:
        raise ValueError(f"a profile holds (J, nb) arrays, got {count.shape}, {sum_v.shape} and {sum_s.shape}")
    J = count.shape[0]
    width, contrast = np.full(J, np.nan, dtype=np.float64), np.full(J, np.nan, dtype=np.float64)
    for j in range(J):
        keep = np.flatnonzero(count[j] >= min_count)
        n = keep.size
        if n < 4:
            continue
        c = count[j, keep].astype(np.float64)
        x, m = sum_s[j, keep].astype(np.float64) / c, sum_v[j, keep].astype(np.float64) / c
        ends = max(1, n // 8)
        low, high = float(np.mean(m[:ends])), float(np.mean(m[n - ends:]))
        contrast[j] = high - low
        if not contrast[j] > 0:
            continue
        p = (m - low) / contrast[j]
        above = np.flatnonzero(p >= 0.5)
        if above.size == 0:
            continue
        start = int(above[0])
        hi = next((i for i in range(start, n) if p[i] >= 0.9), None)
        lo = next((i for i in range(start - 1, -1, -1) if p[i] <= 0.1), None)
        if hi is None or lo is None or hi == 0:
            continue
        x90 = x[hi - 1] + (0.9 - p[hi - 1]) / (p[hi] - p[hi - 1]) * (x[hi] - x[hi - 1])
        x10 = x[lo] + (0.1 - p[lo]) / (p[lo + 1] - p[lo]) * (x[lo + 1] - x[lo])
        width[j] = x90 - x10
    return width, contrast


# ---------------------------------------------------------------- numpy specification

def interface_sides_np(labels, k) -> np.ndarray:
    """uint8, the shape of ``labels``: 0 where ``labels == 0``, 1 where ``0 < labels <= k`` (the darker side: classes are ordered by
    brightness, as ``volume_tissue.segment_tissue`` returns them), 2 where ``labels > k``."""
    labels = u8_np(labels, None, "the labels", ndim=3)
    k = _check_interface(k)
    return np.where(labels == 0, 0, np.where(labels <= k, 1, 2)).astype(np.uint8)


def signed_distance_np(labels, k, spacing=(1, 1, 1)) -> np.ndarray:
    """float32, the shape of ``labels``: with ``sides = interface_sides_np(labels, k)`` and ``w`` the squared voxel sizes
    (``_volume_args.check_spacing``), ``dA = sqrt32(edt_sq_np(sides, 1, w))`` and ``dB = sqrt32(edt_sq_np(sides, 2, w))``, each one
    correctly rounded float32 square root, ``+inf`` where that side is absent.  ``s = +dA`` on side 2, ``s = -dB`` on side 1, NaN on
    side 0.  Distances run between voxel centres: no voxel has ``|s|`` below the smallest voxel size (module docstring)."""
    w = check_spacing(spacing)
    sides = interface_sides_np(labels, k)
    check_extents(sides.shape, "signed_distance_np")
    d_a, d_b = np.sqrt(edt_sq_np(sides, 1, w)), np.sqrt(edt_sq_np(sides, 2, w))
    return np.where(sides == 2, d_a, np.where(sides == 1, -d_b, np.float32(np.nan))).astype(np.float32)


def _check_profile_np(vol, sdist):
    vol, sdist = volume_np(vol, "edge_profile_np"), np.asarray(sdist)
    if sdist.dtype != np.float32 or sdist.ndim != 4 or sdist.shape[1:] != vol.shape or not 1 <= sdist.shape[0] <= MAX_INTERFACES:
        raise ValueError(f"edge_profile_np: the signed distances are float32 (J, {', '.join(str(d) for d in vol.shape)}) with J in "
                         f"1..{MAX_INTERFACES}, got {sdist.dtype} {sdist.shape}")
    return vol, sdist


def edge_profile_np(vol, sdist, radius=4.0, bin_width=0.5) -> EdgeProfile:
    """The specification of ``edge_profile``: ``vol`` float32 (X, Y, Z), ``sdist`` float32 (J, X, Y, Z), one signed distance per
    interface.  ``nb = ceil(2 radius / bin_width)`` in 2..64.  With ``R`` and ``w`` the float32 values of ``radius`` and ``bin_width``, a
    voxel enters bin ``b = floor(fl32(fl32(s + R) / w))`` of interface ``j`` when ``s`` is finite, ``0 <= b < nb`` and ``vol`` is finite
    there.  ``count`` (J, nb) int64; ``sum_v``, ``sum_s``, ``sum_vv`` (J, nb) float64, taken over ``float64(v)``, ``float64(s)`` and
    ``float64(v) * float64(v)`` (``math.fsum``)."""
    r32, w32, nb = check_bins(radius, bin_width)
    vol, sdist = _check_profile_np(vol, sdist)
    J = sdist.shape[0]
    count = np.zeros((J, nb), dtype=np.int64)
    sums = np.zeros((3, J, nb), dtype=np.float64)
    v = vol.reshape(-1)
    for j in range(J):
        s = sdist[j].reshape(-1)
        with np.errstate(invalid="ignore", over="ignore"):
            b = np.floor((s + r32) / w32)                              # float32 + float32, float32 / float32: one rounding each
            ok = np.isfinite(s) & (b >= 0) & (b < nb) & np.isfinite(v)
        idx = b[ok].astype(np.int64)
        v64, s64 = v[ok].astype(np.float64), s[ok].astype(np.float64)
        count[j] = np.bincount(idx, minlength=nb)
        for b_ in np.unique(idx):
            sel = idx == b_
            sums[0, j, b_] = math.fsum(v64[sel])
            sums[1, j, b_] = math.fsum(s64[sel])
            sums[2, j, b_] = math.fsum(v64[sel] * v64[sel])
    return EdgeProfile(count, sums[0], sums[1], sums[2])


def edge_sharpness_np(vol, labels, classes=3, spacing=(1, 1, 1), radius=4.0, bin_width=0.5, min_count=8) -> EdgeSharpness:
    """The specification of ``edge_sharpness``: the signed distances of the ``classes - 1`` interfaces of ``labels``, the profile of
    ``vol`` across each and ``edge_width`` of it."""
    K = check_classes(classes)
    sdist = np.stack([signed_distance_np(labels, k, spacing) for k in range(1, K)])
    profile = edge_profile_np(vol, sdist, radius, bin_width)
    return EdgeSharpness(*edge_width(profile, min_count), profile)


# ---------------------------------------------------------------- device

def _check_f32(t, shape, what, name):
    return cuda_tensor(t, (torch.float32,), what, name=name, shape=shape)


def _check_volume_labels(labels, what):
    return cuda_tensor(labels, (torch.uint8,), what, ndim=3)


def interface_sides(labels: torch.Tensor, k, out=None) -> torch.Tensor:
    """The device form of ``interface_sides_np``: ``labels`` a contiguous uint8 CUDA volume -> a uint8 CUDA volume, one launch.
    ``out``: a uint8 CUDA tensor of that shape to write into."""
    t = _check_volume_labels(labels, "interface_sides")
    k = _check_interface(k)
    out = torch.empty_like(t) if out is None else cuda_tensor(out, (torch.uint8,), "interface_sides (out)", shape=t.shape)
    L.call("mrisr_u8_volume_interface_sides", t.data_ptr(), t.numel(), k, out.data_ptr(), L.stream_ptr(), nbytes=2 * t.numel())
    return out


def signed_distance(labels: torch.Tensor, k, spacing=(1, 1, 1), out=None, scratch=None) -> torch.Tensor:
    """The device form of ``signed_distance_np``, the same contract and the same bits, NaN and infinities included: ``labels`` a
    contiguous uint8 CUDA volume (every axis at most 1024) -> a float32 CUDA volume.  8 launches: the sides, two distance
    transforms (``volume_surface.distance_transform_sq``'s kernels), the signed root.  ``out``: a contiguous float32 CUDA tensor of
    that shape to write into; ``scratch``: ``(sides uint8, dA float32, dB float32)`` of that shape, so that nothing is allocated."""
    t = _check_volume_labels(labels, "signed_distance")
    k, w = _check_interface(k), check_spacing(spacing)
    check_extents(tuple(t.shape), "signed_distance")
    out = torch.empty(t.shape, dtype=torch.float32, device=t.device) if out is None else _check_f32(out, t.shape, "signed_distance", "out")
    if scratch is None:
        scratch = (torch.empty_like(t), torch.empty_like(out), torch.empty_like(out))
    sides, d_a, d_b = scratch
    interface_sides(t, k, out=sides)
    distance_transform_sq(sides, 1, w, out=d_a)
    distance_transform_sq(sides, 2, w, out=d_b)
    L.call("mrisr_f32_volume_signed_distance", sides.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), t.numel(), out.data_ptr(), L.stream_ptr(),
           nbytes=13 * t.numel())
    return out


def signed_distances(labels: torch.Tensor, classes=3, spacing=(1, 1, 1)) -> torch.Tensor:
    """-> float32 CUDA tensor (classes - 1, X, Y, Z): ``signed_distance`` for ``k = 1 .. classes - 1``, one scratch set for all."""
    K = check_classes(classes)
    t = _check_volume_labels(labels, "signed_distances")
    check_spacing(spacing)
    check_extents(tuple(t.shape), "signed_distances")
    out = torch.empty((K - 1,) + tuple(t.shape), dtype=torch.float32, device=t.device)
    scratch = (torch.empty_like(t), torch.empty_like(out[0]), torch.empty_like(out[0]))
    for k in range(1, K):
        signed_distance(t, k, spacing, out=out[k - 1], scratch=scratch)
    return out


class EdgeWorkspace:
    """The buffers of ``edge_profile`` for ``interfaces`` signed distances and ``bins`` bins on ``device`` (any volume size), so that
    nothing is allocated in a call and a call can be captured in a HIP graph; it may serve call after call on one stream.
    ``results`` is the tensor a call returns: the next call with this workspace overwrites it."""

    def __init__(self, interfaces, bins, device):
        if isinstance(interfaces, bool) or not isinstance(interfaces, (int, np.integer)) or not 1 <= interfaces <= MAX_INTERFACES:
            raise ValueError(f"interfaces must be an integer in 1..{MAX_INTERFACES}, got {interfaces!r}")
        if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not MIN_BINS <= bins <= MAX_BINS:
            raise ValueError(f"bins must be an integer in {MIN_BINS}..{MAX_BINS}, got {bins!r}")
        device = cuda_device(device, "EdgeWorkspace")
        self.interfaces, self.bins, self.device = int(interfaces), int(bins), device
        nbytes = int(L.load().mrisr_f32_volume_edge_workspace_bytes(self.interfaces, self.bins))
        self.slots = torch.empty(nbytes // 8, dtype=torch.int64, device=device)
        self.results = torch.zeros((self.interfaces, self.bins, WORDS), dtype=torch.int64, device=device)
        self.host = torch.empty(self.results.shape, dtype=torch.int64).pin_memory()

    def download(self) -> EdgeProfile:
        self.host.copy_(self.results, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return profile_of(self.host.numpy())


def profile_of(words: np.ndarray) -> EdgeProfile:
    """(J, nb, 4) int64 words of ``edge_profile`` on the host -> the ``EdgeProfile`` (copies)."""
    words = np.ascontiguousarray(words)
    sums = words.view(np.float64)
    return EdgeProfile(words[..., 0].copy(), sums[..., 1].copy(), sums[..., 2].copy(), sums[..., 3].copy())


def edge_profile(vol: torch.Tensor, sdist: torch.Tensor, radius=4.0, bin_width=0.5, workspace=None) -> torch.Tensor:
    """The device path of ``edge_profile_np``: ``vol`` a contiguous float32 CUDA volume, ``sdist`` a contiguous float32 CUDA tensor
    (J, X, Y, Z) -> the int64 CUDA tensor (J, nb, 4) of ``workspace.results``: per bin the count and the bits of the float64 sums of
    ``v``, ``s`` and ``v * v`` (``profile_of`` reads it on the host).  The counts equal the specification's; the sums are those of
    another order of addition, the same bits on every run: a wave owns a fixed set of voxels, lanes that share a bin are added in a
    fixed tree, partial sums go to fixed slots and are added in slot order.  Two launches, no host synchronisation, no allocation
    with a ``workspace`` (an ``EdgeWorkspace(J, nb, device)``): capturable in a HIP graph."""
    r32, w32, nb = check_bins(radius, bin_width)
    if not isinstance(vol, torch.Tensor) or not vol.is_cuda or not isinstance(sdist, torch.Tensor) or not sdist.is_cuda:
        raise ValueError(f"edge_profile {NO_CPU}: expected CUDA tensors")
    if vol.dim() != 3:
        raise ValueError(f"edge_profile: expected a volume (X, Y, Z), got {tuple(vol.shape)}")
    v = _check_f32(vol, None, "edge_profile", "vol")
    if sdist.dim() != 4 or not 1 <= sdist.shape[0] <= MAX_INTERFACES:
        raise ValueError(f"edge_profile: the signed distances are (J, X, Y, Z) with J in 1..{MAX_INTERFACES}, got {tuple(sdist.shape)}")
    s = _check_f32(sdist, (sdist.shape[0],) + tuple(v.shape), "edge_profile", "sdist")
    J = int(s.shape[0])
    ws = EdgeWorkspace(J, nb, v.device) if workspace is None else workspace
    if not isinstance(ws, EdgeWorkspace) or ws.interfaces != J or ws.bins != nb or ws.device != v.device:
        raise ValueError(f"the workspace must be an EdgeWorkspace({J}, {nb}, {v.device})")
    L.call("mrisr_f32_volume_edge_profile", v.data_ptr(), s.data_ptr(), J, v.numel(), float(r32), float(w32), nb, ws.slots.data_ptr(),
           ws.results.data_ptr(), L.stream_ptr(), nbytes=4 * (J + 1) * v.numel())
    return ws.results


def edge_sharpness(vol: torch.Tensor, labels: torch.Tensor = None, classes=3, spacing=(1, 1, 1), radius=4.0, bin_width=0.5, min_count=8,
                   workspace=None, sdist=None) -> EdgeSharpness:
    """The device path of ``edge_sharpness_np``: ``vol`` a float32 CUDA volume, ``labels`` a uint8 CUDA label volume of that shape with
    the classes ``1..classes`` ordered by brightness -> ``EdgeSharpness`` on the host, one entry per interface ``k = 1 .. classes - 1``:
    the 10 % - 90 % width of the edge of ``vol`` across it in the unit of ``spacing``, the contrast of its two plateaus and the profile.
    ``sdist``: the result of ``signed_distances(labels, classes, spacing)`` taken earlier (``labels``, ``classes`` and ``spacing`` are
    then not read) - the way to score several volumes against one label volume.  One download for all interfaces, at the end."""
    if sdist is None:
        if labels is None:
            raise ValueError("edge_sharpness needs labels or sdist")
        sdist = signed_distances(labels, classes, spacing)
    ws = workspace
    if ws is None and isinstance(sdist, torch.Tensor) and sdist.is_cuda and sdist.dim() == 4:
        ws = EdgeWorkspace(int(sdist.shape[0]), check_bins(radius, bin_width)[2], sdist.device)
    edge_profile(vol, sdist, radius, bin_width, ws)                    # with ws None it raises: the arguments are wrong
    profile = ws.download()
    return EdgeSharpness(*edge_width(profile, min_count), profile)
