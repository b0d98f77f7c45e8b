"""Surface distances between two label volumes on the device (extension): Dice says how much of a tissue class
overlaps, not how far its boundary has moved.  The companions are the average symmetric surface distance (ASSD), the 95th-percentile
Hausdorff distance (HD95) and the Hausdorff distance (HD) in millimetres.  All three rest on the exact Euclidean distance transform
(EDT) of a voxel set with anisotropic voxel sizes, which is public here on its own.

``boundary_np``, ``distance_table_np``, ``edt_sq_np``, ``surface_distances_np``      the specification.
``label_boundary``, ``distance_transform_sq``, ``surface_distances``, ``SurfaceWorkspace``      the device path
                        (``csrc/volume_surface.hip``), equal to the specification bit for bit except ``assd``, whose float64 sum is
                        added in another order.  There is no CPU path: CPU tensors raise.

The squared distance of a voxel is a minimum over a set of float32 numbers, each formed by the same rounded operations in both
paths; rounding is monotone, so the order in which candidates are visited changes no bit and any exact algorithm gives the same
result.  With unit weights every value is an exact integer (an axis is at most 1024 voxels: 3 * 1023^2 < 2^24).

Device path: ``surface_distances`` makes 2 launches for the two boundaries and, per class and direction, 3 for the transform, 2 for
the gather and the 9 of ``masked_percentiles``; one download of ``(8 K + 1) * 8`` bytes at the end covers all classes.

Not built: morphology by a radius in mm, distances to an atlas surface, a linear-time (lower-envelope)
transform, axes longer than 1024 voxels, a 2-D form for ``scripts/evaluate.py``.  The signed distance to a tissue interface is
``volume_sharpness.signed_distance``.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from ._volume_args import MAX_EXTENT, check_classes, check_extents, check_spacing, cuda_device, cuda_tensor, u8_np      # noqa: F401  (MAX_EXTENT: this module's documented limit)
from ._volume_args import check_weights as _check_weights      # private here as before; it lives there because check_spacing builds on it
from .utils.imageops import np_percentile_f32
from .volume_intensity import masked_percentiles, percentiles_workspace

P95 = 95.0


class SurfaceDistances(NamedTuple):
    counts: np.ndarray               # (K, 2) int64: boundary voxels of class k + 1 in a and in b
    assd: np.ndarray                 # (K,) float64, in the unit of ``spacing``; NaN where a count is 0
    hd95: np.ndarray                 # (K,) float64
    hd: np.ndarray                   # (K,) float64


# ---------------------------------------------------------------- checks shared by both paths

def _check_value(value) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 0 <= value <= 255:
        raise ValueError(f"value must be an integer in 0..255, got {value!r}")
    return int(value)


def _finish(counts, sums, maxima, p95) -> SurfaceDistances:
    """counts (K, 2) int64, sums (K, 2) float64, maxima and p95 (K, 2) float32 -> the three distances; NaN where a count is 0."""
    K = counts.shape[0]
    assd, hd95, hd = (np.full(K, np.nan, dtype=np.float64) for _ in range(3))
    for k in range(K):
        na, nb = int(counts[k, 0]), int(counts[k, 1])
        if na == 0 or nb == 0:
            continue
        assd[k] = (float(sums[k, 0]) + float(sums[k, 1])) / float(na + nb)
        hd95[k] = float(max(p95[k, 0], p95[k, 1]))
        hd[k] = float(max(maxima[k, 0], maxima[k, 1]))
    return SurfaceDistances(counts.astype(np.int64), assd, hd95, hd)


# ---------------------------------------------------------------- numpy specification

def boundary_np(labels, background=True) -> np.ndarray:
    """uint8, the shape of ``labels``: ``out[v] = labels[v]`` if ``labels[v] != 0`` and at least one of the 6 face neighbours differs,
    else 0.  ``background=True``: a neighbour differs if it lies outside the volume or carries another label, 0 included.
    ``background=False``: only if it lies inside the volume and carries another non-zero label - the interfaces between tissues."""
    labels = u8_np(labels, None, "the labels", ndim=3)
    p = np.pad(labels.astype(np.int16), 1, constant_values=-1)           # -1: outside the volume
    X, Y, Z = labels.shape
    edge = np.zeros(labels.shape, dtype=bool)
    for nb in (p[0:X, 1:-1, 1:-1], p[2:X + 2, 1:-1, 1:-1], p[1:-1, 0:Y, 1:-1], p[1:-1, 2:Y + 2, 1:-1], p[1:-1, 1:-1, 0:Z], p[1:-1, 1:-1, 2:Z + 2]):
        edge |= (nb != labels) if background else ((nb > 0) & (nb != labels))
    return np.where(edge & (labels != 0), labels, 0).astype(np.uint8)


def distance_table_np(n, w) -> np.ndarray:
    """float32 (n,): ``T[d] = fl32(w32 * fl32(d * d))``, a rounded float32 product of the float32 weight and the integer ``d * d``
    (exactly representable for d < 4096)."""
    d = np.arange(int(n), dtype=np.int64)
    with np.errstate(over="ignore"):
        return np.float32(w) * (d * d).astype(np.float32)


def edt_sq_np(sites, value=0, weights=(1, 1, 1)) -> np.ndarray:
    """float32 (X, Y, Z): the squared distance of every voxel to the nearest site.  A voxel is a site if ``sites[v] == value``, or if
    ``sites[v] != 0`` when ``value == 0``.  ``g = 0`` at the sites and ``+inf`` elsewhere; then for axis 2, 1, 0:
    ``g'[i] = min_j fl32(g[j] + T[|i - j|])`` along that axis with ``T = distance_table_np(extent, weights[axis])``.  ``weights``: the
    squared voxel sizes, float32.  No site: ``+inf`` everywhere.  An axis is at most 1024 voxels."""
    sites = u8_np(sites, None, "the sites", ndim=3)
    value, w = _check_value(value), _check_weights(weights)
    check_extents(sites.shape, "edt_sq_np")
    g = np.where(sites == value if value else sites != 0, np.float32(0), np.float32(np.inf)).astype(np.float32)
    for axis in (2, 1, 0):
        n = g.shape[axis]
        T = distance_table_np(n, w[axis])
        line = np.moveaxis(g, axis, -1)
        best = np.full(line.shape, np.inf, dtype=np.float32)
        idx = np.arange(n)
        for j in range(n):
            np.minimum(best, line[..., j:j + 1] + T[np.abs(idx - j)], out=best)      # float32 + float32: one rounded sum
        g = np.ascontiguousarray(np.moveaxis(best, -1, axis))
    return g


def surface_distances_np(a, b, classes=3, spacing=(1, 1, 1), background=True) -> SurfaceDistances:
    """The specification of ``surface_distances``: ``a``, ``b`` uint8 label volumes of one shape with labels 0..K.  Per class k:
    ``Sa = boundary_np(a, background) == k``, ``Sb`` likewise; ``Dab = sqrt32(edt_sq_np(boundary_np(b), k, spacing^2))[Sa]`` (a correctly
    rounded float32 square root), ``Dba`` the mirror image; ``hd = max(Dab.max(), Dba.max())``, ``hd95 = max(P95(Dab), P95(Dba))`` with
    numpy's float32 percentile (``utils.imageops.np_percentile_f32``), ``assd = (fsum(Dab) + fsum(Dba)) / (na + nb)`` in float64.  A
    class whose surface is empty on either side gives NaN in all three, decided from the counts: no infinity reaches a sum."""
    K = check_classes(classes)
    w = check_spacing(spacing)
    a = u8_np(a, None, "a", ndim=3)
    b = u8_np(b, a.shape, "b", ndim=3)
    check_extents(a.shape, "surface_distances_np")
    bad = int((a > K).sum()) + int((b > K).sum())
    if bad:
        raise ValueError(f"{bad} voxel(s) carry a label above {K}")
    ba, bb = boundary_np(a, background), boundary_np(b, background)
    counts, sums = np.zeros((K, 2), dtype=np.int64), np.zeros((K, 2), dtype=np.float64)
    maxima, p95 = np.zeros((K, 2), dtype=np.float32), np.zeros((K, 2), dtype=np.float32)
    for k in range(1, K + 1):
        sa, sb = ba == k, bb == k
        counts[k - 1] = int(sa.sum()), int(sb.sum())
        if not counts[k - 1].all():
            continue
        for side, (query, other) in enumerate(((sa, bb), (sb, ba))):
            d = np.sqrt(edt_sq_np(other, k, w))[query]
            sums[k - 1, side] = math.fsum(float(x) for x in d)
            maxima[k - 1, side] = d.max()
            p95[k - 1, side] = np_percentile_f32(np.sort(d), P95)
    return _finish(counts, sums, maxima, p95)


# ---------------------------------------------------------------- device

def label_boundary(labels: torch.Tensor, background=True, out=None) -> torch.Tensor:
    """The device form of ``boundary_np``: ``labels`` a contiguous uint8 CUDA volume (X, Y, Z) -> a uint8 CUDA volume, one launch for all
    classes.  ``out``: a uint8 CUDA tensor of that shape to write into (not ``labels`` itself)."""
    t = cuda_tensor(labels, (torch.uint8,), "label_boundary")
    if t.dim() != 3:
        raise ValueError(f"label_boundary: expected a volume (X, Y, Z), got {tuple(t.shape)}")
    out = torch.empty_like(t) if out is None else cuda_tensor(out, (torch.uint8,), "label_boundary (out)", shape=t.shape)
    L.call("mrisr_u8_volume_label_boundary", t.data_ptr(), *t.shape, int(bool(background)), 255, out.data_ptr(), None, L.stream_ptr(),
           nbytes=2 * t.numel())
    return out


def _edt_launch(sites, shape, value, w, out, passes=7, full_scan=False):
    """``passes`` (a mask of the axes) and ``full_scan`` are for measurement (``tools/surface_bench.py``) and for the tests."""
    L.call("mrisr_u8_volume_edt_sq", sites.data_ptr(), *shape, value, float(w[0]), float(w[1]), float(w[2]), out.data_ptr(),
           int(passes), int(bool(full_scan)), L.stream_ptr())


def distance_transform_sq(sites: torch.Tensor, value=0, weights=(1, 1, 1), out=None) -> torch.Tensor:
    """The device form of ``edt_sq_np``, the same contract: ``sites`` a contiguous uint8 CUDA volume (X, Y, Z), every axis at most 1024
    -> the float32 CUDA volume of squared distances, bit-equal to the specification, infinities included.  Three launches, in place
    in the result, no scratch volume.  ``out``: a contiguous float32 CUDA tensor of that shape to write into."""
    t = cuda_tensor(sites, (torch.uint8,), "distance_transform_sq")
    value, w = _check_value(value), _check_weights(weights)
    check_extents(tuple(t.shape), "distance_transform_sq")
    if out is None:
        out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
    elif not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32 or out.shape != t.shape or not out.is_contiguous():
        raise ValueError(f"distance_transform_sq: out must be a contiguous float32 CUDA tensor of shape {tuple(t.shape)}")
    _edt_launch(t, t.shape, value, w, out)
    return out


class SurfaceWorkspace:
    """Every buffer of ``surface_distances`` for label volumes of ``shape`` and ``classes`` classes on ``device``, so that nothing is
    allocated inside the loop over the classes; it may serve call after call on one stream."""

    def __init__(self, shape, classes, device):
        K = check_classes(classes)
        shape = tuple(int(d) for d in shape)
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError(f"a volume shape (X, Y, Z) is expected, got {shape}")
        check_extents(shape, "SurfaceWorkspace")
        device = cuda_device(device, "SurfaceWorkspace")
        self.shape, self.classes, self.device = shape, K, device
        self.boundary = [torch.empty(shape, dtype=torch.uint8, device=device) for _ in range(2)]
        self.d2 = torch.empty(shape, dtype=torch.float32, device=device)
        self.dist = torch.empty(shape, dtype=torch.float32, device=device)
        self.sel = torch.empty(shape, dtype=torch.uint8, device=device)
        self.slots = torch.empty(int(L.load().mrisr_f32_volume_surface_workspace_bytes()) // 8, dtype=torch.int64, device=device)
        self.percentiles = percentiles_workspace(1, device)
        # 8-byte words, 4 per class and direction: the count, the float64 sum, the maximum, the P95 (float32 in the low half each);
        # the last word counts the voxels with a label above K
        self.results = torch.zeros(K * 2 * 4 + 1, dtype=torch.int64, device=device)
        self.results_f32 = self.results.view(torch.float32)
        self.pcount = torch.empty(1, dtype=torch.int64, device=device)
        self.host = torch.empty(self.results.shape, dtype=torch.int64).pin_memory()

    def download(self) -> np.ndarray:
        self.host.copy_(self.results, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return self.host.numpy()


def _gather(d2, query, value, dist, sel, slots, results, word):
    L.call("mrisr_f32_volume_surface_gather", d2.data_ptr(), query.data_ptr(), int(value), d2.numel(), dist.data_ptr(), sel.data_ptr(),
           slots.data_ptr(), results.data_ptr() + 8 * word, L.stream_ptr(), nbytes=10 * d2.numel())


def surface_distances(a: torch.Tensor, b: torch.Tensor, classes=3, spacing=(1, 1, 1), background=True, workspace=None) -> SurfaceDistances:
    """The device path of ``surface_distances_np``, the same contract: ``a``, ``b`` contiguous uint8 CUDA label volumes of one shape (every
    axis at most 1024) -> ``SurfaceDistances`` on the host; ``counts``, ``hd`` and ``hd95`` equal the specification's, ``assd`` to the
    rounding of a float64 sum added in another order.  P95 is ``masked_percentiles`` of the gathered distances.  ``workspace``: a
    ``SurfaceWorkspace`` of this shape and class count; with one nothing is allocated here.  One download at the end covers all
    classes; a label above K is counted by the boundary kernel and raises ``ValueError`` then."""
    K = check_classes(classes)
    w = check_spacing(spacing)
    a = cuda_tensor(a, (torch.uint8,), "surface_distances")
    b = cuda_tensor(b, (torch.uint8,), "surface_distances", shape=a.shape)
    check_extents(tuple(a.shape), "surface_distances")
    ws = SurfaceWorkspace(a.shape, K, a.device) if workspace is None else workspace
    if not isinstance(ws, SurfaceWorkspace) or ws.shape != tuple(a.shape) or ws.classes != K or ws.device != a.device:
        raise ValueError(f"the workspace must be a SurfaceWorkspace({tuple(a.shape)}, {K}, {a.device})")
    ws.results.zero_()
    above = ws.results.data_ptr() + 8 * (K * 2 * 4)
    for vol, edge in zip((a, b), ws.boundary):
        L.call("mrisr_u8_volume_label_boundary", vol.data_ptr(), *ws.shape, int(bool(background)), K, edge.data_ptr(), above, L.stream_ptr(),
               nbytes=2 * vol.numel())
    for k in range(1, K + 1):
        for side, (query, other) in enumerate(((ws.boundary[0], ws.boundary[1]), (ws.boundary[1], ws.boundary[0]))):
            word = ((k - 1) * 2 + side) * 4
            _edt_launch(other, ws.shape, k, w, ws.d2)
            _gather(ws.d2, query, k, ws.dist, ws.sel, ws.slots, ws.results, word)
            masked_percentiles(ws.dist, ws.sel, (P95,), ws.percentiles, out=(ws.results_f32[2 * (word + 3):2 * (word + 3) + 1], ws.pcount))
    host = ws.download()
    if host[-1]:
        raise ValueError(f"{int(host[-1])} voxel(s) carry a label above {K}")
    words = host[:-1].reshape(K, 2, 4)
    low = np.ascontiguousarray(words).view(np.float32).reshape(K, 2, 4, 2)[..., 0]      # the low half of every word
    return _finish(words[..., 0].copy(), np.ascontiguousarray(words[..., 1]).view(np.float64), low[..., 2], low[..., 3])
