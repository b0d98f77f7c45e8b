"""Tissue classification of volumes on the device and the overlap of two label volumes (extension): whether a
x2 volume keeps the anatomy is judged by segmenting it and the reference into K tissue classes and reporting the Dice overlap per
class.  The model is a Gaussian mixture on a 256-bin quantisation of the foreground with a Potts prior over the 6 face neighbours,
minimised by iterated conditional modes (ICM) in a checkerboard order.  Everything a voxel takes part in is integer arithmetic: the
class parameters and the cost table are computed on the host from a K x 256 joint histogram, by the same numpy function in the
specification and in the device path.

``quantise_np``, ``kmeans_hist_np``, ``cost_table_np``, ``icm_half_np``, ``icm_sweep_np``, ``energy_np``, ``segment_tissue_np``,
``confusion_np``, ``dice_np``        the specification.
``segment_tissue``, ``label_confusion``, ``dice``, ``TissueWorkspace``      the device path (``csrc/volume_tissue.hip``), equal to the
                        specification bit for bit in every field.  There is no CPU path: CPU tensors raise.

Device path, the host round trip: every iteration downloads one small tensor (the number of changed voxels and the K x 256 joint
histogram, at most 12 KB) and uploads the cost table (at most 6 KB).  That is deliberate: the table is then the specification's
own numpy code, and the early exit needs ``changed`` on the host anyway.  The three launches of an iteration (two half-sweeps, the
joint histogram of the new labels) follow each other without synchronisation.

Not built: skull stripping, soft (fuzzy) memberships, a bias field inside the model (``volume_bias`` matches the bias between scans),
atlas priors, a 2-D form for ``scripts/evaluate.py``.
"""
from __future__ import annotations

import logging
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from ._volume_args import MAX_CLASSES, MIN_CLASSES, check_classes, cuda_device, cuda_tensor, mask_tensor, u8_np, volume_np
from .volume_intensity import RANGE, landmarks_np, masked_percentiles, percentiles_workspace

logger = logging.getLogger(__name__)

BINS = 256
MAX_BETA, MAX_ITERATIONS = 16.0, 100
COST_SHIFT = 16                      # costs and beta are fixed point with 16 fractional bits
COST_CAP = 1 << 30                   # cost + 6 beta_q stays below 2^31
MIN_VARIANCE = 1.0 / 12.0            # the variance of a uniform distribution over one bin
KMEANS_ROUNDS = 50


class TissueSegmentation(NamedTuple):
    labels: object                   # uint8, 0 outside the mask, 1..K inside, class 1 the darkest (numpy array / CUDA tensor)
    means: np.ndarray                # (K,) float64, in intensity units: the bin centre of the class mean mapped back through lo, scale
    variances: np.ndarray            # (K,) float64, in intensity units squared
    counts: np.ndarray               # (K,) int64 voxels per class
    sweeps: int                      # ICM sweeps made after the maximum-likelihood labels
    changed: int                     # labels the last sweep changed (0: converged)
    lo: float                        # the masked 1st and 99th percentile: the range of the 256 bins
    hi: float
    degenerate: bool                 # hi == lo, or the range is not finite (an empty mask): every bin is 0


# ---------------------------------------------------------------- checks shared by both paths

def _check_options(classes, beta, iterations):
    K = check_classes(classes)
    try:
        b = float(beta)
    except (TypeError, ValueError):
        b = float("nan")
    if not 0.0 <= b <= MAX_BETA:
        raise ValueError(f"beta must be a number in [0, {MAX_BETA:g}], got {beta!r}")
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or not 0 <= iterations <= MAX_ITERATIONS:
        raise ValueError(f"iterations must be an integer in 0..{MAX_ITERATIONS}, got {iterations!r}")
    return K, int(np.rint(b * (1 << COST_SHIFT))), int(iterations)


def _range_scale(lo, hi):
    """-> (float32 scale, degenerate): ``scale = float32(256) / (hi - lo)``, one rounded float32 operation each."""
    f32 = np.float32
    lo, hi = f32(lo), f32(hi)
    with np.errstate(all="ignore"):
        width = f32(hi - lo)
        scale = f32(f32(256) / width) if width != 0 else f32(np.inf)
    degenerate = bool(hi == lo or not np.isfinite(width) or not np.isfinite(scale))
    return scale, degenerate


# ---------------------------------------------------------------- numpy specification

def quantise_np(vol, lo, hi) -> np.ndarray:
    """uint8, the shape of ``vol``: ``q = clip(int((v - lo) * scale), 0, 255)`` with ``scale = float32(256) / (hi - lo)``, every
    operation one rounded float32 operation, the conversion truncating: ``otsu_bin`` of ``csrc/volume_mask.hip`` clamped on both
    sides, because values lie outside ``[lo, hi]`` here.  ``hi == lo``, or a width or a scale that is not finite: zeros."""
    vol = np.asarray(vol)
    if vol.dtype != np.float32:
        raise ValueError(f"quantise_np: expected a float32 array, got {vol.dtype}")
    scale, degenerate = _range_scale(lo, hi)
    if degenerate:
        return np.zeros(vol.shape, dtype=np.uint8)
    with np.errstate(all="ignore"):
        pos = (vol - np.float32(lo)) * scale                     # float32 array operations: each rounds to float32
    return np.clip(np.trunc(pos), 0, BINS - 1).astype(np.uint8)


def _assign_bins(centres) -> np.ndarray:
    """-> the cluster 0..K-1 of each of the 256 bins: boundaries at the midpoints of neighbouring centres, a bin on a boundary goes
    to the lower cluster."""
    mids = (centres[:-1] + centres[1:]) / 2.0
    return np.searchsorted(mids, np.arange(BINS, dtype=np.float64), side="left")


def kmeans_hist_np(counts256, K) -> np.ndarray:
    """float64 (K,), ascending: Lloyd's k-means on a 256-bin histogram.  The centres start at the bins that hold the quantiles
    (2k + 1) / (2K) of the counts (the smallest bin b with 2K cum[b] >= (2k + 1) N, in integers); every round assigns the bins
    (``_assign_bins``) and moves each centre to the mean bin of its cluster, float64 of two exact integer sums; an empty cluster
    keeps its centre.  It stops when no centre changes or after 50 rounds.  An empty histogram: the centres of K equal parts of
    the bin range.  Host-only: the device path calls this function on the downloaded counts."""
    K = check_classes(K)
    counts = np.asarray(counts256).astype(np.int64).reshape(-1)
    if counts.size != BINS or (counts < 0).any():
        raise ValueError(f"kmeans_hist_np: expected {BINS} non-negative counts, got {counts.shape}")
    N = int(counts.sum())
    if N == 0:
        return (np.arange(K, dtype=np.float64) + 0.5) * (BINS / K) - 0.5
    cum = np.cumsum(counts)
    centres = np.array([np.searchsorted(cum * (2 * K), (2 * k + 1) * N, side="left") for k in range(K)], dtype=np.float64)
    bins = np.arange(BINS, dtype=np.int64)
    for _ in range(KMEANS_ROUNDS):
        member = _assign_bins(centres)
        new = centres.copy()
        for k in range(K):
            sel = member == k
            n = int(counts[sel].sum())
            if n:
                new[k] = float(int((counts[sel] * bins[sel]).sum())) / float(n)
        if np.array_equal(new, centres):
            break
        centres = new
    return centres


def _table_np(means, variances) -> np.ndarray:
    """int32 (K, 256): ``min(int64(rint(((b - mu_k)^2 / (2 var_k) + 0.5 ln var_k - c0) * 2^16)), 2^30)``, ``c0 = min_k 0.5 ln var_k``,
    float64 in this order."""
    b = np.arange(BINS, dtype=np.float64)[None, :]
    mu, var = means[:, None], variances[:, None]
    half_log = 0.5 * np.log(var)
    c0 = half_log.min()
    cost = np.rint(((b - mu) ** 2 / (2.0 * var) + half_log - c0) * float(1 << COST_SHIFT)).astype(np.int64)
    return np.minimum(cost, COST_CAP).astype(np.int32)


def initial_table_np(counts256, K):
    """-> (int32 (K, 256), means, variances): the table before there are labels.  ``means`` = ``kmeans_hist_np``'s centres, every
    variance = the pooled within-cluster variance of that partition, ``sum_b n_b (b - c(b))^2 / N`` in float64, floored at 1/12."""
    counts = np.asarray(counts256).astype(np.int64).reshape(-1)
    centres = kmeans_hist_np(counts, K)
    N = int(counts.sum())
    pooled = MIN_VARIANCE
    if N:
        d = np.arange(BINS, dtype=np.float64) - centres[_assign_bins(centres)]
        pooled = max(float((counts * d * d).sum()) / float(N), MIN_VARIANCE)
    variances = np.full(len(centres), pooled, dtype=np.float64)
    return _table_np(centres, variances), centres, variances


def cost_table_np(joint, prev=None):
    """joint: int64 (K, 256), ``joint[k, b]`` = voxels of class k + 1 in bin b -> (int32 (K, 256), means, variances).  ``n_k``, ``sum b``
    and ``sum b^2`` are exact integers; ``mu_k = sum b / n_k``, ``var_k = max(sum b^2 / n_k - mu_k^2, 1/12)`` in float64.  A class
    with ``n_k == 0`` keeps the mean and variance of ``prev = (means, variances)`` (``ValueError`` without one).  The table: see
    ``_table_np``; it is non-negative and capped at 2^30."""
    joint = np.asarray(joint)
    if joint.ndim != 2 or joint.shape[1] != BINS or not MIN_CLASSES <= joint.shape[0] <= MAX_CLASSES or joint.dtype.kind not in "iu":
        raise ValueError(f"cost_table_np: expected integer counts of shape (K, {BINS}), K in {MIN_CLASSES}..{MAX_CLASSES}, got "
                         f"{joint.dtype} {joint.shape}")
    K = joint.shape[0]
    means, variances = np.empty(K, dtype=np.float64), np.empty(K, dtype=np.float64)
    for k in range(K):
        row = [int(c) for c in joint[k]]
        n = sum(row)
        if n == 0:
            if prev is None:
                raise ValueError(f"cost_table_np: class {k + 1} is empty and there are no previous parameters to keep")
            means[k], variances[k] = float(prev[0][k]), float(prev[1][k])
            continue
        s1, s2 = sum(b * c for b, c in enumerate(row)), sum(b * b * c for b, c in enumerate(row))
        mu = float(s1) / float(n)
        means[k], variances[k] = mu, max(float(s2) / float(n) - mu * mu, MIN_VARIANCE)
    return _table_np(means, variances), means, variances


def _check_sweep_np(q, mask, labels, cost, beta_q):
    q = u8_np(q, None, "q")
    if q.ndim != 3:
        raise ValueError(f"q must be a volume (X, Y, Z), got {q.shape}")
    mask, labels = u8_np(mask, q.shape, "the mask"), u8_np(labels, q.shape, "the labels")
    cost = np.asarray(cost)
    if cost.dtype != np.int32 or cost.ndim != 2 or cost.shape[1] != BINS or not MIN_CLASSES <= cost.shape[0] <= MAX_CLASSES \
            or cost.min() < 0 or cost.max() > COST_CAP:
        raise ValueError(f"the cost table is int32 (K, {BINS}) with entries in 0..2^30, got {cost.dtype} {cost.shape}")
    if not 0 <= int(beta_q) <= int(MAX_BETA) << COST_SHIFT:
        raise ValueError(f"beta_q must be in 0..{int(MAX_BETA) << COST_SHIFT}, got {beta_q}")
    if ((labels != 0) != (mask != 0)).any() or labels.max() > cost.shape[0]:
        raise ValueError("the labels must be 1..K inside the mask and 0 outside it")
    return q, mask, labels, cost, np.int32(beta_q)


def _neighbour_labels(labels):
    """The 6 face neighbours' labels of every voxel, 0 past a face of the volume."""
    p = np.pad(labels, 1)
    X, Y, Z = labels.shape
    return [p[0:X, 1:-1, 1:-1], p[2:X + 2, 1:-1, 1:-1], p[1:-1, 0:Y, 1:-1], p[1:-1, 2:Y + 2, 1:-1], p[1:-1, 1:-1, 0:Z], p[1:-1, 1:-1, 2:Z + 2]]


def _icm_half(q, labels, cost, beta_q, colour):
    X, Y, Z = q.shape
    i, j, k = np.ogrid[0:X, 0:Y, 0:Z]
    update = (labels != 0) & (((i + j + k) & 1) == colour)
    nb = _neighbour_labels(labels)
    nonzero = np.zeros(q.shape, dtype=np.int32)
    for n in nb:
        nonzero += n != 0
    best = np.zeros(q.shape, dtype=np.uint8)
    best_e = np.full(q.shape, np.iinfo(np.int32).max, dtype=np.int32)
    for c in range(cost.shape[0]):
        same = np.zeros(q.shape, dtype=np.int32)
        for n in nb:
            same += n == c + 1
        e = cost[c][q] + beta_q * (nonzero - same)              # int32: at most 2^30 + 6 * 2^20
        better = e < best_e                                      # a tie stays with the smaller class
        best[better], best_e[better] = c + 1, e[better]
    out = labels.copy()
    out[update] = best[update]
    return out


def icm_half_np(q, mask, labels, cost, beta_q, colour) -> np.ndarray:
    """One half-sweep: every voxel inside the mask with ``(i + j + k) & 1 == colour`` takes the class k + 1 of the smallest
    ``cost[k, q] + beta_q * d_k``, ties to the smallest k; ``d_k`` = the number of its 6 face neighbours that lie inside the volume,
    have a non-zero label and a label other than k + 1.  int32 arithmetic.  Its neighbours all have the other colour, so the order
    inside a half-sweep does not matter.  -> the new labels (a copy)."""
    if colour not in (0, 1):
        raise ValueError(f"colour is 0 or 1, got {colour!r}")
    q, mask, labels, cost, beta_q = _check_sweep_np(q, mask, labels, cost, beta_q)
    return _icm_half(q, labels, cost, beta_q, colour)


def icm_sweep_np(q, mask, labels, cost, beta_q):
    """-> (labels, changed): ``icm_half_np`` for colour 0, then for colour 1; ``changed`` = the voxels whose label differs after
    the two from before them.  The labels are 1..K inside the mask and 0 outside it, before and after."""
    q, mask, labels, cost, beta_q = _check_sweep_np(q, mask, labels, cost, beta_q)
    out = _icm_half(q, _icm_half(q, labels, cost, beta_q, 0), cost, beta_q, 1)
    return out, int((out != labels).sum())


def energy_np(q, mask, labels, cost, beta_q) -> int:
    """The Potts energy as a Python integer: the sum of ``cost[label - 1, q]`` over the mask plus ``beta_q`` times the number of
    unordered pairs of face neighbours inside the mask with different labels.  A half-sweep never raises it."""
    q, mask, labels, cost, beta_q = _check_sweep_np(q, mask, labels, cost, beta_q)
    inside = labels != 0
    data = int(cost[labels[inside].astype(np.int64) - 1, q[inside]].astype(np.int64).sum())
    pairs = 0
    for axis in range(3):
        a, b = np.moveaxis(labels, axis, 0)[:-1], np.moveaxis(labels, axis, 0)[1:]
        pairs += int(((a != 0) & (b != 0) & (a != b)).sum())
    return data + int(beta_q) * pairs


def joint_hist_np(q, labels, K) -> np.ndarray:
    """int64 (K, 256): voxels of class k + 1 in bin b; label 0 (and any label above K) is not counted."""
    q, labels = np.asarray(q).reshape(-1), np.asarray(labels).reshape(-1)
    sel = (labels >= 1) & (labels <= K)
    cell = (labels[sel].astype(np.int64) - 1) * BINS + q[sel]
    return np.bincount(cell, minlength=K * BINS).astype(np.int64).reshape(K, BINS)


class _NumpyBackend:
    """The steps of ``_drive`` in numpy."""

    def __init__(self, vol, mask, K):
        self.vol, self.mask, self.K = vol, mask, K

    def quantise(self):
        marks, _ = landmarks_np(self.vol, self.mask, RANGE)
        lo, hi = float(marks[0]), float(marks[1])
        self.q = quantise_np(self.vol, lo, hi)
        self.labels = (self.mask != 0).astype(np.uint8)
        counts = np.bincount(self.q[self.mask != 0].reshape(-1), minlength=BINS).astype(np.int64)
        return lo, hi, counts

    def sweep(self, cost, beta_q):
        self.labels, changed = icm_sweep_np(self.q, self.mask, self.labels, cost, beta_q)
        return changed, joint_hist_np(self.q, self.labels, self.K)


def _drive(backend, K, beta_q, iterations) -> TissueSegmentation:
    """The loop both paths run; ``backend`` does what touches voxels.  The range and the 256 counts; k-means and the first table; the
    labels 1 inside the mask, then one sweep with beta_q = 0: maximum likelihood.  Then up to ``iterations`` times: the table of
    the labels' joint histogram, one sweep; ``changed == 0`` ends the loop.  The parameters returned are those of the final labels."""
    lo, hi, counts = backend.quantise()
    scale, degenerate = _range_scale(lo, hi)
    cost, means, variances = initial_table_np(counts, K)
    changed, joint = backend.sweep(cost, 0)
    sweeps = 0
    for _ in range(iterations):
        cost, means, variances = cost_table_np(joint, (means, variances))
        changed, joint = backend.sweep(cost, beta_q)
        sweeps += 1
        if changed == 0:
            break
    _, means, variances = cost_table_np(joint, (means, variances))
    if degenerate:
        m, v = np.full(K, lo, dtype=np.float64), np.zeros(K, dtype=np.float64)
    else:
        m, v = lo + (means + 0.5) / float(scale), variances / (float(scale) * float(scale))
    return TissueSegmentation(backend.labels, m, v, joint.sum(axis=1).astype(np.int64), sweeps, int(changed), lo, hi, degenerate)


def segment_tissue_np(vol, mask, classes=3, beta=1.0, iterations=20) -> TissueSegmentation:
    """The specification of ``segment_tissue``: ``vol`` a finite float32 volume (X, Y, Z), ``mask`` uint8 (non-zero = inside),
    ``classes`` K in 2..6, ``beta`` in [0, 16] (``beta_q = rint(beta * 2^16)``), ``iterations`` in 0..100; see ``_drive``.  The range
    of the bins is the masked 1st and 99th percentile (``volume_intensity.landmarks_np``).  ``iterations = 0`` returns the
    maximum-likelihood labels.  Nothing raises for a constant foreground or an empty mask: ``degenerate`` is set."""
    K, beta_q, T = _check_options(classes, beta, iterations)
    vol = volume_np(vol, "segment_tissue_np")
    mask = u8_np(mask, vol.shape, "the mask")
    return _drive(_NumpyBackend(vol, mask, K), K, beta_q, T)


def confusion_np(a, b, mask=None, classes=3) -> np.ndarray:
    """int64 (K + 1, K + 1): ``conf[i, j]`` = the voxels (inside ``mask``, when given) with ``a == i`` and ``b == j``.  A label above
    K among them is refused (``ValueError``)."""
    K = check_classes(classes)
    a = u8_np(a, None, "a")
    b = u8_np(b, a.shape, "b")
    if mask is not None:
        sel = u8_np(mask, a.shape, "the mask") != 0
        a, b = a[sel], b[sel]
    a, b = a.reshape(-1).astype(np.int64), b.reshape(-1).astype(np.int64)
    bad = int(((a > K) | (b > K)).sum())
    if bad:
        raise ValueError(f"{bad} voxel(s) carry a label above {K}")
    return np.bincount(a * (K + 1) + b, minlength=(K + 1) ** 2).astype(np.int64).reshape(K + 1, K + 1)


def dice_np(conf) -> np.ndarray:
    """float64 (K,): ``2 n_kk / (row_k + col_k)`` for k = 1..K of a confusion matrix; NaN where a class is absent from both."""
    conf = np.asarray(conf)
    if conf.ndim != 2 or conf.shape[0] != conf.shape[1] or conf.shape[0] < 2 or conf.dtype.kind not in "iu":
        raise ValueError(f"dice_np: expected a square integer confusion matrix, got {conf.dtype} {conf.shape}")
    c = conf.astype(np.float64)
    den = c.sum(axis=1)[1:] + c.sum(axis=0)[1:]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, 2.0 * np.diagonal(c)[1:] / den, np.nan)


# ---------------------------------------------------------------- device

class TissueWorkspace:
    """Every buffer of ``segment_tissue`` for volumes of ``shape`` and ``classes`` classes on ``device``, so that nothing is allocated
    inside the loop; it may serve call after call on one stream.  ``labels`` is the tensor a call returns: the next call with this
    workspace overwrites it."""

    def __init__(self, shape, classes, device):
        K = check_classes(classes)
        shape = tuple(int(d) for d in shape)
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError(f"a volume shape (X, Y, Z) is expected, got {shape}")
        device = cuda_device(device, "TissueWorkspace")
        self.shape, self.classes, self.device = shape, K, device
        self.q = torch.empty(shape, dtype=torch.uint8, device=device)
        self.labels = torch.empty(shape, dtype=torch.uint8, device=device)
        self.percentiles = percentiles_workspace(len(RANGE), device)
        # int64 counters: [0] changed, [1] flags of the quantiser, [2:2 + 256] the masked histogram, then the K x 256 joint histogram
        self.counters = torch.zeros(2 + BINS + K * BINS, dtype=torch.int64, device=device)
        self.cost = torch.empty((K, BINS), dtype=torch.int32, device=device)
        self.host_counters = torch.empty(self.counters.shape, dtype=torch.int64).pin_memory()
        self.host_cost = torch.empty((K, BINS), dtype=torch.int32).pin_memory()

    def download(self) -> np.ndarray:
        self.host_counters.copy_(self.counters, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return self.host_counters.numpy()


def _quantise(vol, mask, range2, q, labels, hist, flags):
    L.call("mrisr_f32_volume_quantise", vol.data_ptr(), mask.data_ptr(), vol.numel(), range2.data_ptr(), q.data_ptr(), L.ptr(labels),
           hist.data_ptr(), flags.data_ptr(), L.stream_ptr(), nbytes=(7 if labels is not None else 6) * vol.numel())


def _joint_hist(q, labels, K, joint):
    L.call("mrisr_u8_volume_joint_hist", q.data_ptr(), labels.data_ptr(), q.numel(), K, joint.data_ptr(), L.stream_ptr(), nbytes=2 * q.numel())


def _icm_half_launch(q, labels, shape, K, cost, beta_q, colour, changed):
    L.call("mrisr_u8_volume_icm_half", q.data_ptr(), labels.data_ptr(), *shape, K, cost.data_ptr(), int(beta_q), int(colour), changed.data_ptr(),
           L.stream_ptr())


class _DeviceBackend:
    """The steps of ``_drive`` on the device; every host read goes through ``TissueWorkspace.download``."""

    def __init__(self, vol, mask, K, ws):
        self.vol, self.mask, self.K, self.ws = vol, mask, K, ws
        self.labels = ws.labels

    def quantise(self):
        ws = self.ws
        marks, _ = masked_percentiles(self.vol, self.mask, RANGE, ws.percentiles)
        ws.counters.zero_()
        _quantise(self.vol, self.mask, marks, ws.q, ws.labels, ws.counters[2:2 + BINS], ws.counters[1:2])
        host = ws.download()
        lo, hi = (float(x) for x in marks.cpu().numpy())
        return lo, hi, host[2:2 + BINS].copy()

    def sweep(self, cost, beta_q):
        ws, K = self.ws, self.K
        ws.host_cost.copy_(torch.from_numpy(cost))
        ws.cost.copy_(ws.host_cost, non_blocking=True)          # the download below ends in a synchronisation: the host copy is free again
        ws.counters.zero_()
        joint = ws.counters[2 + BINS:]
        for colour in (0, 1):
            _icm_half_launch(ws.q, ws.labels, ws.shape, K, ws.cost, beta_q, colour, ws.counters[0:1])
        _joint_hist(ws.q, ws.labels, K, joint)
        host = ws.download()
        return int(host[0]), host[2 + BINS:].reshape(K, BINS).copy()


def segment_tissue(vol: torch.Tensor, mask: torch.Tensor, classes=3, beta=1.0, iterations=20, workspace=None) -> TissueSegmentation:
    """The device path of ``segment_tissue_np``, the same contract: ``vol`` a contiguous float32 CUDA volume (X, Y, Z), ``mask`` a uint8
    or bool CUDA tensor of its shape -> ``TissueSegmentation`` with ``labels`` a uint8 CUDA tensor and host numbers for the rest,
    every field equal to the specification's.  ``workspace``: a ``TissueWorkspace`` of this shape and class count (its ``labels`` is
    returned).  Per iteration: three launches, one download of at most 12 KB and one upload of at most 6 KB (module docstring)."""
    K, beta_q, T = _check_options(classes, beta, iterations)
    v = cuda_tensor(vol, (torch.float32,), "segment_tissue", ndim=3)
    if mask is None:
        raise ValueError("segment_tissue: a mask is required (volume_eval.foreground_mask gives one)")
    m = mask_tensor(mask, v.shape, "segment_tissue")
    ws = TissueWorkspace(v.shape, K, v.device) if workspace is None else workspace
    if not isinstance(ws, TissueWorkspace) or ws.shape != tuple(v.shape) or ws.classes != K or ws.device != v.device:
        raise ValueError(f"the workspace must be a TissueWorkspace({tuple(v.shape)}, {K}, {v.device})")
    return _drive(_DeviceBackend(v, m, K, ws), K, beta_q, T)


def label_confusion(a: torch.Tensor, b: torch.Tensor, mask=None, classes=3) -> np.ndarray:
    """The device form of ``confusion_np``: ``a``, ``b`` contiguous uint8 CUDA tensors of one shape, ``mask`` a uint8 or bool CUDA tensor
    of that shape or None -> the int64 (K + 1, K + 1) matrix on the host (one launch, one download of at most 400 bytes).  A label
    above K inside the mask is counted by the kernel, not tallied, and raises ``ValueError`` here."""
    K = check_classes(classes)
    a = cuda_tensor(a, (torch.uint8,), "label_confusion")
    b = cuda_tensor(b, (torch.uint8,), "label_confusion", shape=a.shape)
    m = None if mask is None else mask_tensor(mask, a.shape, "label_confusion")
    cells = (K + 1) ** 2
    conf = torch.zeros(cells + 1, dtype=torch.int64, device=a.device)
    L.call("mrisr_u8_volume_confusion", a.data_ptr(), b.data_ptr(), L.ptr(m), a.numel(), K, conf.data_ptr(), L.stream_ptr(),
           nbytes=(3 if m is not None else 2) * a.numel())
    host = conf.cpu().numpy()
    if host[cells]:
        raise ValueError(f"{int(host[cells])} voxel(s) carry a label above {K}")
    return host[:cells].reshape(K + 1, K + 1).copy()


dice = dice_np      # the device path's name: a confusion matrix is on the host in both paths
