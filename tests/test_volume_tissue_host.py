"""CPU-only tests of the tissue classification (mri_superresolution_amd/volume_tissue.py, numpy part): the quantiser, k-means on a
histogram, the cost table, the checkerboard sweep and its energy, the driver, the quality on a phantom, the confusion matrix and
Dice, and the C entries' argument checks."""
import numpy as np
import pytest

import tissueutil as U
from mri_superresolution_amd import volume_tissue as T

# Dice against the truth on the phantom (sigma 60, K = 3, beta = 1, 20 iterations), measured once with this specification on the
# CPU and recorded in DESIGN.md section 7; asserted with a margin of a quarter of 1 - Dice
PHANTOM_DICE = (0.99788157, 0.99219766, 0.98680739)


# ---------------------------------------------------------------- quantise_np

def test_quantise_at_and_around_the_range_and_for_negative_values():
    lo, hi = np.float32(-10.0), np.float32(54.0)                     # scale = 4 exactly
    below, above = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(lo, np.float32(np.inf))
    under_hi, over_hi = np.nextafter(hi, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
    v = np.array([lo, hi, below, above, under_hi, over_hi, -1e30, 1e30, -10.25, -9.75, -9.7, 0.0, 53.74, 53.75], dtype=np.float32)
    q = T.quantise_np(v, lo, hi)
    assert q.dtype == np.uint8
    assert q.tolist() == [0, 255, 0, 0, 255, 255, 0, 255, 0, 1, 1, 40, 254, 255]
    # the wording: one rounded float32 operation each, then truncation
    rng = np.random.default_rng(3)
    w = rng.normal(0, 300, 5000).astype(np.float32)
    lo, hi = np.float32(-411.3), np.float32(397.9)
    scale = np.float32(256) / np.float32(hi - lo)
    want = [min(255, max(0, int(np.float32(np.float32(x - lo) * scale)))) for x in w]
    assert T.quantise_np(w, lo, hi).tolist() == want


@pytest.mark.parametrize("lo, hi", [(5.0, 5.0), (np.nan, np.nan), (-3e38, 3e38), (0.0, 1e-44)])
def test_degenerate_range_gives_zeros_and_sets_the_flag(lo, hi):
    v = U.noisy_volume((3, 4, 5), 1)
    assert not T.quantise_np(v, lo, hi).any()
    assert T._range_scale(lo, hi)[1]
    assert not T._range_scale(0.0, 255.0)[1]


def test_constant_foreground_and_empty_mask_do_not_raise():
    v = np.full((4, 5, 6), 7.0, dtype=np.float32)
    s = T.segment_tissue_np(v, np.ones(v.shape, np.uint8), 3, 1.0, 5)
    assert s.degenerate and (s.labels == 1).all() and s.counts.tolist() == [v.size, 0, 0] and s.lo == s.hi == 7.0
    s = T.segment_tissue_np(U.noisy_volume((4, 5, 6), 2), np.zeros(v.shape, np.uint8), 2, 1.0, 5)
    assert s.degenerate and not s.labels.any() and s.counts.tolist() == [0, 0] and s.changed == 0


# ---------------------------------------------------------------- kmeans_hist_np

def test_kmeans_finds_three_spikes_exactly():
    counts = np.zeros(256, dtype=np.int64)
    counts[[20, 100, 200]] = (500, 300, 400)
    assert T.kmeans_hist_np(counts, 3).tolist() == [20.0, 100.0, 200.0]


def test_kmeans_empty_cluster_keeps_its_centre_and_centres_ascend():
    counts = np.zeros(256, dtype=np.int64)
    counts[40] = 1000                                                # every quantile lies in bin 40: two clusters stay empty
    c = T.kmeans_hist_np(counts, 3)
    assert c.tolist() == [40.0, 40.0, 40.0]
    counts[200] = 10
    c = T.kmeans_hist_np(counts, 3)
    assert c[0] == 40.0 and (np.diff(c) >= 0).all()
    assert T.kmeans_hist_np(np.zeros(256, dtype=np.int64), 4).tolist() == [31.5, 95.5, 159.5, 223.5]


@pytest.mark.parametrize("K", [2, 6])
def test_kmeans_for_two_and_six_classes(K):
    rng = np.random.default_rng(K)
    modes = np.linspace(20, 235, K)
    counts = np.bincount(np.clip(np.rint(np.concatenate([rng.normal(m, 4, 2000) for m in modes])), 0, 255).astype(np.int64), minlength=256)
    c = T.kmeans_hist_np(counts, K)
    assert c.shape == (K,) and c.dtype == np.float64 and (np.diff(c) > 0).all()
    assert np.abs(c - modes).max() < 1.0
    # a fixed point: every centre is the mean bin of its cluster
    member = T._assign_bins(c)
    bins = np.arange(256)
    assert [float((counts * bins)[member == k].sum()) / float(counts[member == k].sum()) for k in range(K)] == c.tolist()
    for bad in (1, 7, 2.0, True):
        with pytest.raises(ValueError, match="classes"):
            T.kmeans_hist_np(counts, bad)


# ---------------------------------------------------------------- cost_table_np

def test_cost_table_parameters_cap_sign_and_empty_class():
    joint = np.zeros((3, 256), dtype=np.int64)
    joint[0, [10, 12]] = (5, 5)                                      # mean 11, variance 1
    joint[2, 250] = 9                                                # variance 0 -> 1/12; class 2 is empty
    with pytest.raises(ValueError, match="class 2 is empty"):
        T.cost_table_np(joint)
    prev = (np.array([1.0, 77.0, 3.0]), np.array([4.0, 25.0, 6.0]))
    cost, means, variances = T.cost_table_np(joint, prev)
    assert means.tolist() == [11.0, 77.0, 250.0] and variances.tolist() == [1.0, 25.0, 1.0 / 12.0]
    assert cost.dtype == np.int32 and cost.shape == (3, 256) and cost.min() >= 0 and cost.max() == 1 << 30
    assert cost[2, 0] == 1 << 30                                      # 250^2 * 6 * 2^16 is far above the cap
    assert cost[2, 250] == 0                                          # the smallest half log-variance is the offset
    b = np.arange(256, dtype=np.float64)
    want = np.rint(((b - 11.0) ** 2 / 2.0 + 0.5 * np.log(1.0) - 0.5 * np.log(1.0 / 12.0)) * 65536.0)
    assert cost[0].tolist() == np.minimum(want, 1 << 30).astype(np.int64).tolist()


def test_initial_table_uses_the_centres_and_the_pooled_variance():
    counts = np.zeros(256, dtype=np.int64)
    counts[[20, 22, 100, 200]] = (100, 100, 300, 400)
    cost, means, variances = T.initial_table_np(counts, 3)
    assert means.tolist() == [21.0, 100.0, 200.0]
    assert variances.tolist() == [200.0 / 900.0] * 3
    assert (cost.argmin(axis=0)[[0, 21, 60, 61, 149, 151, 255]] == [0, 0, 0, 1, 1, 2, 2]).all()
    _, _, variances = T.initial_table_np(np.bincount([50, 90], minlength=256), 2)
    assert variances.tolist() == [1.0 / 12.0] * 2                     # floored


def test_one_sweep_without_beta_is_the_argmin_of_the_table():
    q, mask, labels, cost = U.sweep_problem((5, 6, 7), 4, 11)
    out, changed = T.icm_sweep_np(q, mask, labels, cost, 0)
    want = np.where(mask != 0, cost.argmin(axis=0)[q] + 1, 0)
    assert (out == want).all() and changed == int((want != labels).sum())
    assert not out[mask == 0].any()                                   # labels outside the mask stay 0


# ---------------------------------------------------------------- the sweep and its energy

def _energies_along(q, mask, labels, cost, beta_q, sweeps):
    e = [T.energy_np(q, mask, labels, cost, beta_q)]
    for _ in range(sweeps):
        for colour in (0, 1):
            labels = T.icm_half_np(q, mask, labels, cost, beta_q, colour)
            e.append(T.energy_np(q, mask, labels, cost, beta_q))
    return e, labels


def test_energy_never_rises_on_random_cases():
    for seed in range(200):
        K = 2 + seed % 5
        beta_q = (0, 1, 40000, 65536, 300000, 16 << 16)[seed % 6]
        q, mask, labels, cost = U.sweep_problem((5, 6, 7), K, seed, ("random", "ones")[seed % 2])
        if seed % 3 == 0:
            cost = (cost >> 6).astype(np.int32)                      # costs of the size of beta_q: the prior decides
        e, _ = _energies_along(q, mask, labels, cost, beta_q, 2)
        assert all(b <= a for a, b in zip(e, e[1:])), (seed, e)
        assert all(isinstance(x, int) for x in e)


def test_energy_never_rises_on_the_phantom_and_counts_pairs():
    vol, mask, truth = U.phantom()
    lo, hi = (float(x) for x in T.landmarks_np(vol, mask, T.RANGE)[0])
    q = T.quantise_np(vol, lo, hi)
    cost, _, _ = T.initial_table_np(np.bincount(q[mask != 0], minlength=256), 3)
    labels, _ = T.icm_sweep_np(q, mask, mask.copy(), cost, 0)
    e, labels = _energies_along(q, mask, labels, cost, 65536, 3)
    assert all(b <= a for a, b in zip(e, e[1:])) and e[-1] < e[0]
    # the definition, on a tiny case by hand: two voxels inside, different labels, one pair
    q2 = np.array([[[3, 4, 5]]], dtype=np.uint8)
    m2 = np.array([[[1, 1, 0]]], dtype=np.uint8)
    l2 = np.array([[[1, 2, 0]]], dtype=np.uint8)
    c2 = np.arange(512, dtype=np.int32).reshape(2, 256)
    assert T.energy_np(q2, m2, l2, c2, 1000) == 3 + (256 + 4) + 1000
    assert T.energy_np(q2, m2, np.array([[[2, 2, 0]]], dtype=np.uint8), c2, 1000) == (256 + 3) + (256 + 4)


def test_isolated_voxel_follows_the_table_and_neighbours_pull():
    cost = np.zeros((2, 256), dtype=np.int32)
    cost[0, :] = 100                                                  # class 2 is cheaper by 100 everywhere
    q = np.zeros((3, 3, 3), dtype=np.uint8)
    mask = np.zeros((3, 3, 3), dtype=np.uint8)
    mask[1, 1, 1] = 1
    labels = mask.copy()
    out, changed = T.icm_sweep_np(q, mask, labels, cost, 16 << 16)
    assert out[1, 1, 1] == 2 and changed == 1 and out.sum() == 2      # no neighbour inside the mask: the table alone
    mask[0, 1, 1] = mask[1, 0, 1] = 1                                 # two neighbours of class 1
    labels = mask.copy()
    out = T.icm_half_np(q, mask, labels, cost, 49, 1)                 # (1, 1, 1) has colour 1: 0 + 2 * 49 < 100 -> class 2
    assert out[1, 1, 1] == 2 and out[0, 1, 1] == 1
    out = T.icm_half_np(q, mask, labels, cost, 50, 1)                 # 0 + 2 * 50 == 100: the tie goes to the smaller class
    assert out[1, 1, 1] == 1
    out = T.icm_half_np(q, mask, labels, cost, 50, 0)                 # the two others (colour 0) pay 100 + 0 against 0 + 50
    assert out[0, 1, 1] == out[1, 0, 1] == 2 and out[1, 1, 1] == 1
    assert (T.icm_half_np(q, mask, labels, cost, 101, 0) == labels).all()      # 100 + 0 against 0 + 101
    with pytest.raises(ValueError, match="inside the mask"):
        T.icm_sweep_np(q, mask, np.zeros_like(mask), cost, 0)
    with pytest.raises(ValueError, match="colour"):
        T.icm_half_np(q, mask, labels, cost, 0, 2)


# ---------------------------------------------------------------- the driver

def test_zero_iterations_return_the_maximum_likelihood_labels_and_no_change_ends_the_loop():
    vol, mask, _ = U.phantom()
    s = T.segment_tissue_np(vol, mask, 3, 1.0, 0)
    q = T.quantise_np(vol, s.lo, s.hi)
    cost, _, _ = T.initial_table_np(np.bincount(q[mask != 0], minlength=256), 3)
    assert s.sweeps == 0 and (s.labels == np.where(mask != 0, cost.argmin(axis=0)[q] + 1, 0)).all()
    assert s.counts.tolist() == np.bincount(s.labels.reshape(-1), minlength=4)[1:].tolist()
    full = T.segment_tissue_np(vol, mask, 3, 1.0, 100)
    assert full.changed == 0 and 0 < full.sweeps < 100
    again = T.segment_tissue_np(vol, mask, 3, 1.0, full.sweeps)
    assert (again.labels == full.labels).all() and again.sweeps == full.sweeps
    short = T.segment_tissue_np(vol, mask, 3, 1.0, 1)
    assert short.sweeps == 1 and short.changed > 0
    assert (np.diff(full.means) > 0).all() and full.labels.dtype == np.uint8 and not full.degenerate
    for bad in (dict(classes=1), dict(classes=7), dict(beta=-0.1), dict(beta=16.5), dict(beta="x"), dict(iterations=101), dict(iterations=1.0)):
        with pytest.raises(ValueError):
            T.segment_tissue_np(vol, mask, **bad)


def test_quality_on_the_phantom():
    vol, mask, truth = U.phantom()
    with_prior = T.dice_np(T.confusion_np(T.segment_tissue_np(vol, mask, 3, 1.0, 20).labels, truth, mask, 3))
    without = T.dice_np(T.confusion_np(T.segment_tissue_np(vol, mask, 3, 0.0, 20).labels, truth, mask, 3))
    print(f"phantom sigma {U.PHANTOM_SIGMA:g}: Dice beta = 1 {with_prior.tolist()}, beta = 0 {without.tolist()}")
    for k in range(3):
        assert with_prior[k] > without[k]
        assert with_prior[k] >= PHANTOM_DICE[k] - 0.25 * (1.0 - PHANTOM_DICE[k])


# ---------------------------------------------------------------- confusion_np, dice_np

def test_confusion_and_dice():
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 4, (6, 7, 8), dtype=np.uint8), rng.integers(0, 4, (6, 7, 8), dtype=np.uint8)
    mask = (rng.random(a.shape) < 0.6).astype(np.uint8)
    for m in (None, mask):
        conf = T.confusion_np(a, b, m, 3)
        sel = np.ones(a.shape, bool) if m is None else m != 0
        assert conf.dtype == np.int64 and conf.shape == (4, 4)
        assert conf.sum(axis=1).tolist() == np.bincount(a[sel], minlength=4).tolist()
        assert conf.sum(axis=0).tolist() == np.bincount(b[sel], minlength=4).tolist()
        assert conf[2, 1] == int(((a == 2) & (b == 1) & sel).sum())
    assert T.dice_np(T.confusion_np(a, a, None, 3)).tolist() == [1.0, 1.0, 1.0]
    c = np.where(a == 0, 0, a % 3 + 1).astype(np.uint8)              # every class moved to another: disjoint
    assert T.dice_np(T.confusion_np(a, c, None, 3)).tolist() == [0.0, 0.0, 0.0]
    d = T.dice_np(T.confusion_np(np.minimum(a, 2), np.minimum(a, 2), None, 3))
    assert d[:2].tolist() == [1.0, 1.0] and np.isnan(d[2])           # class 3 is absent from both
    assert T.dice_np(np.array([[0, 0, 0], [0, 3, 1], [0, 2, 4]])).tolist() == [6.0 / 9.0, 8.0 / 11.0]
    assert T.dice is T.dice_np
    a[0, 0, 0] = 4
    with pytest.raises(ValueError, match="label above 3"):
        T.confusion_np(a, b, None, 3)
    assert T.confusion_np(a, b, None, 4).shape == (5, 5)
    hidden = np.ones(a.shape, np.uint8)
    hidden[0, 0, 0] = 0
    assert T.confusion_np(a, b, hidden, 3).sum() == a.size - 1       # outside the mask nothing is examined


def test_device_entries_refuse_cpu_tensors():
    import torch
    vol, mask, _ = U.phantom(shape=(4, 5, 6))
    v, m = torch.from_numpy(vol.copy()), torch.from_numpy(mask.copy())
    for call in (lambda: T.segment_tissue(v, m), lambda: T.label_confusion(m, m), lambda: T.TissueWorkspace(v.shape, 3, "cpu")):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()


# ---------------------------------------------------------------- the C side, without a GPU

def test_library_declares_the_entry_points_and_checks_their_arguments():
    import ctypes
    import os
    from mri_superresolution_amd import _lib
    lib = _lib.load()
    names = ("mrisr_f32_volume_quantise", "mrisr_u8_volume_joint_hist", "mrisr_u8_volume_icm_half", "mrisr_u8_volume_confusion")
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mrisr.h")) as f:
        header = f.read()
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and f"int {name}(" in header
    assert lib.mrisr_version() == _lib.ABI_VERSION >= 323
    ARG, SHAPE = -1, -2
    buf = (ctypes.c_uint64 * 64)()                       # host memory: nothing is launched when a check fails
    p = ctypes.addressof(buf)
    q, r, w = p + 64, p + 128, p + 256
    assert lib.mrisr_f32_volume_quantise(None, q, 4, p, r, None, w, w + 8, None) == ARG
    assert lib.mrisr_f32_volume_quantise(p, q, 4, p, r, None, None, w + 8, None) == ARG
    assert lib.mrisr_f32_volume_quantise(p, q, 4, p, r, None, w + 4, w + 8, None) == ARG           # misaligned counters
    assert lib.mrisr_f32_volume_quantise(p, q, 4, p, q, None, w, w + 8, None) == ARG               # q_out is the mask
    assert b"of their own" in lib.mrisr_last_error()
    assert lib.mrisr_f32_volume_quantise(p, q, 0, p, r, None, w, w + 8, None) == SHAPE
    assert lib.mrisr_f32_volume_quantise(p, q, 1 << 32, p, r, None, w, w + 8, None) == SHAPE
    assert lib.mrisr_u8_volume_joint_hist(None, q, 4, 3, w, None) == ARG
    assert lib.mrisr_u8_volume_joint_hist(p, q, 4, 1, w, None) == ARG
    assert lib.mrisr_u8_volume_joint_hist(p, q, 4, 7, w, None) == ARG
    assert b"classes" in lib.mrisr_last_error()
    assert lib.mrisr_u8_volume_joint_hist(p, q, 0, 3, w, None) == SHAPE
    assert lib.mrisr_u8_volume_icm_half(p, None, 1, 1, 1, 3, r, 0, 0, w, None) == ARG
    assert lib.mrisr_u8_volume_icm_half(p, p, 1, 1, 1, 3, r, 0, 0, w, None) == ARG
    assert lib.mrisr_u8_volume_icm_half(p, q, 1, 1, 1, 3, r + 2, 0, 0, w, None) == ARG
    assert lib.mrisr_u8_volume_icm_half(p, q, 1, 1, 1, 8, r, 0, 0, w, None) == ARG
    assert lib.mrisr_u8_volume_icm_half(p, q, 1, 1, 1, 3, r, -1, 0, w, None) == ARG
    assert lib.mrisr_u8_volume_icm_half(p, q, 1, 1, 1, 3, r, (16 << 16) + 1, 0, w, None) == ARG
    assert b"beta_q" in lib.mrisr_last_error()
    assert lib.mrisr_u8_volume_icm_half(p, q, 1, 1, 1, 3, r, 0, 2, w, None) == ARG
    assert lib.mrisr_u8_volume_icm_half(p, q, 1, 0, 1, 3, r, 0, 0, w, None) == SHAPE
    assert lib.mrisr_u8_volume_icm_half(p, q, 1, 1, 32768, 3, r, 0, 0, w, None) == SHAPE
    assert lib.mrisr_u8_volume_confusion(p, None, None, 4, 3, w, None) == ARG
    assert lib.mrisr_u8_volume_confusion(p, q, None, 4, 3, w + 4, None) == ARG
    assert lib.mrisr_u8_volume_confusion(p, q, None, 4, 0, w, None) == ARG
    assert lib.mrisr_u8_volume_confusion(p, q, None, 0, 3, w, None) == SHAPE


# ---------------------------------------------------------------- the command lines

def test_command_lines_parse_the_new_options():
    from scripts import evaluate_volume as eval_cli
    from scripts import segment_volume as seg_cli
    args = eval_cli.parse_args(["--reference", "r.nii"])
    assert args.tissue_dice == 0
    assert eval_cli.parse_args(["--reference", "r.nii", "--mask", "otsu", "--tissue_dice", "3"]).tissue_dice == 3
    eval_cli.check_options(None, None, "linear", "header", "none", "none")
    eval_cli.check_options(None, None, "linear", "header", "none", "none", tissue_dice=3, mask="otsu")
    with pytest.raises(ValueError, match="--tissue_dice goes with --mask"):
        eval_cli.check_options(None, None, "linear", "header", "none", "none", tissue_dice=3)
    for bad in (1, 7, -2):
        with pytest.raises(ValueError, match="--tissue_dice is 0"):
            eval_cli.check_options(None, None, "linear", "header", "none", "none", tissue_dice=bad, mask="otsu")
    assert eval_cli.CSV_COLUMNS_MASKED == ["scan", "region", "method", "ssim", "psnr", "mse", "rmse", "mae"]
    assert eval_cli.dice_columns(3) == ["dice_1", "dice_2", "dice_3"] and eval_cli.dice_columns(0) == []
    args = seg_cli.parse_args(["--input", "a.nii", "--output", "b.nii"])
    assert (args.classes, args.beta, args.iterations, args.mask, args.mask_close, args.mask_largest, args.mask_fill_holes, args.compare) == \
        (3, 1.0, 20, "otsu", 0, False, None, None)
    with pytest.raises(SystemExit):
        seg_cli.parse_args(["--input", "a.nii"])
    assert seg_cli.main(seg_cli.parse_args(["--input", "a.nii", "--output", "b.nii", "--cpu"])) == 1
