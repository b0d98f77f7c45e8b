"""Gibbs-ringing removal on the device (csrc/volume_unring.hip): ``unring_axis`` against its numpy specification, bit for bit, at
every launch shape - each bundle width (lines up to 128, 256, 512), a bundle with missing lines, line lengths that are no multiple
of the register block, a chunk that ends inside a thread's outputs, more bundles than one wave of workgroups - then ``out=``, graph
capture, refusals, ``unring`` against its parts assembled by hand and ``kspace_split`` against float64 ``np.fft``.

The candidates of a (shape, axis, K) are formed once on the host (``shifted_lines_np``) and judged per window (``select_np``);
``unring_axis_np`` is exactly that composition (tests/test_unring_host.py)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from mri_superresolution_amd import _lib                    # noqa: E402
from mri_superresolution_amd import volume_unring as U      # noqa: E402

SHAPES = [(8, 8, 8), (9, 11, 13), (8, 1, 70), (33, 17, 65), (5, 3, 512), (512, 1, 8), (8, 512, 3), (40, 40, 40), (129, 8, 130),
          (257, 2, 8)]
SHIFTS = (1, 3, 20)
WINDOWS = ((1, 3), (1, 1), (2, 4))


def values(shape, seed, special=False):
    v = np.random.default_rng(seed).uniform(-3000.0, 3000.0, shape).astype(np.float32)
    if special:
        flat = v.reshape(-1)
        flat[0] = np.nan
        flat[-1] = np.inf
    return v


def same_bits(got, want):
    """Equal uint32 views wherever the specification is a number; NaN exactly where it is NaN."""
    if got.dtype != np.float32 or want.dtype != np.float32 or got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def run(v, axis, K, window, **kw):
    out = U.unring_axis(torch.from_numpy(v).cuda(), axis, K, window, **kw)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == v.shape
    return out.cpu().numpy()


def compare(v, axes, shifts=SHIFTS, windows=WINDOWS):
    for axis in axes:
        for K in shifts:
            shifted = U.shifted_lines_np(v, axis, K)
            for window in windows:
                want = U.select_np(v, shifted, axis, K, window)
                got = run(v, axis, K, window)
                assert same_bits(got, want), (v.shape, axis, K, window, int((got.view(np.uint32) != want.view(np.uint32)).sum()))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_unring_axis_is_bit_equal_to_the_specification(shape):
    """Values uniform in +-3000: every axis with a line of 8..512 samples, K in 1, 3, 20, the three windows."""
    v = values(shape, sum(shape))
    axes = [a for a in range(3) if U.MIN_LINE <= shape[a] <= U.MAX_LINE]
    assert axes
    compare(v, axes)


def test_the_most_shifts_once():
    compare(values((9, 11, 13), 32), (0, 1, 2), shifts=(32,), windows=((1, 3),))
    compare(values((2, 3, 200), 33), (2,), shifts=(32,), windows=((2, 4),))


@pytest.mark.parametrize("shape", [(9, 11, 13), (3, 5, 130), (260, 2, 9)], ids=str)
def test_nan_and_inf_go_where_the_specification_puts_them(shape):
    v = values(shape, 5, special=True)
    axes = [a for a in range(3) if shape[a] >= U.MIN_LINE]
    compare(v, axes, shifts=(3, 20), windows=((1, 3),))
    want = U.unring_axis_np(v, axes[0], 3)
    assert not np.isfinite(want).all() and np.isfinite(want).any()


def test_exact_ties_take_the_first_minimum():
    """Piecewise constant with small integer levels: most windows are flat at offset zero and keep their input bits, many
    variations are equal to the bit, and the strict comparison decides."""
    rng = np.random.default_rng(9)
    v = np.repeat(np.repeat(np.repeat(rng.integers(0, 4, (5, 4, 6)), 4, 0), 5, 1), 6, 2).astype(np.float32) * 64.0
    assert v.shape == (20, 20, 36)
    for axis in range(3):
        want = U.unring_axis_np(v, axis, 20)
        assert 0.3 < (want == v).mean() < 1.0
    compare(v, (0, 1, 2), shifts=(3, 20))
    sym = np.zeros((8, 8, 16), dtype=np.float32)                   # a symmetric box: left and right variations tie
    sym[:, :, 4:12] = 100.0
    compare(sym, (0, 2), shifts=(20,))
    const = np.full((8, 9, 10), -7.5, dtype=np.float32)
    for axis in range(3):
        assert same_bits(run(const, axis, 20, (1, 3)), const)


def test_out_two_runs_and_nothing_outside_the_volume():
    shape, margin = (9, 10, 14), 4096
    v = values(shape, 7)
    n = v.size
    src = torch.full((n + 2 * margin,), float("nan"), device="cuda")
    dst = torch.full((n + 2 * margin,), -5.0, device="cuda")
    src[margin:margin + n] = torch.from_numpy(v).cuda().reshape(-1)
    x = src[margin:margin + n].view(shape)
    out = dst[margin:margin + n].view(shape)
    for axis in range(3):
        want = U.unring_axis_np(v, axis, 3)
        back = U.unring_axis(x, axis, 3, out=out)
        assert back is out and same_bits(out.cpu().numpy(), want)
        assert bool((dst[:margin] == -5.0).all()) and bool((dst[margin + n:] == -5.0).all())
        again = U.unring_axis(x, axis, 3)
        assert again.data_ptr() != out.data_ptr() and torch.equal(again.view(torch.int32), out.view(torch.int32))
    assert torch.equal(x.cpu(), torch.from_numpy(v))                # the source is left alone


def test_graph_capture_and_replay_give_the_same_bits():
    """(2, 3, 512) along axis 2 takes 78 KB of LDS: the launch that raises the 64 KB limit is captured too."""
    v, long = values((12, 10, 70), 3), values((2, 3, 512), 4)
    x, y = torch.from_numpy(v).cuda(), torch.from_numpy(long).cuda()
    want = [U.unring_axis_np(v, axis, 20) for axis in range(3)] + [U.unring_axis_np(long, 2, 3)]
    for axis in range(3):
        U.unring_axis(x, axis)                                      # the tables of these extents are uploaded outside the capture
    U.unring_axis(y, 2, 3)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = [U.unring_axis(x, axis) for axis in range(3)] + [U.unring_axis(y, 2, 3)]
    for o in outs:
        o.fill_(0.0)
    graph.replay()
    torch.cuda.synchronize()
    for o, w in zip(outs, want):
        assert same_bits(o.cpu().numpy(), w)


def test_refusals():
    x = torch.zeros((8, 9, 10), device="cuda")
    with pytest.raises(ValueError, match="CUDA tensor"):
        U.unring_axis(x.cpu(), 0)
    with pytest.raises(ValueError, match="CUDA tensor"):
        U.unring(x.cpu())
    with pytest.raises(ValueError, match="CUDA tensor"):
        U.kspace_split(x.cpu())
    with pytest.raises(ValueError, match="float32"):
        U.unring_axis(x.double(), 0)
    with pytest.raises(ValueError, match="axis"):
        U.unring_axis(x, 3)
    with pytest.raises(ValueError, match="a line of 7 samples"):
        U.unring_axis(torch.zeros((7, 8, 8), device="cuda"), 0)
    with pytest.raises(ValueError, match="a line of 513 samples"):
        U.unring_axis(torch.zeros((1, 513, 1), device="cuda"), 1)
    for K in (0, 33, 2.0, True):
        with pytest.raises(ValueError, match="shifts"):
            U.unring_axis(x, 0, K)
    for window in ((0, 3), (2, 1), (1, 5), (1,), 3, (1.0, 2)):
        with pytest.raises(ValueError, match="window"):
            U.unring_axis(x, 0, 20, window)
    with pytest.raises(ValueError, match="weighting"):
        U.unring(x, (0, 1), weighting="none")
    with pytest.raises(ValueError, match="weighting"):
        U.unring(x, (0,), weighting="sinc")
    with pytest.raises(ValueError, match="axis 0"):
        U.unring(torch.zeros((7, 8, 8), device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        U.unring_axis(x, 0, out=x)
    with pytest.raises(ValueError, match="out must be"):
        U.unring_axis(x, 0, out=torch.zeros((8, 9, 11), device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        U.unring_axis(x, 0, out=torch.zeros((8, 9, 10)))
    # the entry itself, without a launch: null, misaligned, overlapping, the line, K, the window
    fn = _lib.load().mrisr_f32_volume_unring_axis
    t = torch.zeros(64, device="cuda")
    big = torch.full((2 * 512 + 16,), 9.0, device="cuda")
    p, d = big.data_ptr(), big.data_ptr() + 4 * 520
    assert fn(None, 8, 8, 8, 0, 20, 1, 3, t.data_ptr(), t.data_ptr(), d, None) == -1
    assert fn(p, 8, 8, 8, 0, 20, 1, 3, None, t.data_ptr(), d, None) == -1
    assert fn(p, 8, 8, 8, 0, 20, 1, 3, t.data_ptr(), None, d, None) == -1
    assert fn(p + 2, 8, 8, 8, 0, 20, 1, 3, t.data_ptr(), t.data_ptr(), d, None) == -1
    assert fn(p, 8, 8, 8, 0, 20, 1, 3, t.data_ptr(), t.data_ptr(), p, None) == -1
    assert fn(p, 8, 8, 8, 0, 20, 1, 3, t.data_ptr(), t.data_ptr(), p + 4 * 511, None) == -1          # the last voxel of src is dst's first
    assert fn(p, 8, 8, 8, 3, 20, 1, 3, t.data_ptr(), t.data_ptr(), d, None) == -1
    assert fn(p, 8, 8, 8, 0, 0, 1, 3, t.data_ptr(), t.data_ptr(), d, None) == -1
    assert fn(p, 8, 8, 8, 0, 33, 1, 3, t.data_ptr(), t.data_ptr(), d, None) == -1
    assert fn(p, 8, 8, 8, 0, 20, 0, 3, t.data_ptr(), t.data_ptr(), d, None) == -1
    assert fn(p, 8, 8, 8, 0, 20, 3, 2, t.data_ptr(), t.data_ptr(), d, None) == -1
    assert fn(p, 8, 8, 8, 0, 20, 1, 5, t.data_ptr(), t.data_ptr(), d, None) == -1
    assert fn(p, 7, 8, 8, 0, 20, 1, 3, t.data_ptr(), t.data_ptr(), d, None) == -2
    assert fn(p, 1, 513, 1, 1, 20, 1, 3, t.data_ptr(), t.data_ptr(), d, None) == -2
    assert fn(p, 0, 8, 8, 1, 20, 1, 3, t.data_ptr(), t.data_ptr(), d, None) == -2
    torch.cuda.synchronize()
    assert bool((big == 9.0).all())                                 # nothing ran


def test_unring_is_the_sum_of_its_parts():
    v = values((12, 10, 16), 21)
    x = torch.from_numpy(v).cuda()
    for axes in ((0, 1, 2), (0, 2), (1, 2), (2, 0, 1)):
        parts = U.kspace_split(x, axes)
        assert len(parts) == len(axes) and all(p.is_contiguous() and p.dtype == torch.float32 for p in parts)
        want = None
        for p, a in zip(parts, sorted(axes)):
            u = U.unring_axis(p, a, 3, (1, 2))
            want = u if want is None else want + u
        got = U.unring(x, axes, 3, (1, 2))
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), axes
    # one axis: no split, and the same bits with either weighting
    one = U.unring(x, (1,), 3)
    assert U.kspace_split(x, (1,))[0] is x
    assert torch.equal(one.view(torch.int32), U.unring_axis(x, 1, 3).view(torch.int32))
    assert torch.equal(one.view(torch.int32), U.unring(x, (1,), 3, weighting="none").view(torch.int32))
    U.kspace_split(torch.zeros((8, 8, 10), device="cuda"), (0, 1))
    assert len(U._WEIGHTS) == 1                                     # the weights are as large as the spectra: the last shape only
    assert torch.equal(x.cpu(), torch.from_numpy(v))


@pytest.mark.parametrize("shape,axes", [((16, 12, 20), (0, 1, 2)), ((8, 8, 8), (0, 1, 2)), ((24, 10, 16), (0, 2)), ((9, 16, 32), (1, 2))],
                         ids=str)
def test_kspace_split_agrees_with_the_float64_fft(shape, axes):
    """The bound.  A float32 FFT of N points computed by butterflies satisfies (Higham, Accuracy and Stability of Numerical
    Algorithms, theorem 24.2)  ||fl(F x) - F x||_2 <= log2(N) eta ||F x||_2  with  eta = mu + gamma_4 (sqrt(2) + mu)  <  7 u  for
    twiddle factors good to mu = u = 2^-24: 3.5 eps32 log2(N) per transform, eps32 = 2^-23.  The split is a forward transform, a
    product with a weight 0 <= G <= 1 that is itself rounded (one u each: together 1 eps32), an inverse transform of that product
    (another 3.5 eps32 log2(N), on a vector no longer than the input's transform since G <= 1), and the reference is rounded once
    (0.5 eps32): relative to ||v||_2 at most  (7 log2(N) + 1.5) eps32 <= 8 eps32 log2(N)  for N >= 4, so c = 8.  Divided by sqrt(N) this
    bounds the root-mean-square difference by  c eps32 log2(N) rms(v) <= c eps32 log2(N) max|v|:  that is asserted.  Every single
    voxel is held to the same figure,  c eps32 log2(N) max|v|:  there it is the issue's bound backed by measurement (the worst voxel
    lies at 0.04 of it, profiles/NOTES.md), not by the normwise theorem, which only keeps a voxel below the 2-norm, sqrt(N) times
    more.  The parts also sum to the input within len(axes) times the figure, per voxel.  The extents are products of 2, 3 and 5,
    where the transform is butterflies throughout.  N is the number of points transformed (the product of the extents of ``axes``)."""
    v = values(shape, sum(shape))
    want = U.kspace_split_np(v, axes)
    parts = U.kspace_split(torch.from_numpy(v).cuda(), axes)
    got = np.stack([p.cpu().numpy() for p in parts])
    assert got.shape == want.shape == (len(axes),) + shape
    N = int(np.prod([shape[a] for a in axes]))
    bound = 8.0 * 2.0 ** -23 * math.log2(N) * float(np.abs(v).max())
    diff = got.astype(np.float64) - want.astype(np.float64)
    rms, worst = float(np.sqrt((diff ** 2).mean())), float(np.abs(diff).max())
    print(f"kspace_split {shape} axes {axes}: rms / bound = {rms / bound:.4f}, max / bound = {worst / bound:.4f}")
    assert rms <= bound and worst <= bound
    total = got.astype(np.float64).sum(axis=0)
    assert np.abs(total - v).max() <= len(axes) * bound
