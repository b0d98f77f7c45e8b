"""Zero-filled x2 interpolation and k-space truncation on the device (csrc/volume_kspace.hip): ``zerofill2`` and ``truncate2`` against
their numpy specifications, bit for bit, at every launch shape - each bundle width, lines shorter and longer than a block of source
samples, a chunk that ends inside a thread's outputs, the limit along each axis, more bundles than one workgroup takes."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from mri_superresolution_amd import volume_kspace as K      # noqa: E402

AXES = ((0,), (1,), (2,), (0, 1, 2))
# the source shapes of zerofill2; truncate2 gets their doubled counterparts and gives these shapes back
SHAPES = [(1, 1, 1), (2, 2, 2), (3, 5, 7), (1, 1, 70), (33, 17, 65), (5, 3, 512), (512, 1, 2), (2, 512, 3), (40, 40, 40)]


def values(shape, seed, special=False):
    v = np.random.default_rng(seed).uniform(-3000.0, 3000.0, shape).astype(np.float32)
    if special:                                                     # a single voxel has room for the Inf alone
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


def run(fn, v, axes, window, **kw):
    out = fn(torch.from_numpy(v).cuda(), axes, window, **kw)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_zerofill2_is_bit_equal_to_the_specification(shape):
    for special in (False, True):
        v = values(shape, sum(shape) + special, special)
        for window in K.WINDOWS:
            for axes in AXES:
                want = K.zerofill2_np(v, axes, window)
                got = run(K.zerofill2, v, axes, window)
                assert same_bits(got, want), (shape, axes, window, special, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
                if special:
                    assert not np.isfinite(want).all()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_truncate2_is_bit_equal_to_the_specification(shape):
    fine = tuple(2 * d for d in shape)                              # the doubled counterpart: even on every axis
    for special in (False, True):
        v = values(fine, sum(fine) + special, special)
        for window in K.WINDOWS:
            for axes in AXES:
                want = K.truncate2_np(v, axes, window)
                got = run(K.truncate2, v, axes, window)
                assert same_bits(got, want), (fine, axes, window, special, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
                if special:
                    assert not np.isfinite(want).all()


def test_negative_values_and_ringing_are_kept():
    v = np.zeros((4, 4, 16), dtype=np.float32)
    v[:, :, 8:] = 100.0
    got = run(K.zerofill2, v, (2,), "none")
    assert got.min() < -1.0 and got.max() > 101.0                   # Gibbs ringing, not clipped


def test_out_two_runs_and_views():
    v = values((6, 10, 14), 7)
    x = torch.from_numpy(v).cuda()
    want = K.zerofill2_np(v, (0, 2), "hamming")
    out = torch.full((12, 10, 28), -7.0, device="cuda")
    back = K.zerofill2(x, (0, 2), "hamming", out=out)
    assert back is out and same_bits(out.cpu().numpy(), want)
    again = K.zerofill2(x, (0, 2), "hamming")
    assert again.data_ptr() != out.data_ptr() and torch.equal(again.view(torch.int32), out.view(torch.int32))
    low = torch.empty((3, 10, 7), device="cuda")
    assert K.truncate2(x, (0, 2), out=low) is low and same_bits(low.cpu().numpy(), K.truncate2_np(v, (0, 2)))
    assert torch.equal(K.truncate2(x, (0, 2)).view(torch.int32), low.view(torch.int32))
    assert torch.equal(x.cpu(), torch.from_numpy(v))                # the source is left alone


def test_nothing_is_read_or_written_outside_the_volumes():
    shape, margin = (5, 6, 9), 4096
    v = values(shape, 11)
    n_in, n_out = v.size, 8 * v.size
    src = torch.full((n_in + 2 * margin,), float("nan"), device="cuda")
    dst = torch.full((n_out + 2 * margin,), -5.0, device="cuda")
    src[margin:margin + n_in] = torch.from_numpy(v).cuda().reshape(-1)
    x = src[margin:margin + n_in].view(shape)
    out = dst[margin:margin + n_out].view(10, 12, 18)
    K.zerofill2(x, out=out)
    assert same_bits(out.cpu().numpy(), K.zerofill2_np(v))
    assert bool((dst[:margin] == -5.0).all()) and bool((dst[margin + n_out:] == -5.0).all())


def test_graph_capture_and_replay_give_the_same_bits():
    v = values((12, 10, 70), 3)
    x = torch.from_numpy(v).cuda()
    want_up, want_down = K.zerofill2_np(v, window="hamming"), K.truncate2_np(v)
    K.zerofill2(x, window="hamming"), K.truncate2(x)                 # the tables of these extents are uploaded outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        up = K.zerofill2(x, window="hamming")
        down = K.truncate2(x)
    for _ in range(2):
        up.fill_(0.0), down.fill_(0.0)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(up.cpu().numpy(), want_up) and same_bits(down.cpu().numpy(), want_down)


def test_refusals():
    x = torch.zeros((4, 6, 8), device="cuda")
    with pytest.raises(ValueError, match="CUDA tensor"):
        K.zerofill2(x.cpu())
    with pytest.raises(ValueError, match="float32"):
        K.zerofill2(x.double())
    with pytest.raises(ValueError, match="float32"):
        K.truncate2(torch.zeros((0, 4, 4), device="cuda"))
    with pytest.raises(ValueError, match="window"):
        K.zerofill2(x, window="hann")
    with pytest.raises(ValueError, match="axes"):
        K.truncate2(x, (0, 3))
    with pytest.raises(ValueError, match="extent 3 of axis 1 is odd"):
        K.truncate2(torch.zeros((4, 3, 8), device="cuda"))
    with pytest.raises(ValueError, match="longer than the limit of 512"):
        K.zerofill2(torch.zeros((1, 513, 1), device="cuda"), (1,))
    assert tuple(K.zerofill2(torch.zeros((1, 513, 1), device="cuda"), (0, 2)).shape) == (2, 513, 2)      # the limit is per doubled axis
    with pytest.raises(ValueError, match="longer than the limit of 1024"):
        K.truncate2(torch.zeros((1026, 1, 1), device="cuda"), (0,))
    with pytest.raises(ValueError, match="out must be"):
        K.zerofill2(x, (0,), out=torch.zeros((4, 6, 8), device="cuda"))          # not the doubled shape
    with pytest.raises(ValueError, match="out must be"):
        K.zerofill2(x, (0,), out=torch.zeros((8, 6, 8), device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError, match="out must be"):
        K.zerofill2(x, (0,), out=torch.zeros((8, 6, 8)))
    both = torch.zeros(2 * x.numel(), device="cuda")
    with pytest.raises(ValueError, match="out must be"):
        K.zerofill2(both[:x.numel()].view(4, 6, 8), (0,), out=both.view(8, 6, 8))      # aliased
