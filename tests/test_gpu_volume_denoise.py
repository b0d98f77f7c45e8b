"""Rician non-local-means denoising (GPU): csrc/volume_denoise.hip against the numpy specification of volume_denoise.py, bit for
bit, the noise estimate, HIP-graph capture of the whole filter and the entry points' refusals."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import denoiseutil as U                                                      # noqa: E402
from mri_superresolution_amd import volume_denoise as D                      # noqa: E402

E_ARG, E_SHAPE = -1, -2      # MRISR_E_ARG, MRISR_E_SHAPE (include/mrisr.h)
F = np.float32
# the kernel's tile is 8 x 16 x 32 voxels (axis 0, 1, 2): (9, 17, 33) exceeds it by one voxel on every axis
TILE_PLUS_ONE = (9, 17, 33)
SMALL = [(1, 1, 1), (2, 3, 5), (8, 8, 8), TILE_PLUS_ONE]
SHAPES = SMALL + [(19, 23, 37), (5, 64, 12), (3, 4, 70)]
CASES = [(s, r) for s in SHAPES for r in (1, 2, 3)] + [(s, 5) for s in SMALL]
# x = d * inv_h2 with d around 27 * 2 * 80^2 = 3.5e5 for noise of +- 80: 2.5e-5 spreads x over [0, 16) and past it
SPREAD, NO_WEIGHT, FULL_WEIGHT = F(2.5e-5), F(np.inf), F(1e-30)


def params_on_device(inv_h2, two_sigma2):
    return torch.tensor([inv_h2, two_sigma2, 0.0, 1.0], dtype=torch.float32).cuda()


def table_indices(v, inv_h2, radius):
    """The distinct table indices the specification reads for this volume."""
    seen = set()
    for t in D.offsets(radius):
        x = D.patch_distance_np(v, t) * inv_h2
        x = x[np.isfinite(x) & (x < 16)]
        seen.update(np.unique((x * F(256)).astype(np.int32)).tolist())
    return seen


@pytest.mark.parametrize("shape,radius", CASES, ids=[f"{'x'.join(map(str, s))}-R{r}" for s, r in CASES])
def test_denoise_equals_the_specification(shape, radius):
    v = U.messy_volume(shape, sum(shape) + radius)
    two_sigma2 = D.noise_params_np(40.0)[1]
    if v.size >= 500:
        assert len(table_indices(v, SPREAD, radius)) >= 100
    aligned, shifted = U.on_device(v, 0), U.on_device(v, 1)
    out_shifted = U.on_device(np.zeros(shape, dtype=np.float32), 1)
    for rician in (True, False):
        for inv_h2 in (SPREAD, NO_WEIGHT, FULL_WEIGHT):
            want = D.denoise_np(v, inv_h2, two_sigma2, radius, rician)
            p = params_on_device(inv_h2, two_sigma2)
            got = D.denoise(aligned, p, radius, rician)
            assert U.same_bits(got.cpu().numpy(), want), (shape, radius, rician, float(inv_h2), "aligned")
            res = D.denoise(shifted, p, radius, rician, out=out_shifted)
            assert res is out_shifted and U.same_bits(out_shifted.cpu().numpy(), want), (shape, radius, rician, float(inv_h2), "shifted")


def test_estimate_noise():
    noisy = U.rician(U.phantom(), 30.0)
    noisy[3, 4, 5:8] = [np.nan, np.inf, -np.inf]
    _, r = U.radius_grid()
    air = (r > 17).astype(np.uint8)
    want_sigma, want_count = D.estimate_sigma_np(noisy, air)
    vol, bg = torch.from_numpy(noisy).cuda(), torch.from_numpy(air).cuda()
    params, count = D.estimate_noise(vol, bg, beta=0.5)
    again, _ = D.estimate_noise(vol, bg, beta=0.5)
    got = params.cpu().numpy()
    assert int(count) == want_count
    print("sigma", got[2], want_sigma)
    assert abs(float(got[2]) - float(want_sigma)) <= float(np.spacing(want_sigma))
    inv_h2, two_sigma2, sigma = D.noise_params_np(got[2], 0.5)
    assert np.array_equal(U.bits(got), U.bits(np.array([inv_h2, two_sigma2, sigma, 0.5], dtype=np.float32)))
    assert torch.equal(params.view(torch.int32), again.view(torch.int32))
    # a bool mask, params given
    mine = torch.empty(4, dtype=torch.float32, device="cuda")
    res, _ = D.estimate_noise(vol, bg != 0, beta=0.5, params=mine)
    assert res is mine and torch.equal(mine.view(torch.int32), params.view(torch.int32))
    # an empty background: sigma 0, inv_h2 inf, and the filter then returns the non-negative input
    params, count = D.estimate_noise(vol, torch.zeros_like(bg))
    got = params.cpu().numpy()
    assert int(count) == 0 and got[2] == 0 and got[1] == 0 and got[0] == np.inf
    clean = np.abs(U.messy_volume((6, 7, 9), 2))
    clean[~np.isfinite(clean)] = 3.0
    assert U.same_bits(D.denoise(torch.from_numpy(clean).cuda(), params, 2, True).cpu().numpy(), clean)
    # sigma given: no sums
    params, count = D.estimate_noise(vol, None, beta=2.0, sigma=12.5)
    inv_h2, two_sigma2, sigma = D.noise_params_np(12.5, 2.0)
    assert int(count) == 0
    assert np.array_equal(U.bits(params.cpu().numpy()), U.bits(np.array([inv_h2, two_sigma2, sigma, 2.0], dtype=np.float32)))
    assert torch.equal(D.noise_params(12.5, 2.0, "cuda").view(torch.int32), params.view(torch.int32))
    # the background mask
    assert np.array_equal(D.background_mask(vol, 3).cpu().numpy().astype(np.uint8), D.background_mask_np(noisy, 3))


def test_denoise_volume_is_graph_capturable():
    first, second = U.rician(U.phantom(), 60.0, seed=0), U.rician(U.phantom(), 40.0, seed=1)
    vol = torch.from_numpy(first).cuda()
    eager = D.denoise_volume(vol, beta=0.5, radius=2, check=False)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        D.denoise_volume(vol, beta=0.5, radius=2, check=False)      # warm-up: code objects loaded, the table uploaded
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = D.denoise_volume(vol, beta=0.5, radius=2, check=False)
    for data in (first, second):
        vol.copy_(torch.from_numpy(data))
        graph.replay()
        torch.cuda.synchronize()
        want = D.denoise_volume(vol, beta=0.5, radius=2, check=False)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))
        if data is first:
            assert torch.equal(out.view(torch.int32), eager.view(torch.int32))
        # the device's sigma is within an ulp of the specification's (test_estimate_noise): the filter is checked with the device's
        p = D.estimate_noise(vol, D.background_mask(vol), beta=0.5)[0].cpu().numpy()
        assert abs(float(p[2]) - float(D.estimate_sigma_np(data, D.background_mask_np(data))[0])) <= float(np.spacing(p[2]))
        assert U.same_bits(out.cpu().numpy(), D.denoise_np(data, p[0], p[1], 2, True))


def test_denoise_volume_checks_the_estimate():
    noisy = U.rician(U.phantom(), 60.0)
    _, r = U.radius_grid()
    vol = torch.from_numpy(noisy).cuda()
    out, noise = D.denoise_volume(vol, radius=1, return_noise=True)
    assert abs(noise["sigma"] - 60.0) < 3.0 and noise["count"] == int(D.background_mask_np(noisy).sum()) >= 1000
    stripped = noisy.copy()
    stripped[r > 14] = 0.0                                       # zeroed air: nothing to estimate from
    with pytest.raises(ValueError, match="--sigma"):
        D.denoise_volume(torch.from_numpy(stripped).cuda(), radius=1)
    tiny = torch.from_numpy(np.ascontiguousarray(noisy[:6, :6, :6])).cuda()      # fewer than 1000 voxels in all
    with pytest.raises(ValueError, match="--sigma"):
        D.denoise_volume(tiny, radius=1)
    given = D.denoise_volume(torch.from_numpy(stripped).cuda(), sigma=60.0, radius=1)
    inv_h2, two_sigma2, _ = D.noise_params_np(60.0)
    assert U.same_bits(given.cpu().numpy(), D.denoise_np(stripped, inv_h2, two_sigma2, 1, True))


def test_device_argument_errors():
    v = torch.zeros((4, 4, 4), dtype=torch.float32, device="cuda")
    p = D.noise_params(10.0, 1.0, "cuda")
    for radius in (0, 6):
        with pytest.raises(ValueError):
            D.denoise(v, p, radius)
    with pytest.raises(ValueError):
        D.denoise(v.double(), p)
    with pytest.raises(ValueError):
        D.denoise(v[:, :, ::2], p)
    with pytest.raises(ValueError):
        D.denoise(v, p[:3])
    with pytest.raises(ValueError):
        D.denoise(v, p, out=v)
    with pytest.raises(ValueError):
        D.denoise(v, p, out=torch.zeros((4, 4, 5), device="cuda"))
    with pytest.raises(ValueError):
        D.estimate_noise(v, torch.ones((4, 4, 5), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        D.estimate_noise(v, torch.ones((4, 4, 4), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        D.denoise_volume(v, beta=0.0)
    # the C entry points refuse on their own and launch nothing: the outputs keep their sentinel
    from mri_superresolution_amd import _lib as L
    lib = L.load()
    table = torch.from_numpy(D.WEIGHT_TABLE.copy()).cuda()
    out = torch.full_like(v, -7.0)

    def nlm(vol=v.data_ptr(), X=4, Y=4, Z=4, radius=2, params=p.data_ptr(), tab=table.data_ptr(), o=out.data_ptr()):
        return lib.mrisr_f32_volume_nlm(vol, X, Y, Z, radius, 1, params, tab, o, None)

    assert nlm(radius=0) == E_ARG and nlm(radius=6) == E_ARG and nlm(radius=-1) == E_ARG
    assert nlm(vol=None) == E_ARG and nlm(params=None) == E_ARG and nlm(tab=None) == E_ARG and nlm(o=None) == E_ARG
    assert nlm(o=v.data_ptr()) == E_ARG
    assert nlm(X=0) == E_SHAPE and nlm(Y=0) == E_SHAPE and nlm(Z=32768) == E_SHAPE
    bg = torch.ones((4, 4, 4), dtype=torch.uint8, device="cuda")
    got = torch.full((4,), -7.0, dtype=torch.float32, device="cuda")
    count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(int(lib.mrisr_f32_volume_noise_workspace_bytes()) // 8, dtype=torch.int64, device="cuda")

    def noise(vol=v.data_ptr(), b=bg.data_ptr(), n=64, beta=1.0, sigma=0.0, pr=got.data_ptr(), c=count.data_ptr(), w=ws.data_ptr()):
        return lib.mrisr_f32_volume_noise_params(vol, b, n, beta, sigma, pr, c, w, None)

    assert noise(vol=None) == E_ARG and noise(b=None) == E_ARG and noise(pr=None) == E_ARG and noise(c=None) == E_ARG and noise(w=None) == E_ARG
    assert noise(beta=0.0) == E_ARG and noise(beta=float("nan")) == E_ARG and noise(sigma=-1.0) == E_ARG and noise(sigma=float("inf")) == E_ARG
    assert noise(n=0) == E_SHAPE
    torch.cuda.synchronize()
    assert (out == -7).all() and (got == -7).all() and (count == -7).all()
    assert nlm() == 0 and noise() == 0 and noise(vol=None, b=None, sigma=3.0) == 0
    torch.cuda.synchronize()
    assert (out == 0).all() and int(count) == 0 and float(got[2]) == 3.0
