"""The unmasked ``mrisr_f32_volume_metrics`` kernel against RECORDED sums.

``ssim_term()`` in csrc/volume_metrics.hip spells out every rounding of the SSIM term, one product fused (``mu1^2`` into
``mu1^2 + mu2^2``): the form the compiler had chosen for the expression before the kernel became a template on ``kMasked``.  The
recorded values (tests/golden/volume_metrics_sums.json, doubles as hex strings) are the three sums - sum |a - b|, sum of SSIM terms,
sum (a - b)^2 - that the kernel of the commit BEFORE the masked form gave on an MI355X for the inputs below, so this test holds the
unmasked results where they were: another choice of the fused product moves the SSIM sum by about 3e-9 relative.

Bar: 1e-12 relative per sum.  The float32 terms are bit-equal by construction; only the order of the double additions (wave
shuffles, one atomic per block) is free, and n <= 116550 doubles of one sign add up within n * 2^-53 = 1.3e-11 relative in the
worst case, about sqrt(n) * 2^-53 = 4e-14 in practice.  The SSIM terms are not all of one sign in general, but on these inputs
(prediction = truth plus 5 % noise) every term is positive.
"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "volume_metrics_sums.json")
SHAPES = [(1, 1, 1), (5, 3, 40), (12, 11, 10), (70, 37, 45)]
WINDOWS = [3, 5, 7, 9, 11, 13, 15]


def _pair(shape):
    rs = np.random.RandomState(1234)
    ref = rs.rand(*shape).astype(np.float32)
    pred = np.clip(ref + np.float32(0.05) * rs.randn(*shape).astype(np.float32), 0, 1).astype(np.float32)
    return pred, ref


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_unmasked_sums_are_the_recorded_ones(shape, golden):
    from mri_superresolution_amd import _lib as L
    pred, ref = _pair(shape)
    a, b = torch.from_numpy(pred).cuda(), torch.from_numpy(ref).cuda()
    for win in WINDOWS:
        want = np.array([float.fromhex(h) for h in golden["x".join(map(str, shape)) + f"_w{win}"]])
        sums = torch.zeros(3, dtype=torch.float64, device="cuda")
        L.call("mrisr_f32_volume_metrics", a.data_ptr(), b.data_ptr(), *shape, 1.0, 1.5, win, sums.data_ptr(), L.stream_ptr())
        got = sums.cpu().numpy()
        err = np.abs(got - want) / np.abs(want).clip(min=1e-300)
        print(f"{shape} window {win}: relative distance from the recorded sums {err}")
        assert np.all(want[[0, 2]] >= 0) and want[1] > 0
        assert np.all(err <= 1e-12), (shape, win, got.tolist(), want.tolist())
