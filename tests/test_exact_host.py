"""Why tests/test_gpu_exact.py exists, pinned down on the CPU: one missing (pixel, tap, channel) product passes the bf16
tolerance of the parity tests and cannot pass the exact comparison.  Plus the exact helpers' own checks (hiputil.dyadic,
hiputil.assert_exact)."""
import pytest
import torch
import torch.nn.functional as F

from mri_superresolution_amd import _lib as L
import hiputil as U
from test_gpu_kernels import TOL_OUT, rnd

SHAPE = (1, 256, 128, 16, 32)              # the ring kernel's smallest launch
ELEM = (0, 5, 8, 16)                       # the output element that loses one product


def test_dyadic_is_seeded_and_on_the_grid():
    a, b = U.dyadic((3, 5, 7), 1, 0.25), U.dyadic((3, 5, 7), 1, 0.25)
    assert torch.equal(a, b) and a.dtype == torch.float32
    assert not torch.equal(a, U.dyadic((3, 5, 7), 2, 0.25))
    big = U.dyadic((64, 64, 16), 3, 0.25, values=(-2, 0.5, 4))
    assert set(big.unique().tolist()) == {-2.0, 0.0, 0.5, 4.0}
    assert 0.22 < float((big != 0).float().mean()) < 0.28
    assert not U.dyadic((100,), 4, 0.0).any() and U.dyadic((100,), 4, 1.0).all()


def _tier_a_reference():
    n, cin, cout, h, w = SHAPE
    x, wt = U.dyadic((n, cin, h, w), 41, 0.25), U.dyadic((cout, cin, 3, 3), 42, 0.25)
    ref = F.conv2d(x.double(), wt.double(), padding=1)
    return x, wt, ref


def _first_nonzero_product(x, wt):
    """(ci, ky, kx) of the first non-zero product x * w in the sum of output ELEM."""
    n, co, y, xx = ELEM
    for ci in range(x.shape[1]):
        for ky in range(3):
            for kx in range(3):
                if x[n, ci, y + ky - 1, xx + kx - 1] != 0 and wt[co, ci, ky, kx] != 0:
                    return ci, ky, kx
    raise AssertionError("no non-zero product")


def test_one_missing_product_fails_the_exact_check_and_names_the_element():
    x, wt, ref = _tier_a_reference()
    n, co, y, xx = ELEM
    ci, ky, kx = _first_nonzero_product(x, wt)
    for dt in (L.F32, L.BF16, L.F16):
        # the fp32 CPU conv equals the float64 one bit for bit, and the intact result passes in every storage type
        assert torch.equal(F.conv2d(x, wt, padding=1).double(), ref)
        U.assert_exact(ref.to(U.tdt(dt)).float(), ref, dt)
        got = ref.clone()
        got[ELEM] -= float(x[n, ci, y + ky - 1, xx + kx - 1] * wt[co, ci, ky, kx])
        with pytest.raises(AssertionError) as e:
            U.assert_exact(got.to(U.tdt(dt)).float(), ref, dt)
        assert "1 of" in str(e.value) and str(ELEM) in str(e.value)


def test_the_same_defect_passes_the_bf16_tolerance():
    """The randn data of test_gpu_kernels.py::test_conv_ring_raw_source (its generators and seeds) at the smallest ring shape:
    the same defect - one product missing from output ELEM - stays within TOL_OUT[BF16] of the intact result for the product
    of median size, and for more than nine in ten of the 2304 products of that element."""
    n, cin, cout, h, w = SHAPE
    x, wt = U.rounded(rnd(n, cin, h, w, seed=41), L.BF16), U.rounded(rnd(cout, cin, 3, 3, seed=42, scale=0.1), L.BF16)
    ref = F.conv2d(x, wt, padding=1)
    bn, co, y, xx = ELEM
    products = x[bn, :, y - 1:y + 2, xx - 1:xx + 2] * wt[co]
    assert torch.allclose(products.sum(), ref[ELEM], rtol=1e-4)              # these ARE the terms of that element
    median = products.flatten()[products.abs().flatten().argsort()[products.numel() // 2]]
    got = ref.clone()
    got[ELEM] -= median
    err = U.relerr(got, ref)
    assert 0 < err <= TOL_OUT[L.BF16], err
    passing = (products.abs() / ref.abs().max() <= TOL_OUT[L.BF16]).float().mean()
    assert passing > 0.9, passing


def test_assert_exact_rejects_a_reference_off_the_grid():
    ref = torch.tensor([[1.0, 257.0, -3.0]], dtype=torch.float64)          # 257 needs 9 significant bits
    U.assert_exact(ref.float(), ref, L.F32)
    U.assert_exact(ref.float(), ref, L.F16)
    with pytest.raises(AssertionError, match="not on the"):
        U.assert_exact(ref.to(torch.bfloat16).float(), ref, L.BF16)
    with pytest.raises(AssertionError, match="not on the"):
        U.assert_exact(torch.tensor([0.1]), torch.tensor([0.1], dtype=torch.float64), L.F32)
    with pytest.raises(AssertionError, match="not finite"):
        U.assert_exact(torch.tensor([1.0]), torch.tensor([float("nan")], dtype=torch.float64), L.F32)


def test_assert_exact_tier_b_rounds_the_reference_once():
    ref = torch.tensor([257.0, 3.2001953125, -0.2001953125], dtype=torch.float64)
    once = ref.to(torch.bfloat16)
    assert once.tolist() == [256.0, 3.203125, -0.2001953125]
    U.assert_exact(once.float(), ref, L.BF16, tier="B")
    with pytest.raises(AssertionError, match="1 of 3"):
        U.assert_exact(torch.tensor([258.0, 3.203125, -0.2001953125]), ref, L.BF16, tier="B")
    # a NaN in the result is a mismatch, and shapes must agree
    with pytest.raises(AssertionError):
        U.assert_exact(torch.tensor([float("nan"), 3.203125, -0.2001953125]), ref, L.BF16, tier="B")
    with pytest.raises(AssertionError, match="shape"):
        U.assert_exact(once.float()[:2], ref, L.BF16, tier="B")


def test_int_pattern_is_a_non_zero_integer_start_value():
    p = U.int_pattern((4, 3, 2), torch.float64)
    assert p.shape == (4, 3, 2) and torch.equal(p, p.round()) and p.abs().max() <= 3 and (p != 0).float().mean() > 0.5
