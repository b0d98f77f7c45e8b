"""The numpy restatement of the float percentile window (utils/imageops.percentile_bounds_np) is the specification the selection
kernel of csrc/percentile.hip is tested against (tests/test_gpu_percentile.py); here it is itself pinned to np.percentile on
float32 input, by value, for every input class and shape of the GPU tests.  No GPU needed."""
import numpy as np
import pytest

from mri_superresolution_amd.utils.imageops import percentile_bounds_np

SHAPES = [(1, 1), (1, 2), (1, 3), (7, 9), (1, 201), (24, 40), (50, 70), (128, 128), (512, 512)]
QS = [0.0, 0.5, 50.0, 99.5, 100.0]


def input_class(name, shape, seed=0):
    """One float32 image of the named class (shared with tests/test_gpu_percentile.py)."""
    rng = np.random.default_rng([seed, shape[0], shape[1]])
    n = shape[0] * shape[1]
    if name == "normal":             # both signs
        a = rng.standard_normal(n) * 1000.0
    elif name == "mri":              # ~60 % exact zeros, the rest integers 0..4095: ties straddle the selected ranks
        a = np.where(rng.random(n) < 0.6, 0.0, rng.integers(0, 4096, n).astype(np.float64))
    elif name == "constant":
        a = np.full(n, 1234.5)
    elif name == "two_values":
        a = np.where(rng.random(n) < 0.3, -7.25, 3.5)
    elif name == "last_digit":       # 1 + i 2^-23, shuffled: only the last radix digit (and for n > 256 the one before) differs
        a = 1.0 + rng.permutation(n).astype(np.float64) * 2.0 ** -23
    elif name == "magnitudes":       # 1e-30 .. 1e30, both signs
        a = 10.0 ** rng.uniform(-30, 30, n) * rng.choice([-1.0, 1.0], n)
    else:
        raise KeyError(name)
    return a.astype(np.float32).reshape(shape)


CLASSES = ["normal", "mri", "constant", "two_values", "last_digit", "magnitudes"]


@pytest.mark.parametrize("name", CLASSES)
def test_restatement_equals_np_percentile(name):
    for shape in SHAPES:
        a = input_class(name, shape)
        for q in QS:
            want = np.percentile(a, q)
            assert want.dtype == np.float32
            got = percentile_bounds_np(a, q, q)
            assert got.dtype == np.float32 and got[0] == want and got[1] == want, (name, shape, q, got, want)
    a = input_class(name, (50, 70), seed=3)
    got = percentile_bounds_np(a, 0.5, 99.5)
    assert got[0] == np.percentile(a, 0.5) and got[1] == np.percentile(a, 99.5)


def test_restatement_is_the_float32_interpolation_not_the_rounded_float64_one():
    """What the kernel has to reproduce is numpy's float32 path; the float64 interpolation rounded to float32 is another
    number on some inputs (here: in the last place at q = 99.5)."""
    differs = 0
    for seed in range(40):
        a = input_class("normal", (24, 40), seed=seed)
        got = percentile_bounds_np(a, 0.5, 99.5)[1]
        assert got == np.percentile(a, 99.5)
        differs += int(got != np.float32(np.percentile(a.astype(np.float64), 99.5)))
    assert differs > 0


def test_restatement_refuses_other_input():
    with pytest.raises(ValueError):
        percentile_bounds_np(np.zeros((4, 4), dtype=np.float64))
    with pytest.raises(ValueError):
        percentile_bounds_np(np.zeros((0, 4), dtype=np.float32))
