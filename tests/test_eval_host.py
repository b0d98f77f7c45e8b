"""CPU-only checks of the device-side evaluation feature: the flags of scripts/evaluate.py, the argument validation of
utils/evalops.py that happens before any launch, the new entries of the C ABI."""
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def test_evaluate_flags_default_to_the_per_image_path():
    from scripts import evaluate as ev
    a = ev.parse_args(["--full_res_dir", "hr", "--low_res_dir", "lr"])
    assert (a.batch_size, a.no_graph) == (0, False)
    a = ev.parse_args(["--full_res_dir", "hr", "--low_res_dir", "lr", "--batch_size", "16", "--no_graph"])
    assert (a.batch_size, a.no_graph) == (16, True)
    assert "--batch_size" in ev.__doc__ and "--no_graph" in ev.__doc__
    with pytest.raises(ValueError):
        ev.run_benchmarks_batched([], None, "cuda", batch_size=0)


def test_evalops_refuses_cpu_tensors_and_bad_arguments():
    from mri_superresolution_amd.utils import evalops
    x = torch.zeros((4, 6), dtype=torch.uint8)
    with pytest.raises(ValueError, match="Unknown interpolation method: nearest"):
        evalops.upscale2_u8(x, "nearest")
    for method in ("bilinear", "bicubic", "sharp_bilinear"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evalops.upscale2_u8(x, method)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evalops.unit_from_u8(x)
    f = torch.zeros((1, 1, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evalops.image_metrics(f, f)
    with pytest.raises(NotImplementedError):
        evalops.image_metrics(f, f, window_size=4)
    assert evalops.METRIC_COLUMNS == ("ssim", "mse", "rmse", "mae", "psnr")


def test_library_exports_the_evaluation_entries():
    from mri_superresolution_amd import _lib
    lib = _lib.load()
    for name in ("mrisr_u8_upscale2", "mrisr_u8_to_unit_f32", "mrisr_image_metrics", "mrisr_metrics_finalize"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    # argument validation happens on the host, before any launch
    assert lib.mrisr_u8_upscale2(None, None, None, 1, 4, 4, 0, None) == -1
    assert lib.mrisr_image_metrics(None, None, None, 1, 4, 4, 1.0, 1.5, 11, None) == -1
