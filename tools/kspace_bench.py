#!/usr/bin/env python3
"""Cost of the circulant kernels (csrc/volume_kspace.hip) next to the same operators written with torch.fft, and next to a copy.

    python tools/kspace_bench.py [--size 256] [--reps 5] [--warmup 2] [--inner 3] [--window none]

(a) ``zerofill2`` of a size^3 float32 volume over all three axes (three launches; 256^3 -> 512^3) and ``truncate2`` of a (2 size)^3
    volume (512^3 -> 256^3), HIP events, the median of ``--reps`` alternating rounds;
(b) the same results by ``torch.fft``: ``rfftn``, the phase ramp of the quarter-sample shift and the Nyquist split per axis,
    zero-padding (or cropping) of the spectrum, ``irfftn`` - the index and ramp tensors are made before the clock starts; the largest
    absolute difference between the two results is printed next to the data range;
(c) a device copy of the ALGORITHMIC bytes of each operator - the source read once, the result written once.
The kernel costs O(n) per output where the FFT costs O(log n): its multiply-add pairs per call are printed, and the rate they
run at.  Prints one JSON line (README.md, "Zero-filling and k-space truncation")."""
import argparse
import json
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.benchutil import alternating_times      # noqa: E402


def _weights(n, window, device):
    """w_|k| in torch.fft's bin order, float64."""
    k = torch.fft.fftfreq(n, 1.0 / n, dtype=torch.float64, device=device).abs()
    return torch.ones_like(k) if window == "none" else 0.54 + 0.46 * torch.cos(math.pi * k / ((n + 1) // 2))


def _full_axis(n, window, device, up):
    """(source bins, destination bins, multipliers) of one full (c2c) axis: ``up`` pads n bins into 2n with the ramp of the shift
    by -1/4 sample, else crops the 2n bins of the fine grid to n with the ramp of +1/2 fine sample; an even n splits its Nyquist
    bin over +-n/2."""
    k = torch.fft.fftfreq(n, 1.0 / n, dtype=torch.float64, device=device)
    w = _weights(n, window, device)
    period = 2 * n
    angle = -2 * math.pi * k * 0.25 / n if up else math.pi * k / period
    mult = w * torch.exp(1j * angle)
    kk = k.to(torch.int64)
    src, dst = (torch.arange(n, device=device), kk % period) if up else (kk % period, torch.arange(n, device=device))
    if n % 2 == 0:
        h = n // 2                                                # bin h holds k = -n/2; its other half goes to / comes from +n/2
        mult[h] = mult[h] * 0.5
        src = torch.cat([src, src.new_tensor([h])])
        dst = torch.cat([dst, dst.new_tensor([h])])
        mult = torch.cat([mult, torch.conj(mult[h:h + 1])])
    return src, dst, mult.to(torch.complex64)


def _half_axis(n, window, device, up):
    """Multipliers of the rfft axis, bins 0 .. n // 2.  Up: an even n's Nyquist bin keeps half of itself (irfftn implies the other
    half); down: it stays whole, and the c2r transform's Hermitian projection adds the two halves."""
    k = torch.arange(n // 2 + 1, dtype=torch.float64, device=device)
    w = _weights(n, window, device)[:n // 2 + 1]
    mult = w * torch.exp(1j * (-2 * math.pi * k * 0.25 / n if up else math.pi * k / (2 * n)))
    if up and n % 2 == 0:
        mult[-1] = mult[-1] * 0.5
    return mult.to(torch.complex64)


def make_zerofill_fft(shape, window, device):
    n0, n1, n2 = shape
    a0, a1, m2 = _full_axis(n0, window, device, True), _full_axis(n1, window, device, True), _half_axis(n2, window, device, True)

    def run(v):
        spec = torch.fft.rfftn(v) * m2
        y = spec.new_zeros((2 * n0, n1, n2 // 2 + 1)).index_add_(0, a0[1], spec[a0[0]] * a0[2][:, None, None])
        z = spec.new_zeros((2 * n0, 2 * n1, n2 + 1))
        z[:, :, :n2 // 2 + 1].index_add_(1, a1[1], y[:, a1[0]] * a1[2][None, :, None])
        return torch.fft.irfftn(z, s=(2 * n0, 2 * n1, 2 * n2)) * 8.0
    return run


def make_truncate_fft(shape, window, device):
    n0, n1, n2 = (d // 2 for d in shape)
    a0, a1, m2 = _full_axis(n0, window, device, False), _full_axis(n1, window, device, False), _half_axis(n2, window, device, False)

    def run(v):
        spec = torch.fft.rfftn(v)[:, :, :n2 // 2 + 1] * m2
        y = spec.new_zeros((n0, 2 * n1, n2 // 2 + 1)).index_add_(0, a0[1], spec[a0[0]] * a0[2][:, None, None])
        z = spec.new_zeros((n0, n1, n2 // 2 + 1)).index_add_(1, a1[1], y[:, a1[0]] * a1[2][None, :, None])
        return torch.fft.irfftn(z, s=(n0, n1, n2)) * 0.125
    return run


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=256, help="the coarse extent n: zerofill2 n^3 -> (2n)^3, truncate2 (2n)^3 -> n^3")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--inner", type=int, default=3)
    p.add_argument("--window", type=str, choices=["none", "hamming"], default="none")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kspace_bench needs the MI355X: there is nothing to time on a CPU")
    from mri_superresolution_amd.volume_kspace import truncate2, zerofill2

    n, dev = args.size, torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    coarse = torch.rand((n, n, n), device=dev, generator=g) * 4095.0
    fine = torch.rand((2 * n, 2 * n, 2 * n), device=dev, generator=g) * 4095.0
    up_fft, down_fft = make_zerofill_fft(coarse.shape, args.window, dev), make_truncate_fft(fine.shape, args.window, dev)
    up_out, down_out = torch.empty_like(fine), torch.empty_like(coarse)
    words = coarse.numel() + fine.numel()
    copy_src, copy_dst = torch.empty(words // 2, device=dev), torch.empty(words // 2, device=dev)      # reads and writes 4 * words bytes
    res = {"gpu": torch.cuda.get_device_name(0), "size": n, "window": args.window, "reps": args.reps, "inner": args.inner}
    res["max_abs_diff"] = {"zerofill2": float((zerofill2(coarse, window=args.window) - up_fft(coarse)).abs().max()),
                           "truncate2": float((truncate2(fine, window=args.window) - down_fft(fine)).abs().max()), "data_range": 4095.0}
    fns = {"zerofill2": lambda: zerofill2(coarse, window=args.window, out=up_out), "zerofill_fft": lambda: up_fft(coarse),
           "truncate2": lambda: truncate2(fine, window=args.window, out=down_out), "truncate_fft": lambda: down_fft(fine),
           "copy": lambda: copy_dst.copy_(copy_src)}
    res["times"] = alternating_times(fns, args.reps, args.warmup, args.inner)
    t = {k: v["us_median"] for k, v in res["times"].items()}
    # multiply-add pairs: per pass, outputs times the line's source samples
    pairs_up = sum(n ** 3 * 2 ** (a + 1) * n for a in range(3))
    pairs_down = sum((2 * n) ** 3 // 2 ** (a + 1) * (2 * n) for a in range(3))
    for name, fft, pairs in (("zerofill2", "zerofill_fft", pairs_up), ("truncate2", "truncate_fft", pairs_down)):
        res[name] = {"ms": round(t[name] / 1e3, 3), "over_fft": round(t[name] / t[fft], 3), "over_copy": round(t[name] / t["copy"], 3),
                     "G_pairs": round(pairs / 1e9, 2), "T_pairs_per_s": round(pairs / (t[name] * 1e-6) / 1e12, 3)}
    res["copy_TBps"] = round(4 * words / (t["copy"] * 1e-6) / 1e12, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
