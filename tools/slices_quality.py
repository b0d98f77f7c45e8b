#!/usr/bin/env python3
"""The quality table of the slice-to-volume motion correction: the numpy SPECIFICATION on the CPU (no GPU needed), on the structured
phantom of tests/sliceutil.py with per-slice poses uniform within +-1.5 voxels and +-3 degrees (fixed seed).

    python tools/slices_quality.py --factors 2 3 4 --noise 0 20 --rounds 1

Per thickness factor and noise sigma: the truth-RMSE without and with motion correction and their ratio, the RMS corner displacement
of the injected poses and of what is left after the correction (active slices) and their ratio, and the same on unmoved stacks."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (REPO, os.path.join(REPO, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

import sliceutil as U      # noqa: E402


def main(args):
    print("factor noise moved | rmse plain  fixed  ratio | corner mm injected  left  ratio | active slices")
    for factor in args.factors:
        for noise in args.noise:
            for moved in (True, False):
                q = U.quality_case(factor, noise, moved, args.rounds, args.iterations, not args.ellipsoids, args.limit_mm, args.limit_deg)
                ratio = q["residual"] / q["injected"] if q["injected"] else float("nan")
                left = q["residual"] if moved else q["recovered"]
                print(f"{factor:6d} {noise:5g} {str(moved):5s} | {q['rmse_plain']:9.3f} {q['rmse_fixed']:7.3f} {q['rmse_fixed'] / q['rmse_plain']:6.4f} | "
                      f"{q['injected']:17.4f} {left:6.4f} {ratio:6.4f} | {q['active']} of {q['slices']}", flush=True)
    return 0


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Quality of the slice-to-volume motion correction (CPU specification)")
    p.add_argument("--factors", type=int, nargs="+", default=[2, 3, 4])
    p.add_argument("--noise", type=float, nargs="+", default=[0.0, 20.0])
    p.add_argument("--rounds", type=int, default=1)
    p.add_argument("--iterations", type=int, default=4)
    p.add_argument("--limit_mm", type=float, default=3.0)
    p.add_argument("--limit_deg", type=float, default=6.0)
    p.add_argument("--ellipsoids", action="store_true", help="the nearly symmetric phantom of tests/stackutil.py instead of the structured one")
    return p.parse_args(argv)


if __name__ == "__main__":
    sys.exit(main(parse_args()))
