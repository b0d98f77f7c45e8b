"""The HIP-event timing loops that several per-tool benchmarks under ``tools/`` share, each as it stood in those tools.  ``bench.py``
does not use this module."""
import statistics

import torch


def alternating_times(fns, reps, warmup, inner, digits=1):
    """``fns``: name -> callable.  ``reps`` rounds; in each round every callable in turn is timed over ``inner`` calls between two
    events, so that drift hits all of them alike -> name -> microseconds per call (median, min, max), rounded to ``digits``."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / inner)
    return {k: {"us_median": round(statistics.median(v), digits), "us_min": round(min(v), digits), "us_max": round(max(v), digits)}
            for k, v in times.items()}


def alternating_times_fine(fns, reps, warmup, inner):
    """``alternating_times`` rounded to two decimals: the kernels of ``intensity_bench`` and ``register_bench`` take microseconds."""
    return alternating_times(fns, reps, warmup, inner, digits=2)


def timed(fn, iters, warmup):
    """ms per call: device events around the whole loop."""
    for _ in range(warmup):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def event_times(fn, reps, warmup):
    """Every call between two events of its own -> microseconds (median, min)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return {"us_median": round(statistics.median(times), 1), "us_min": round(min(times), 1)}
