"""Times the GroupNorm + LeakyReLU backward of one node, alone on the chip: two launches (reduce + apply) against the one-pass
kernel, for every node shape of the headline model that takes the one-pass path (plain consumers: act_bwd_onepass_kernel;
a 2x2-pooled encoder node with its skip consumer: act_bwd_onepass_window_kernel).
    python tools/gn_bwd_bench.py [--iters 20] [--batch 16]
With a timing build (tools/build_src_variant.sh pt norm_bwd_onepass.hip -DMRISR_ONEPASS_PT, MRISR_LIB=.../libmrisr_pt.so) it also
prints the share of the middle block's time in each part of the one-pass launch (s_memtime stamps, csrc/norm_bwd_onepass.hip).
"""
import argparse
import ctypes as C
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from mri_superresolution_amd import _lib as L  # noqa: E402

PARTS = ("load", "pre-arrive", "wait", "post-barrier", "store", "dgamma/dbeta")
# (C, H = W, plain consumers, pooled): the decoder / bottleneck nodes, then the three encoder nodes with pool + skip
NODES = [(64, 256, 1, False), (64, 256, 2, False), (128, 128, 1, False), (128, 128, 2, False), (256, 64, 1, False), (512, 32, 1, False),
         (64, 256, 1, True), (128, 128, 1, True), (256, 64, 1, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    dt, tdt = L.BF16, torch.bfloat16
    st = torch.cuda.current_stream().cuda_stream
    lib = L.load()
    SL, words = lib.mrisr_act_bwd_onepass_slots(), lib.mrisr_act_bwd_onepass_barrier_words()
    phases = hasattr(lib, "mrisr_debug_onepass_cycles")
    for (c, hw, ncons, pooled) in NODES:
        n = a.batch
        x = torch.randn(n, hw, hw, c, device=dev).to(tdt)
        das = [torch.randn(n, hw, hw, c, device=dev).to(tdt) for _ in range(ncons)]
        if pooled:
            das.append(torch.randn(n, hw // 2, hw // 2, c, device=dev).to(tdt))
        scale, shift = torch.rand(n * c, device=dev) + 0.5, torch.randn(n * c, device=dev) * 0.1
        mr = torch.stack([torch.zeros(n * 8, device=dev), torch.ones(n * 8, device=dev)], 1).contiguous()
        gamma = torch.ones(c, device=dev)
        carr = (L.Consumer * 2)()
        for i, d in enumerate(das):
            carr[i].da, carr[i].C_total, carr[i].c_off, carr[i].H, carr[i].W = d.data_ptr(), c, 0, d.shape[1], d.shape[2]
            carr[i].spatial, carr[i].off_y, carr[i].off_x, carr[i].weight_mode = (L.SP_POOL2 if d.shape[1] != hw else L.SP_NONE), 0, 0, 0
        dx = torch.empty_like(x)
        dg, db = torch.zeros(c, device=dev), torch.zeros(c, device=dev)
        count = float((c // 8) * hw * hw)
        nb = x.numel() * 2
        nda = sum(d.numel() * 2 for d in das)
        res = []
        for onepass in (False, True, False, True):
            reds = [torch.zeros(SL * n * c * 2 + n * words, device=dev) for _ in range(a.iters + 1)]

            def run(k):
                red = reds[k]
                fin = L.GnBwdFin(red.data_ptr(), gamma.data_ptr(), mr.data_ptr(), dg.data_ptr(), db.data_ptr(), None, None, None, count, 0.0, 8)
                if onepass:
                    arrive = red[SL * n * c * 2:]
                    L.call("mrisr_act_bwd_onepass", dt, x.data_ptr(), scale.data_ptr(), shift.data_ptr(), mr.data_ptr(), len(das), carr,
                           red.data_ptr(), arrive.data_ptr(), C.byref(fin), dx.data_ptr(), n, hw, hw, c, st)
                else:
                    L.call("mrisr_act_bwd_reduce", dt, x.data_ptr(), scale.data_ptr(), shift.data_ptr(), mr.data_ptr(), len(das), carr,
                           None, None, red.data_ptr(), None, n, hw, hw, c, 8, st)
                    L.call("mrisr_act_bwd_apply_fused", dt, x.data_ptr(), scale.data_ptr(), shift.data_ptr(), len(das), carr, None,
                           None, C.byref(fin), dx.data_ptr(), n, hw, hw, c, st)
            run(a.iters)
            torch.cuda.synchronize()
            if phases:
                lib.mrisr_debug_onepass_cycles(None)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(a.iters):
                run(k)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / a.iters
            nbytes = (2 * nb + nda) if onepass else (3 * nb + 2 * nda)
            res.append(f"{'onepass' if onepass else 'twopass'} {us:7.1f} us {nbytes / us / 1e6:5.2f} TB/s")
            if phases and onepass:
                buf = (C.c_ulonglong * 8)()
                lib.mrisr_debug_onepass_cycles(buf)
                tot = max(sum(buf[:6]), 1)
                res.append("[" + ", ".join(f"{name} {100.0 * buf[k] / tot:4.1f}%" for k, name in enumerate(PARTS)) +
                           f"; {tot / max(buf[7], 1):.0f} ticks per launch]")
        print(f"C={c:4d} {hw}^2 x{n} consumers={ncons}{'+pool' if pooled else ''}: " + " | ".join(res), flush=True)


if __name__ == "__main__":
    main()
