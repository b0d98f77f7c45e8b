"""Launch plumbing that the engine (engine.py), the stand-alone blocks (standalone.py) and the VGG stack (vgg.py) share:
the consumer record of the GroupNorm backward and its marshalling, the input-gradient descriptor, the GroupNorm finalize."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

from . import _lib as L

GN_GROUPS, GN_EPS = 8, 1e-5


@dataclass
class Consumer:
    """One convolution (or the output head) that read an activation, as the activation's backward pass gathers from it:
    ``da`` = dL/d(that reader's input), ``C_total`` channels of which this activation owns the window from ``c_off``;
    H, W, spatial and the padding offsets are how the reader saw it.  ``weight_mode``: 1 / 2 = the alpha blend's two
    branches.  ``head`` (spatial SP_HEAD): the head's (sigmoid output, 1x1 weight, per-image scratch, dW, db)."""
    da: torch.Tensor
    C_total: int
    c_off: int
    H: int
    W: int
    spatial: int
    off_y: int
    off_x: int
    weight_mode: int = 0
    head: Optional[Tuple[torch.Tensor, ...]] = None


def marshal_consumers(consumers: Sequence[Consumer]):
    """The ``Consumer[2]`` array the act_bwd entry points take (one or two used)."""
    if not 1 <= len(consumers) <= 2:
        raise RuntimeError(f"internal: {len(consumers)} consumers of an activation")
    cons = (L.Consumer * 2)()
    for c, k in zip(cons, consumers):
        c.da = k.da.data_ptr()
        c.C_total, c.c_off, c.H, c.W = k.C_total, k.c_off, k.H, k.W
        c.spatial, c.off_y, c.off_x, c.weight_mode = k.spatial, k.off_y, k.off_x, k.weight_mode
        if k.head is not None:
            c.head_out, c.head_w, c.head_part, c.head_dw, c.head_db = (t.data_ptr() for t in k.head)
    return cons


def dgrad_desc(dt: int, dy: torch.Tensor, Cin: int, Cout: int, ks: int, wpacked: torch.Tensor, out: torch.Tensor,
               wpacked_ring: Optional[torch.Tensor] = None, cu_limit: int = 0) -> L.ConvDesc:
    """Input gradient of a convolution Cin -> Cout: the same implicit-GEMM kernel (mrisr_conv_forward) on ``dy``
    (N,H,W,Cout) with the mirrored, transposed weight image ``wpacked``, written to ``out`` (N,H,W,Cin).  The descriptor
    holds addresses only: the caller keeps ``dy``, ``wpacked``, ``wpacked_ring`` and ``out`` alive until the launch is enqueued."""
    N, H, W, _ = dy.shape
    d = L.ConvDesc()
    d.dtype, d.N, d.H, d.W = dt, N, H, W
    d.Cin, d.Cout, d.ksize, d.nsrc = Cout, Cin, ks, 1
    d.combine, d.out_mode, d.groups, d.relu_out = L.COMBINE_CONCAT, L.OUT_PLAIN, 0, 0
    s = d.src[0]
    s.ptr, s.C, s.H, s.W, s.mode, s.spatial = dy.data_ptr(), Cout, H, W, L.SRC_RAW, L.SP_NONE
    d.wpacked, d.wpacked_ring, d.out, d.cu_limit = wpacked.data_ptr(), L.ptr(wpacked_ring), out.data_ptr(), cu_limit
    return d


def gn_finalize(stats: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, N: int, Cc: int, H: int, W: int, stream):
    """GroupNorm statistics of a raw (N,H,W,Cc) tensor -> the per-(n,c) affine its readers apply: (scale, shift, meanrstd)."""
    dev = stats.device
    scale = torch.empty(N * Cc, dtype=torch.float32, device=dev)
    shift = torch.empty(N * Cc, dtype=torch.float32, device=dev)
    meanrstd = torch.empty(N * GN_GROUPS * 2, dtype=torch.float32, device=dev)
    L.call("mrisr_gn_finalize", stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), scale.data_ptr(), shift.data_ptr(),
           meanrstd.data_ptr(), N, Cc, GN_GROUPS, float((Cc // GN_GROUPS) * H * W), GN_EPS, stream)
    return scale, shift, meanrstd
