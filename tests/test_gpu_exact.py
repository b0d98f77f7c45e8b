"""Exact-arithmetic tests (GPU) of every convolution kernel variant: no tolerance, ``torch.equal`` against float64.

The tolerance tests of test_gpu_kernels.py show the kernels are right to the rounding noise of the storage type; a single
missing (pixel, tap, channel) product lies below the bf16 tolerance (tests/test_exact_host.py pins that down).  Here every
such term is visible.

The grid.  Inputs, weights, biases and output gradients are small integers (mostly {-1, 0, 1}; hiputil.dyadic), so every
product is an integer and so is every partial sum.  All kernels accumulate in fp32 (the 16-bit ones multiply bf16 / fp16
operands exactly on the MFMAs), and an fp32 sum of integers is exact and independent of the order of summation, of split-K,
of atomics and of the tile schedule as long as every partial sum stays below 2^24.  Each case asserts that bound ON THE
REFERENCE in its order-independent form: sum |x| |w| over the whole reduction (the conv of the absolute values) < 2^24 grid
units.  The stored result is then the one correct value, and any missing, duplicated or mis-indexed term moves it by at
least one grid unit.

Tier A: the float64 reference is representable in the storage type (hiputil.assert_exact checks that first, so no case can
pass vacuously); nothing is rounded anywhere and the output must equal the reference.  Stored sources, ReLU sources, max-pooled
sources (a max of grid values), the alpha = 0 blend (sigmoid = 1/2 exactly; grid unit 1/2), bias, ReLU, the ReLU mask and
the pixel shuffle (a permutation) are Tier A.  GroupNorm sources with non-negative pre-activations are Tier A too (that is
all MRISR_F32 gets: 0.2f times an integer is not exact in fp32).

Tier B: GroupNorm sources (scale, shift, LeakyReLU in the loader) with negative pre-activations on the 16-bit types.  Scales
in {1, 2} and shifts in {-1, 0, 1} are chosen per channel such that every pre-activation is a small integer and every
NEGATIVE one is -2^k; LeakyReLU then yields RNE_dt(0.2) 2^k on the fp32 route and on the packed 16-bit route alike (205/1024
for bf16, 1638/8192 for fp16).  The accumulators stay exact - sums of multiples of 2^-10 / 2^-13, the same bound in those
units - and the result is rounded ONCE when it is stored: the output must equal the float64 reference rounded once to the
storage type.  Weight gradients of such sources are fp32 and are not rounded at all.  The statistics of Tier B cases stay on
the tolerances of test_gpu_kernels.py.

Statistics.  On Tier A data the GroupNorm sums and sums of squares are integers (multiples of 1/4 for the blend).  Each case
asserts that the reference's per-image, per-group sum of squares is below 2^24 units, so a kernel that reduces in fp32 before
its fp64 atomic is still exact, and then requires the buffer's sum over the slots to EQUAL the reference - the stand-alone
pass over the stored tensor (groups narrower than 4 channels) included.

Accumulate contract.  dw and the statistics are ACCUMULATED (include/mrisr.h): every case starts them from a non-zero
integer pattern and requires pattern + sum exactly.

Guard bands.  Every out, dw, statistics and workspace buffer lies inside a larger allocation with 4 KiB of a sentinel
pattern on both sides (hiputil.Guarded), which must be unchanged after the launch: the ring and producer / consumer kernels
store whole tiles unpredicated, and only their eligibility rules keep those stores inside the tensor.

Smallest qualifying shapes (N, Cin, Cout, H, W; cu_limit shrinks the grid the occupancy rules are checked against):
ring (1,256,128,16,32) at cu_limit 1; producer/consumer 128-channel blocks (1,64,128,8,32) at 1; 64-channel tall tiles
(1,32,64,16,32) at 1; the 32-channel blend (1,32,32,8,32) at 1; 1x1 GEMM (1,32,64,8,16) (no occupancy rule: one 128-pixel tile).

Not here (weights that are not dyadic): the bilinear x2 (MRISR_SP_UP2, mrisr_conv_upadj), the sigmoid
head, the GroupNorm backward.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from mri_superresolution_amd import _lib as L          # noqa: E402
import hiputil as U                                    # noqa: E402

DTS = [L.F32, L.BF16, L.F16]
DTS16 = [L.BF16, L.F16]
LIMIT = float(2 ** 24)
# (scale, shift) of a GroupNorm source over x in {-1, 0, 1}: every negative pre-activation is -1 or -2
AFFINE = [(1., 0.), (2., 0.), (1., -1.), (1., 1.), (2., 1.)]
AFFINE_NONNEG = [(1., 0.), (2., 0.), (1., 1.), (2., 1.)]     # over x in {0, 1}
# present tolerances of the statistics of GroupNorm-source convs (test_gpu_kernels.py: _conv_pc_case)
STAT_RTOL_SUM, STAT_RTOL_SQ = 1e-4, 1e-3


def leaky_unit(dt):
    """Grid unit of LeakyReLU(0.2)(-2^k) in the storage type: RNE_dt(0.2) = 205 / 2^10 (bf16), 1638 / 2^13 (fp16)."""
    return {L.BF16: 2.0 ** -10, L.F16: 2.0 ** -13}[dt]


def raw_src(n, c, h, w, seed, density=0.25, mode=L.SRC_RAW, spatial=L.SP_NONE, off=(0, 0)):
    return U.SrcSpec(U.dyadic((n, c, h, w), seed, density), mode, spatial, off=off)


def norm_src(n, c, h, w, seed, dt, off=(0, 0), nonneg=False):
    """GroupNorm source on the grid.  Returns (SrcSpec, has negative pre-activations)."""
    nonneg = nonneg or dt == L.F32
    x = U.dyadic((n, c, h, w), seed, 0.5)
    table = torch.tensor(AFFINE_NONNEG if nonneg else AFFINE)
    if nonneg:
        x = x.abs()
    pick = torch.randint(len(table), (n, c), generator=torch.Generator().manual_seed(seed + 1000))
    sc, sh = table[pick][..., 0].contiguous(), table[pick][..., 1].contiguous()
    pre = x * sc.view(n, c, 1, 1) + sh.view(n, c, 1, 1)
    neg = pre[pre < 0]
    assert torch.equal(torch.log2(-neg), torch.log2(-neg).round())      # every negative pre-activation is -2^k
    assert not (nonneg and neg.numel())
    return U.SrcSpec(x, L.SRC_NORM, L.SP_NONE, sc, sh, off=off), bool(neg.numel())


def fields(name):
    """Template arguments of a kernel name: "k<a,b,c>" -> ["a", "b", "c"]."""
    return name[name.index("<") + 1:name.rindex(">")].split(",")


def stats_start(n):
    return U.int_pattern((L.STAT_SLOTS, n, 8, 2), torch.float64)


def check_out(out, ref64, dt, tier, what):
    U.assert_exact(out, ref64, dt, tier, what)


def check_stats(stats, stats0, o64, groups_view, tier, unit, what):
    """stats: buffer summed over the slots [N][8][2]; o64: the float64 conv output viewed [N][8][...]."""
    o = o64.reshape(groups_view)
    s_ref, q_ref = o.sum((2, 3, 4)), (o * o).sum((2, 3, 4))
    got = stats - stats0.sum(0)
    if tier == "A":
        assert float((o * o).sum((2, 3, 4)).max()) / (unit * unit) < LIMIT, f"{what}: sum of squares leaves the exact range"
        U.assert_exact(stats[..., 0], s_ref + stats0.sum(0)[..., 0], "f64", "A", what + " sums")
        U.assert_exact(stats[..., 1], q_ref + stats0.sum(0)[..., 1], "f64", "A", what + " sums of squares")
    else:
        assert torch.allclose(got[..., 0], s_ref, rtol=STAT_RTOL_SUM, atol=1e-4 * o.abs().sum((2, 3, 4)).max().item()), what
        assert torch.allclose(got[..., 1], q_ref, rtol=STAT_RTOL_SQ), what


def check_dw(dw, ref64, what):
    U.assert_exact(dw, ref64, L.F32, "A", what)


def forward_case(dt, srcs, w, h, wd, ks, expect, *, tier="A", unit=1.0, stats=True, bias=None, relu_out=0, relu_mask=None,
                 out_mode=L.OUT_PLAIN, combine=L.COMBINE_CONCAT, alpha=None, flip=0, cu_limit=0, use_ring=True):
    """Runs one guarded forward launch and compares it with the float64 reference.  ``expect``: predicate on the kernel name."""
    xin = U.ref_conv_input(srcs, dt, h, wd, combine, alpha).double()
    wt = w.double()
    conv = (lambda a, b: F.conv_transpose2d(a, b, padding=ks // 2)) if flip else (lambda a, b: F.conv2d(a, b, padding=ks // 2))
    ref = conv(xin, wt)
    # order-independent exactness bound: the sum of the absolute values of all terms of any output
    worst = float(conv(xin.abs(), wt.abs()).max()) + (float(bias.abs().max()) if bias is not None else 0.0)
    assert worst / unit < LIMIT, f"partial sums may leave the exact fp32 range: {worst} / {unit}"
    if bias is not None:
        ref = ref + bias.double().view(1, -1, 1, 1)
    pre = ref                                            # the statistics are those of the conv output (+ bias)
    if relu_out:
        ref = F.relu(ref)
    if relu_mask is not None:
        ref = ref * (relu_mask > 0)
    n, cout = ref.shape[:2]
    view = (n, 8, cout // 8, h, wd)
    if out_mode == L.OUT_PIXEL_SHUFFLE2:
        ref, pre = F.pixel_shuffle(ref, 2), F.pixel_shuffle(pre, 2)
        view = (n, 8, cout // 32, 2 * h, 2 * wd)
    stats0 = stats_start(n) if stats else None
    out, st, ran = U.conv_forward_guarded(dt, srcs, w, h, wd, ks, bias=bias, combine=combine, out_mode=out_mode, alpha=alpha,
                                          stats0=stats0, use_ring=use_ring, cu_limit=cu_limit, relu_out=relu_out,
                                          relu_mask=relu_mask, flip=flip)
    assert expect(ran), ran
    check_out(out, ref, dt, tier, ran)
    if stats and not (tier == "B" and (cout // 8) % 4):     # (narrow groups of Tier B: statistics of the ROUNDED tensor)
        check_stats(st, stats0, pre, view, tier, unit, ran)
    return ran


def is_classic(dma=None, ws=None, loader=None, epi=None):
    def pred(name):
        if not name.startswith("conv_igemm_kernel<"):
            return False
        f = fields(name)          # T, BN, loader, KS, WS, EPI, DMA
        return ((dma is None or f[6] == str(dma)) and (ws is None or f[4] == str(ws)) and
                (loader is None or f[2] == str(loader)) and (epi is None or (f[5] != "0") == bool(epi)))
    return pred


def grid_weight(cout, cin, ks, seed, density=0.25):
    return U.dyadic((cout, cin, ks, ks), seed, density)


# ------------------------------------------------------------------------------------------- classic kernel
CLASSIC = {  # n, cins, cout, h, w, cu_limit
    "tiny": (1, (8,), 16, 9, 13, 0),                   # one partial tile, groups of 2 channels (stand-alone statistics pass)
    "cin_tail": (1, (40,), 96, 17, 33, 0),             # Cin no multiple of the chunk: zero-filled channel tail
    "concat_pad": (1, (24, 16), 64, 25, 35, 0),        # concat boundary inside a 64-byte chunk, second source padded
    "narrow_image": (2, (32,), 32, 40, 12, 0),         # tiles narrower than 8 x 32
    "multitile": (3, (64,), 64, 24, 40, 2),            # 2 workgroups x 9 tiles, 6 tiles per image: ranges cross image boundaries
}


def classic_sources(case, mode_of, seed=100):
    n, cins, cout, h, w, cu = CLASSIC[case]
    srcs = []
    for i, c in enumerate(cins):
        hs, ws, off = (h, w, (0, 0)) if i == 0 else (h - 1, w - 2, (0, 1))
        srcs.append(mode_of(n, c, hs, ws, seed + i, off))
    return srcs


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mode", [L.SRC_RAW, L.SRC_RELU])
@pytest.mark.parametrize("case", list(CLASSIC))
def test_classic_kernel_dma_on_and_off(dt, mode, case):
    """conv_igemm_kernel with the LDS-DMA halo path (stored sources) and without it (MRISR_SRC_RELU sources take the vector
    loader), Tier A, statistics included."""
    n, cins, cout, h, w, cu = CLASSIC[case]
    dens = 0.5 if sum(cins) < 32 else 0.25
    srcs = classic_sources(case, lambda n_, c, hs, ws, seed, off: raw_src(n_, c, hs, ws, seed, dens, mode=mode, off=off))
    wt = grid_weight(cout, sum(cins), 3, 110, dens)
    forward_case(dt, srcs, wt, h, w, 3, is_classic(dma=1 if mode == L.SRC_RAW else 0), cu_limit=cu)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", ["cin_tail", "concat_pad", "multitile"])
def test_classic_kernel_norm_sources(dt, case):
    """The vector loader's GroupNorm + LeakyReLU (Tier B on the 16-bit types, non-negative pre-activations in fp32)."""
    n, cins, cout, h, w, cu = CLASSIC[case]
    negs = []

    def mk(n_, c, hs, ws, seed, off):
        s, neg = norm_src(n_, c, hs, ws, seed, dt, off)
        negs.append(neg)
        return s
    srcs = classic_sources(case, mk, seed=120)
    assert all(negs) == (dt != L.F32)
    tier, unit = ("B", leaky_unit(dt)) if dt != L.F32 else ("A", 1.0)
    forward_case(dt, srcs, grid_weight(cout, sum(cins), 3, 130), h, w, 3, is_classic(dma=0), tier=tier, unit=unit, cu_limit=cu)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape,ks", [((1, 224, 32, 20, 40), 3), ((1, 288, 64, 20, 40), 3), ((2, 800, 64, 12, 20), 1),
                                      ((1, 832, 24, 9, 33), 1)])
def test_streamed_weight_images(dt, shape, ks):
    """Weight images that do not fit LDS next to the halo tiles are streamed in 1-KiB pieces (WS = 0 in the kernel name).
    (1,832,24,9,33): only the fp32 image (52 chunks) is streamed, the 16-bit ones (26 chunks of 2 KiB) are stationary."""
    n, cin, cout, h, w = shape
    streamed = not (cin == 832 and dt != L.F32)
    forward_case(dt, [raw_src(n, cin, h, w, 140)], grid_weight(cout, cin, ks, 141), h, w, ks,
                 is_classic(dma=1, ws=0 if streamed else 1))


EPILOGUES = [("bias", 3), ("relu_out", 3), ("relu_mask", 3), ("pixel_shuffle", 3), ("dgrad", 3), ("pool", 3), ("blend", 3),
             ("src_relu", 3), ("bias", 1), ("relu_out", 1), ("dgrad", 1), ("src_relu", 1)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind,ks", EPILOGUES)
def test_epilogues_and_operands(dt, kind, ks):
    """Integer bias, ReLU, ReLU mask, pixel shuffle, the input-gradient operand, pooled / blended / ReLU sources on the
    classic 3x3 and 1x1 kernels - all Tier A."""
    n, cin, cout, h, w = 2, 16, 32, 11, 19
    wt = grid_weight(cout, cin, ks, 150, 0.5)
    bias = U.dyadic((cout,), 151, 0.75, values=(-3, -2, -1, 1, 2, 3))
    kw, expect = {}, is_classic(epi=0)
    srcs = [raw_src(n, cin, h, w, 152, 0.5)]
    if kind == "bias":
        kw = dict(bias=bias)
    elif kind == "relu_out":
        kw = dict(bias=bias, relu_out=1, stats=False)
    elif kind == "relu_mask":
        kw = dict(relu_mask=U.dyadic((n, cout, h, w), 153, 0.6, values=(-1, 1, 2)), stats=False)
        expect = is_classic(epi=1)
    elif kind == "pixel_shuffle":
        kw = dict(bias=bias, out_mode=L.OUT_PIXEL_SHUFFLE2)
        expect = is_classic(epi=1)
    elif kind == "dgrad":      # sources carry the forward conv's Cout channels, the result its Cin
        srcs = [raw_src(n, cout, h, w, 154, 0.5)]
        kw = dict(flip=1, stats=False)
    elif kind == "pool":
        srcs = [raw_src(n, cin, 2 * h, 2 * w + 1, 155, 0.5, spatial=L.SP_POOL2)]
        expect = is_classic(loader=L.SP_POOL2, dma=0)
    elif kind == "blend":
        srcs = [raw_src(n, cin, h, w, 156 + i, 0.5) for i in range(2)]
        kw = dict(combine=L.COMBINE_BLEND, alpha=torch.tensor(0.0), unit=0.5)
        expect = is_classic(loader=3, dma=0)
    else:
        srcs = [raw_src(n, cin, h, w, 158, 0.5, mode=L.SRC_RELU)]
        expect = is_classic(dma=0)
    forward_case(dt, srcs, wt, h, w, ks, expect, **kw)


# ------------------------------------------------------------------------------------------- ring kernel
RING = {  # n, cin, cout, plane, source, offset, cu_limit
    "one_tile": (1, 256, 128, (16, 32), (16, 32), (0, 0), 1),            # the smallest launch that qualifies
    "multi_tile_stats": (3, 256, 128, (16, 96), (16, 96), (0, 0), 2),    # 9 tiles on 2 workgroups (5 + 4): image changes inside
    "padded_offset": (1, 256, 256, (32, 64), (29, 57), (1, 4), 4),       # halo pixels outside the source: the zero block
    "cin272_bias_relu": (1, 272, 128, (16, 64), (16, 64), (0, 0), 2),    # 17 chunks; bias + ReLU epilogue, no statistics
}


@pytest.mark.parametrize("dt", DTS16)
@pytest.mark.parametrize("case", list(RING))
def test_ring_kernel(dt, case):
    """conv_ring_kernel (unpredicated 16 x 32 x 128 tile stores) and the classic kernel on the same descriptor: both equal
    to the float64 reference."""
    n, cin, cout, (h, w), (hs, ws), off, cu = RING[case]
    srcs = [raw_src(n, cin, hs, ws, 160, off=off)]
    wt = grid_weight(cout, cin, 3, 161)
    kw = dict(cu_limit=cu)
    if case == "cin272_bias_relu":
        kw.update(bias=U.dyadic((cout,), 162, 0.75, values=(-3, -2, -1, 1, 2, 3)), relu_out=1, stats=False)
    forward_case(dt, srcs, wt, h, w, 3, lambda name: name.startswith("conv_ring_kernel<"), **kw)
    forward_case(dt, srcs, wt, h, w, 3, is_classic(dma=1), use_ring=False, **kw)


# ------------------------------------------------------------------------------------------- producer / consumer kernel
PC = {  # kind, n, cins, cout, h, w, norm, cu_limit, bias + relu
    # 128-channel blocks
    "k4_norm_one_tile": (4, 1, (64,), 128, 8, 32, True, 1, False),             # the smallest launch that qualifies
    "k4_raw_image_change": (4, 3, (144,), 128, 24, 32, False, 2, False),       # 9 tiles on 2 workgroups; 9 chunks: 45 / 36 items
    "k4_norm_concat_chunk_switch": (4, 2, (48, 32), 128, 16, 64, True, 4, False),   # sources switch at chunk 3; second one padded
    "k4_raw_odd_items": (4, 1, (176,), 128, 24, 32, False, 1, False),          # 3 tiles x 11 chunks = 33 items: the padding half
    "k4_raw_bias_relu": (4, 1, (144,), 128, 8, 64, False, 2, True),
    # 64-channel blocks on tall (16 x 32) tiles
    "k2_norm_one_tile": (2, 1, (32,), 64, 16, 32, True, 1, False),
    "k2_norm_192": (2, 1, (32,), 192, 16, 64, True, 4, False),                 # three 64-channel blocks
    "k2_raw_odd_items_image_change": (2, 3, (176,), 64, 16, 32, False, 1, False),
    "k2_norm_concat_chunk_switch": (2, 2, (48, 32), 64, 16, 64, True, 4, False),
}


@pytest.mark.parametrize("dt", DTS16)
@pytest.mark.parametrize("case", list(PC))
def test_producer_consumer_kernel(dt, case):
    """conv_pc_kernel, 128-channel blocks (kind 4) and 64-channel blocks on tall tiles (kind 2): GroupNorm sources are Tier B,
    stored sources Tier A with exact statistics; the classic kernel on the same descriptor must equal the reference too."""
    kind, n, cins, cout, h, w, norm, cu, bias_relu = PC[case]
    srcs, tier, unit = [], "A", 1.0
    for i, c in enumerate(cins):
        hs, ws, off = (h, w, (0, 0)) if i == 0 else (h - 3, w - 5, (1, 2))
        if norm:
            s, neg = norm_src(n, c, hs, ws, 170 + i, dt, off)
            assert neg
            tier, unit = "B", leaky_unit(dt)
        else:
            s = raw_src(n, c, hs, ws, 170 + i, off=off)
        srcs.append(s)
    wt = grid_weight(cout, sum(cins), 3, 175)
    kw = dict(cu_limit=cu, tier=tier, unit=unit)
    if bias_relu:
        kw.update(bias=U.dyadic((cout,), 176, 0.75, values=(-3, -2, -1, 1, 2, 3)), relu_out=1, stats=False)
    tail = ",64>" if kind == 2 else f",{1 if norm else 0}>"
    forward_case(dt, srcs, wt, h, w, 3, lambda name: name.startswith("conv_pc_kernel<") and name.endswith(tail), **kw)
    forward_case(dt, srcs, wt, h, w, 3, is_classic(dma=0 if norm else 1), use_ring=False, **kw)


@pytest.mark.parametrize("dt", DTS16)
@pytest.mark.parametrize("case", ["tall_image_change", "short_tiles", "one_tile"])
def test_producer_consumer_blend(dt, case):
    """conv_pc_kernel's 32-channel blend variant (kind 1): two GroupNorm sources blended by the staging waves at alpha = 0.
    Non-negative pre-activations keep sigmoid(0) (a + b) = (a + b) / 2 on the half-integer grid: Tier A, exact statistics
    (groups of 4 channels)."""
    n, h, w, cu = {"tall_image_change": (2, 16, 64, 1),      # 4 tall items in one workgroup, 2 per image
                   "short_tiles": (1, 24, 32, 1),            # 24 rows: the 8 x 32 items
                   "one_tile": (1, 8, 32, 1)}[case]          # the smallest launch that qualifies
    cin = cout = 32
    srcs = [norm_src(n, cin, h, w, 180 + i, dt, nonneg=True)[0] for i in range(2)]
    wt = grid_weight(cout, cin, 3, 183)
    kw = dict(combine=L.COMBINE_BLEND, alpha=torch.tensor(0.0), unit=0.5, cu_limit=cu)
    forward_case(dt, srcs, wt, h, w, 3, lambda name: name.startswith("conv_pc_kernel<") and name.endswith(",1>"), **kw)
    forward_case(dt, srcs, wt, h, w, 3, is_classic(loader=3, dma=0), use_ring=False, **kw)


# ------------------------------------------------------------------------------------------- 1x1 GEMM
C1X1 = {  # n, cin, cout, h, w, norm, dgrad operand, cu_limit
    "norm_wide": (1, 64, 256, 8, 32, True, False, 1),                # 256-channel blocks (2 tiles fill "1 CU" twice over)
    "norm_narrow": (1, 32, 64, 8, 16, True, False, 0),               # the smallest launch that qualifies: one tile, one block
    "raw_dgrad": (2, 64, 128, 8, 16, False, True, 1),                # stored source, mirrored operand, 128-channel blocks
    "two_images_per_few_tiles": (2, 32, 128, 8, 16, True, False, 0),  # one tile per image
}


@pytest.mark.parametrize("dt", DTS16)
@pytest.mark.parametrize("case", list(C1X1))
def test_conv1x1_gemm(dt, case):
    n, cin, cout, h, w, norm, dgrad, cu = C1X1[case]
    tier, unit = "A", 1.0
    if norm:
        s, neg = norm_src(n, cin, h, w, 190, dt)
        assert neg
        srcs, tier, unit = [s], "B", leaky_unit(dt)
    else:
        srcs = [raw_src(n, cin, h, w, 190)]
    wt = grid_weight(cin, cout, 1, 191, 0.5) if dgrad else grid_weight(cout, cin, 1, 191, 0.5)
    kw = dict(tier=tier, unit=unit, cu_limit=cu, flip=1 if dgrad else 0)
    tail = f",{1 if norm else 0}>"
    forward_case(dt, srcs, wt, h, w, 1, lambda name: name.startswith("conv1x1_gemm_kernel<") and name.endswith(tail),
                 stats=False, **kw)
    # with statistics requested the launch takes the classic kernel
    forward_case(dt, srcs, wt, h, w, 1, is_classic(dma=0 if norm else 1), stats=True, **kw)


# ------------------------------------------------------------------------------------------- stem
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cin", [0, 1, 2, 3, 4])
def test_stem_forward_and_wgrad(dt, cin):
    """mrisr_stem_forward (cin = 0 here) and mrisr_stem_forward_multi for 1..4 image channels, with their weight gradients,
    on an odd plane: integer image, weights and output gradient."""
    single, cin = cin == 0, max(cin, 1)
    n, cout, h, w = 2, 32, 11, 21
    x = U.dyadic((n, cin, h, w), 200, 0.6, values=(-2, -1, 1, 2))
    wt = U.dyadic((cout, cin, 3, 3), 201, 0.6)
    ref = F.conv2d(x.double(), wt.double(), padding=1)
    xd, wd = x.to(U.DEV).contiguous(), wt.permute(0, 2, 3, 1).contiguous().to(U.DEV)        # [Cout][9][Cin]
    out = U.Guarded(torch.full((n, h, w, cout), float("nan"), dtype=U.tdt(dt)))
    stats0 = stats_start(n)
    stats = U.Guarded(stats0)
    if single:
        L.call("mrisr_stem_forward", dt, xd.data_ptr(), wd.data_ptr(), out.data_ptr(), stats.data_ptr(), n, h, w, cout, 8, U.stream())
    else:
        L.call("mrisr_stem_forward_multi", dt, xd.data_ptr(), wd.data_ptr(), out.data_ptr(), stats.data_ptr(), n, h, w, cin, cout, 8,
               U.stream())
    torch.cuda.synchronize()
    out.check("stem out")
    stats.check("stem stats")
    check_out(U.nchw(out.t), ref, dt, "A", "stem forward")
    check_stats(stats.t.cpu().sum(0), stats0, ref, (n, 8, cout // 8, h, w), "A", 1.0, "stem")
    # weight gradient, accumulated onto a non-zero start
    dy = U.dyadic((n, cout, h, w), 202, 0.25)
    wr = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wr, padding=1).backward(dy.double())
    wa = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().abs(), wa, padding=1).backward(dy.double().abs())
    assert float(wa.grad.max()) + 3 < LIMIT
    dw0 = U.int_pattern((cout, cin, 3, 3), torch.float32)
    dw = U.Guarded(dw0.permute(0, 2, 3, 1).contiguous())
    dyd = U.nhwc(dy, dt)
    if single:
        L.call("mrisr_stem_wgrad", dt, xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), n, h, w, cout, U.stream())
    else:
        L.call("mrisr_stem_wgrad_multi", dt, xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), n, h, w, cin, cout, U.stream())
    torch.cuda.synchronize()
    dw.check("stem dw")
    check_dw(dw.t.cpu().permute(0, 3, 1, 2), wr.grad + dw0.double(), "stem wgrad")


# ------------------------------------------------------------------------------------------- weight gradients
def wgrad_case(dt, srcs, n, cin, cout, h, w, ks, use_ws, expect, unit=1.0, cu_limit=0, dy_density=0.25, seed=210):
    dy = U.dyadic((n, cout, h, w), seed, dy_density)
    xin = U.ref_conv_input(srcs, dt, h, w).double()
    wr = torch.zeros(cout, cin, ks, ks, dtype=torch.float64, requires_grad=True)
    F.conv2d(xin, wr, padding=ks // 2).backward(dy.double())
    wa = torch.zeros(cout, cin, ks, ks, dtype=torch.float64, requires_grad=True)
    F.conv2d(xin.abs(), wa, padding=ks // 2).backward(dy.double().abs())
    dw0 = U.int_pattern((cout, cin, ks, ks), torch.float32)
    # max |dw| < 2^24 grid units, in the order-independent form (sum of |terms| + the start value)
    worst = float(wa.grad.max()) + float(dw0.abs().max())
    assert worst / unit < LIMIT, f"partial sums may leave the exact fp32 range: {worst} / {unit}"
    dw, ran = U.conv_wgrad_guarded(dt, srcs, dy, cout, cin, h, w, ks, dw0, use_ws=use_ws, cu_limit=cu_limit)
    assert expect(ran), ran
    check_dw(dw, wr.grad + dw0.double(), f"{ran} use_ws={use_ws}")


def wgrad_norm(n, c, h, w, seed, dt, off=(0, 0)):
    s, neg = norm_src(n, c, h, w, seed, dt, off)
    assert neg == (dt != L.F32)
    return s


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("use_ws", [False, True])
@pytest.mark.parametrize("case", ["raw", "pool", "concat", "k1", "fast1", "fast2", "fast4"])
def test_conv_wgrad_classic(dt, case, use_ws):
    """conv_wgrad_kernel (generic and the unrolled FAST variants) with float atomics and with the two-stage workspace
    reduction.  The shapes keep out of the row kernel's domain (Cin no multiple of 32, a pooled source, 1x1, planes lower than
    16 rows; k1 takes a plain source here, the bilinear x2 of the tolerance test's k1 case is not dyadic); fast*: 18 tiles on a split-K of 4 (cu_limit), several tiles per workgroup.  GroupNorm sources: the fp32 dw of
    Tier B data is exact in units of RNE(0.2)'s last bit."""
    cu, ks, fast, loader = 0, 3, 0, 0
    unit = 1.0 if dt == L.F32 else leaky_unit(dt)
    if case.startswith("fast"):
        cin, cout, cu = {"fast1": (64, 128, 8), "fast2": (64, 32, 4), "fast4": (32, 32, 4)}[case]
        n, h, w = 3, 12, 72
        fast = 0 if dt == L.F32 else int(case[4])
        srcs = [wgrad_norm(n, cin, h, w, 220, dt)]
    elif case == "raw":
        n, cin, cout, h, w = 2, 40, 96, 21, 37
        srcs = [wgrad_norm(n, cin, h, w, 221, dt)]
    elif case == "pool":
        n, cin, cout, h, w, loader = 2, 32, 64, 12, 17, L.SP_POOL2
        s = wgrad_norm(n, cin, 24, 35, 222, dt)
        s.spatial = L.SP_POOL2
        srcs = [s]
    elif case == "concat":
        n, cin, cout, h, w = 2, 48, 32, 17, 33
        srcs = [wgrad_norm(n, 32, h, w, 223, dt), wgrad_norm(n, 16, 16, 32, 224, dt, off=(1, 1))]
    else:
        n, cin, cout, h, w, ks = 2, 64, 32, 20, 28, 1
        srcs = [wgrad_norm(n, cin, h, w, 225, dt)]
    t = {L.F32: "f32", L.BF16: "bf16", L.F16: "f16"}[dt]
    name = f"conv_wgrad_kernel<{t},{loader},{ks},{fast}>"
    wgrad_case(dt, srcs, n, cin, cout, h, w, ks, use_ws, lambda ran: ran == name, unit=unit, cu_limit=cu, dy_density=0.1)


@pytest.mark.parametrize("dt", DTS16)
@pytest.mark.parametrize("use_ws", [False, True])
@pytest.mark.parametrize("case", ["norm_edges", "raw_wide", "concat_pad", "deep_small", "narrow_raw_32x32", "narrow_64to32",
                                  "narrow_32to64_norm"])
def test_conv_wgrad_rows(dt, case, use_ws):
    """conv_wgrad_rows_kernel: the case kinds of test_gpu_kernels.py's test_conv_wgrad_rows at reduced planes.  norm_edges: 12
    tiles on a split-K of 4 (cu_limit), three tiles per workgroup."""
    cu, unit = 0, 1.0
    if case == "norm_edges":
        n, cin, cout, h, w, cu = 2, 64, 128, 24, 40, 8
        srcs = [wgrad_norm(n, cin, h, w, 230, dt)]
    elif case == "raw_wide":
        n, cin, cout, h, w = 2, 128, 64, 16, 32
        srcs = [raw_src(n, cin, h, w, 231)]
    elif case == "concat_pad":
        n, cin, cout, h, w = 1, 128, 64, 17, 19
        srcs = [wgrad_norm(n, 64, h, w, 232, dt), wgrad_norm(n, 64, 16, 17, 233, dt, off=(0, 1))]
    elif case == "deep_small":
        n, cin, cout, h, w = 4, 256, 128, 16, 16
        srcs = [wgrad_norm(n, cin, h, w, 234, dt)]
    elif case == "narrow_raw_32x32":
        n, cin, cout, h, w = 2, 32, 32, 24, 40
        srcs = [raw_src(n, cin, h, w, 235)]
    elif case == "narrow_64to32":
        n, cin, cout, h, w = 1, 64, 32, 33, 48
        srcs = [raw_src(n, cin, h, w, 236)]
    else:
        n, cin, cout, h, w = 2, 32, 64, 24, 40
        srcs = [wgrad_norm(n, cin, h, w, 237, dt)]
    raw = all(s.mode == L.SRC_RAW for s in srcs)
    if not raw:
        unit = leaky_unit(dt)
    t = {L.BF16: "bf16", L.F16: "f16"}[dt]
    name = f"conv_wgrad_rows_kernel<{t},{1 if cout % 64 else 2},{1 if cin % 64 else 2},{1 if raw else 0}>"
    wgrad_case(dt, srcs, n, cin, cout, h, w, 3, use_ws, lambda ran: ran == name, unit=unit, cu_limit=cu,
               dy_density=0.25 if raw else 0.1)


# ------------------------------------------------------------------------------------------- packers
@pytest.mark.parametrize("dt", DTS)
def test_pack_weights_batched_equals_single_jobs(dt):
    """mrisr_pack_weights_batched (the launch that runs after every optimiser step) over one job list that mixes the forward,
    mirrored, ring and upadj operands of four layer shapes must fill buffers byte-identical to one mrisr_pack_weights call per
    job; both sides start from zero-filled buffers so that padding compares equal."""
    lib = L.load()
    layers = [(128, 256, 3), (64, 40, 3), (16, 32, 3), (64, 832, 1)]      # (Cout, Cin, k): ring both ways; Cin tail; upadj; 1x1
    jobs_spec = []
    for li, (co, ci, ks) in enumerate(layers):
        for flip in (0, 1):
            oc, ic = (ci, co) if flip else (co, ci)
            jobs_spec.append((li, flip, lib.mrisr_packed_weight_bytes(dt, oc, ic, ks)))
            if lib.mrisr_conv_ring_bn(dt, oc, ic, ks) > 0:
                jobs_spec.append((li, flip | L.PACK_RING, lib.mrisr_packed_weight_bytes_ring(dt, oc, ic, ks)))
        if lib.mrisr_packed_weight_bytes_upadj(dt, co, ci, ks) > 0:
            jobs_spec.append((li, L.PACK_UPADJ, lib.mrisr_packed_weight_bytes_upadj(dt, co, ci, ks)))
    kinds = {f & (L.PACK_RING | L.PACK_UPADJ) for _, f, _ in jobs_spec}
    assert kinds == ({0, L.PACK_RING, L.PACK_UPADJ} if dt != L.F32 else {0})
    masters = [U.w_cl(torch.randn(co, ci, ks, ks, generator=torch.Generator().manual_seed(240 + i)))
               for i, (co, ci, ks) in enumerate(layers)]
    single, batched = [], []
    jobs = (L.PackJob * len(jobs_spec))()
    for i, (li, flag, nbytes) in enumerate(jobs_spec):
        co, ci, ks = layers[li]
        assert nbytes > 0
        one = torch.zeros(nbytes, dtype=torch.uint8, device=U.DEV)
        L.call("mrisr_pack_weights", dt, masters[li].data_ptr(), co, ci, ks, flag, one.data_ptr(), U.stream())
        single.append(one)
        buf = U.Guarded(torch.zeros(nbytes, dtype=torch.uint8))
        batched.append(buf)
        j = jobs[i]
        j.w, j.packed, j.Cout, j.Cin, j.ksize, j.transpose_flip = masters[li].data_ptr(), buf.data_ptr(), co, ci, ks, flag
    jobs_dev = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(U.DEV)
    L.call("mrisr_pack_weights_batched", dt, jobs_dev.data_ptr(), len(jobs_spec), U.stream())
    torch.cuda.synchronize()
    for (li, flag, nbytes), one, buf in zip(jobs_spec, single, batched):
        buf.check(f"packed image of layer {layers[li]} flags {flag}")
        assert one.any(), (layers[li], flag)
        diff = (one != buf.t).nonzero()
        assert diff.numel() == 0, f"layer {layers[li]} flags {flag}: {diff.numel()} of {nbytes} bytes differ, first at {int(diff[0])}"
