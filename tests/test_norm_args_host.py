"""Argument checks of the GroupNorm + LeakyReLU backward entry points (csrc/norm_bwd*.hip), without a GPU.

Every check of these entries happens before the first HIP call and a device pointer is never dereferenced on the host, so
small non-zero integers serve as pointers.  Each row below is a call that would be valid but for ONE defect; the expected
return code is the one the library gave before the host side of these files was reorganised, and no row may reach a launch
(no expected code is MRISR_E_HIP).  The rows of a dtype the library does not know reach the end of the checks: they pin that
nothing is launched for it either."""
import ctypes as C
from types import SimpleNamespace

import pytest

from mri_superresolution_amd import _lib
from mri_superresolution_amd._lib import BF16, F32, SP_HEAD, SP_NONE, SP_POOL2, SP_UP2, BlendBranch, Consumer, GnBwdFin

E_ARG, E_SHAPE, E_DTYPE, E_UNSUPPORTED = -1, -2, -3, -5      # (-4, MRISR_E_HIP, would mean that a row reached a launch)
OUT_PLAIN, OUT_PIXEL_SHUFFLE2 = 0, 1


def P(k):
    """A distinct fake device pointer."""
    return 0x10000 * (k + 1)


def _base():
    """The arguments of a valid call: a bf16 node [2][8][8][16], 8 groups, one plain consumer with the node's geometry."""
    a = SimpleNamespace(dtype=BF16, N=2, H=8, W=8, C=16, groups=8, count=128.0, out_mode=OUT_PLAIN)
    a.x, a.scale, a.shift, a.meanrstd, a.red, a.g, a.dx, a.arrive = (P(k) for k in range(8))
    a.gamma, a.dgamma, a.dbeta, a.coef_out, a.da, a.dx2 = (P(k) for k in range(8, 14))
    a.blend_alpha = a.alpha_slots = a.coef = a.dbias = a.alpha = a.dalpha = None
    a.consumers, a.ncons = True, 1
    a.cons0 = Consumer(da=P(20), C_total=16, c_off=0, H=8, W=8, spatial=SP_NONE)
    a.cons1 = Consumer(da=P(21), C_total=16, c_off=0, H=8, W=8, spatial=SP_NONE)
    a.fin = GnBwdFin(red=a.red, gamma=a.gamma, meanrstd=a.meanrstd, dgamma=a.dgamma, dbeta=a.dbeta, count=128.0, alpha_sign=1.0, groups=8)
    # the blend pair: two branches with their own sums and slots, and the fin of each
    a.ps = BlendBranch(x=P(30), scale=P(31), shift=P(32), meanrstd=P(33), red=P(34), alpha_slots=P(35), weight_mode=1)
    a.bil = BlendBranch(x=P(40), scale=P(41), shift=P(42), meanrstd=P(43), red=P(44), alpha_slots=P(45), weight_mode=2)
    a.fin_ps = GnBwdFin(red=P(34), gamma=P(36), meanrstd=P(33), dgamma=P(37), dbeta=P(38), alpha_slots=P(35), alpha=P(50),
                        dalpha=P(51), count=128.0, alpha_sign=1.0, groups=8)
    a.fin_bil = GnBwdFin(red=P(44), gamma=P(46), meanrstd=P(43), dgamma=P(47), dbeta=P(48), alpha_slots=P(45), alpha=P(50),
                         dalpha=P(51), count=128.0, alpha_sign=-1.0, groups=8)
    return a


def _cons(a):
    return (Consumer * 2)(a.cons0, a.cons1) if a.consumers else None


def _ref(s):
    return None if s is None else C.byref(s)


CALLS = {
    "act_bwd_reduce": lambda L, a: L.mrisr_act_bwd_reduce(a.dtype, a.x, a.scale, a.shift, a.meanrstd, a.ncons, _cons(a), a.blend_alpha, a.g,
                                                          a.red, a.alpha_slots, a.N, a.H, a.W, a.C, a.groups, None),
    "act_bwd_apply_fused": lambda L, a: L.mrisr_act_bwd_apply_fused(a.dtype, a.x, a.scale, a.shift, a.ncons, _cons(a), a.blend_alpha, a.coef,
                                                                    _ref(a.fin), a.dx, a.N, a.H, a.W, a.C, None),
    "act_bwd_onepass": lambda L, a: L.mrisr_act_bwd_onepass(a.dtype, a.x, a.scale, a.shift, a.meanrstd, a.ncons, _cons(a), a.red, a.arrive,
                                                            _ref(a.fin), a.dx, a.N, a.H, a.W, a.C, None),
    "act_bwd_apply_fused_unshuffle": lambda L, a: L.mrisr_act_bwd_apply_fused_unshuffle(a.dtype, a.x, a.scale, a.shift, _cons(a), a.blend_alpha,
                                                                                        _ref(a.fin), a.dx, a.dbias, a.N, a.H, a.W, a.C, None),
    "act_bwd_blend_reduce": lambda L, a: L.mrisr_act_bwd_blend_reduce(a.dtype, a.da, _ref(a.ps), _ref(a.bil), a.blend_alpha, a.N, a.H, a.W,
                                                                      a.C, a.groups, None),
    "act_bwd_blend_apply": lambda L, a: L.mrisr_act_bwd_blend_apply(a.dtype, a.da, _ref(a.ps), _ref(a.bil), a.blend_alpha, _ref(a.fin_ps),
                                                                    _ref(a.fin_bil), a.dx, a.dx2, a.dbias, a.N, a.H, a.W, a.C, None),
    "act_bwd_finalize": lambda L, a: L.mrisr_act_bwd_finalize(a.red, a.gamma, a.meanrstd, a.dgamma, a.dbeta, a.coef_out, a.N, a.C, a.groups,
                                                              a.count, a.alpha_slots, a.alpha, a.dalpha, 1.0, None),
    "act_bwd_apply": lambda L, a: L.mrisr_act_bwd_apply(a.dtype, a.x, a.g, a.coef, a.dx, a.N, a.H, a.W, a.C, a.out_mode, a.dbias, None),
}
# what the base call lacks to be valid for an entry (the blend entries need the blend weight, apply its coefficients)
ENTRY_BASE = {"act_bwd_blend_reduce": {"blend_alpha": P(60)}, "act_bwd_blend_apply": {"blend_alpha": P(60)}, "act_bwd_apply": {"coef": P(61)}}

POOL = {"cons0.spatial": SP_POOL2, "cons0.H": 4, "cons0.W": 4}          # a 2x2-pool consumer that fits
UP2 = {"cons0.spatial": SP_UP2, "cons0.H": 16, "cons0.W": 16}           # a bilinear x2 consumer that fits
HEAD = {"cons0.spatial": SP_HEAD, "cons0.head_out": P(70), "cons0.head_w": P(71), "cons0.head_part": P(72), "cons0.head_dw": P(73),
        "cons0.head_db": P(74)}
ALPHA = {"blend_alpha": P(60)}


def _rows(entry, rows):
    return [pytest.param(entry, defect, rc, word, id=f"{entry}-{name}") for name, defect, rc, word in rows]


def _nulls(names, rc=E_ARG):
    return [(f"null-{n}", {n: None}, rc, "") for n in names]


CASES = []
CASES += _rows("act_bwd_reduce", _nulls(["x", "scale", "shift", "meanrstd", "red"]) + [
    ("null-consumers", {"consumers": False}, E_ARG, ""),
    ("null-consumer-da", {"cons0.da": None}, E_ARG, ""),
    ("consumers-0", {"ncons": 0}, E_ARG, ""),
    ("consumers-3", {"ncons": 3}, E_ARG, ""),
    ("C-not-vector", {"C": 12, "groups": 4}, E_SHAPE, ""),
    ("groups-0", {"groups": 0}, E_SHAPE, ""),
    ("groups-33", {"groups": 33}, E_SHAPE, ""),
    ("alpha_slots-without-alpha", {"alpha_slots": P(62)}, E_ARG, "alpha_slots"),
    ("alpha_slots-pooled-consumer", {"alpha_slots": P(62), **ALPHA, **POOL}, E_ARG, "alpha_slots"),
    ("weight_mode-3", {"cons0.weight_mode": 3, **ALPHA}, E_ARG, "weight_mode"),
    ("weight_mode-without-alpha", {"cons0.weight_mode": 1}, E_ARG, "weight_mode"),
    ("window-past-C_total", {"cons0.c_off": 8}, E_SHAPE, "channels"),
    ("pool2-extent", {**POOL, "cons0.H": 3}, E_SHAPE, "POOL2"),
    ("up2-extent", {**UP2, "cons0.H": 15}, E_SHAPE, "UP2"),
    ("head-with-second-consumer", {**HEAD, "ncons": 2}, E_ARG, "head consumer"),
    ("head-null-pointer", {**HEAD, "cons0.head_w": None, "g": None}, E_ARG, "head consumer"),
    ("head-with-g", {**HEAD}, E_ARG, "g = NULL"),
    ("no-g-with-up2-consumer", {**UP2, "g": None}, E_ARG, "g = NULL"),
    ("dtype-7", {"dtype": 7}, E_DTYPE, "dtype"),
    ("dtype-7-window", {"dtype": 7, "g": None, **POOL}, E_DTYPE, "dtype"),
])
FIN_ROWS = [
    ("fin-null-red", {"fin.red": None}, E_ARG, "fin"),
    ("fin-null-dbeta", {"fin.dbeta": None}, E_ARG, "fin"),
    ("fin-groups-0", {"fin.groups": 0}, E_SHAPE, "groups"),
    ("fin-groups-33", {"fin.groups": 33}, E_SHAPE, "groups"),
    ("fin-groups-not-dividing-C", {"fin.groups": 3}, E_SHAPE, "groups"),
    ("fin-count-0", {"fin.count": 0.0}, E_SHAPE, ""),
]
CASES += _rows("act_bwd_apply_fused", _nulls(["x", "scale", "shift", "dx"]) + FIN_ROWS + [
    ("null-consumers", {"consumers": False}, E_ARG, ""),
    ("null-consumer-da", {"cons0.da": None}, E_ARG, ""),
    ("coef-and-fin", {"coef": P(61)}, E_ARG, "coef / fin"),
    ("neither-coef-nor-fin", {"fin": None}, E_ARG, "coef / fin"),
    ("alpha_slots-without-alpha", {"fin.alpha_slots": P(62)}, E_ARG, "alpha_slots"),
    ("alpha_slots-without-dalpha", {"fin.alpha_slots": P(62), "fin.alpha": P(63)}, E_ARG, "alpha_slots"),
    ("consumers-0", {"ncons": 0}, E_ARG, ""),
    ("consumers-3", {"ncons": 3}, E_ARG, ""),
    ("C-not-vector", {"C": 12, "fin.groups": 4}, E_SHAPE, ""),
    ("head-with-second-consumer", {**HEAD, "ncons": 2}, E_ARG, "head consumer"),
    ("head-null-dw", {**HEAD, "cons0.head_dw": None}, E_ARG, "head consumer"),
    ("head-with-coef", {**HEAD, "coef": P(61), "fin": None}, E_ARG, "needs fin"),
    ("weight_mode-3", {"cons0.weight_mode": 3, **ALPHA}, E_ARG, "weight_mode"),
    ("window-past-C_total", {"cons0.c_off": 8}, E_SHAPE, "channels"),
    ("pool2-extent", {**POOL, "cons0.H": 3}, E_SHAPE, "POOL2"),
    ("up2-consumer", {**UP2}, E_UNSUPPORTED, ""),
    ("pool2-odd-node", {**POOL, "H": 7, "cons0.H": 3}, E_UNSUPPORTED, ""),
    ("dtype-7", {"dtype": 7}, E_DTYPE, "dtype"),
    ("dtype-7-window", {"dtype": 7, **POOL}, E_DTYPE, "dtype"),
])
CASES += _rows("act_bwd_onepass", _nulls(["x", "scale", "shift", "meanrstd", "red", "arrive", "fin", "dx"]) + FIN_ROWS[1:] + [
    ("null-consumers", {"consumers": False}, E_ARG, ""),
    ("fin-red-is-not-red", {"fin.red": P(64)}, E_ARG, "fin"),
    ("fin-alpha_slots", {"fin.alpha_slots": P(62), "fin.alpha": P(63), "fin.dalpha": P(65)}, E_UNSUPPORTED, "blend"),
    ("alpha_slots-without-alpha", {"fin.alpha_slots": P(62)}, E_UNSUPPORTED, "blend"),
    ("alpha_slots-and-groups-0", {"fin.alpha_slots": P(62), "fin.groups": 0}, E_SHAPE, "groups"),      # the fin's own defects come first
    ("consumers-0", {"ncons": 0}, E_UNSUPPORTED, ""),
    ("consumers-3", {"ncons": 3}, E_UNSUPPORTED, ""),
    ("C-not-vector", {"C": 12, "fin.groups": 4}, E_UNSUPPORTED, ""),
    ("C-not-power-of-two", {"C": 24}, E_UNSUPPORTED, ""),
    ("weight_mode-3", {"cons0.weight_mode": 3}, E_UNSUPPORTED, ""),
    ("window-past-C_total", {"cons0.c_off": 8}, E_SHAPE, "channels"),
    ("null-consumer-da", {"cons0.da": None}, E_ARG, ""),
    ("pool2-extent", {**POOL, "cons0.H": 3}, E_UNSUPPORTED, ""),
    ("up2-consumer", {**UP2}, E_UNSUPPORTED, ""),
    ("head-with-second-consumer", {**HEAD, "ncons": 2}, E_UNSUPPORTED, ""),
    ("float32", {"dtype": F32}, E_UNSUPPORTED, ""),
    ("dtype-7", {"dtype": 7}, E_UNSUPPORTED, ""),
])
CASES += _rows("act_bwd_apply_fused_unshuffle", _nulls(["x", "scale", "shift", "dx", "fin"]) + FIN_ROWS + [
    ("null-consumer", {"consumers": False}, E_ARG, ""),
    ("null-consumer-da", {"cons0.da": None}, E_ARG, ""),
    ("alpha_slots-without-alpha", {"fin.alpha_slots": P(62)}, E_ARG, "alpha_slots"),
    ("C-not-vector", {"C": 12, "fin.groups": 4}, E_SHAPE, "even dims"),
    ("odd-H", {"H": 7, "cons0.H": 7}, E_SHAPE, "even dims"),
    ("pool2-consumer", {**POOL}, E_UNSUPPORTED, ""),
    ("consumer-of-another-size", {"cons0.H": 16}, E_UNSUPPORTED, ""),
    ("weight_mode-3", {"cons0.weight_mode": 3, **ALPHA}, E_ARG, "weight_mode"),
    ("window-past-C_total", {"cons0.c_off": 8}, E_SHAPE, "channels"),
    ("dtype-7", {"dtype": 7}, E_DTYPE, "dtype"),
])
BLEND_ROWS = _nulls(["da", "ps", "bil", "blend_alpha"]) + [
    ("null-branch-x", {"ps.x": None}, E_ARG, "branch 0"),
    ("null-branch-alpha_slots", {"bil.alpha_slots": None}, E_ARG, "branch 1"),
    ("weight_mode-3", {"bil.weight_mode": 3}, E_ARG, "weight_mode"),
    ("weight_mode-0", {"ps.weight_mode": 0}, E_ARG, "weight_mode"),
    ("C-not-vector", {"C": 12}, E_UNSUPPORTED, ""),
    ("odd-H", {"H": 7}, E_UNSUPPORTED, ""),
    ("N-0", {"N": 0}, E_UNSUPPORTED, ""),
    ("float32", {"dtype": F32}, E_UNSUPPORTED, ""),
    ("dtype-7", {"dtype": 7}, E_UNSUPPORTED, ""),
]
CASES += _rows("act_bwd_blend_reduce", BLEND_ROWS + [
    ("groups-0", {"groups": 0}, E_SHAPE, "groups"),
    ("groups-33", {"groups": 33}, E_SHAPE, "groups"),
    ("groups-not-dividing-C", {"groups": 3}, E_SHAPE, "groups"),
])
CASES += _rows("act_bwd_blend_apply", BLEND_ROWS + _nulls(["fin_ps", "fin_bil", "dx", "dx2"]) + [
    ("fin-groups-differ", {"fin_bil.groups": 4}, E_SHAPE, "groups"),
    ("groups-0", {"fin_ps.groups": 0, "fin_bil.groups": 0}, E_SHAPE, "groups"),
    ("groups-33", {"fin_ps.groups": 33, "fin_bil.groups": 33}, E_SHAPE, "groups"),
    ("fin-red-of-another-tensor", {"fin_bil.red": P(64)}, E_ARG, "fin 1"),
    ("fin-null-gamma", {"fin_ps.gamma": None}, E_ARG, "fin 0"),
    ("fin-count-0", {"fin_ps.count": 0.0}, E_SHAPE, "fin 0 count"),
    ("fin-alpha_slots-of-another-tensor", {"fin_ps.alpha_slots": P(64)}, E_ARG, "fin 0"),
    ("alpha_slots-without-alpha", {"fin_bil.alpha": None}, E_ARG, "fin 1"),
])
CASES += _rows("act_bwd_finalize", _nulls(["red", "gamma", "meanrstd", "dgamma", "dbeta", "coef_out"]) + [
    ("groups-0", {"groups": 0}, E_SHAPE, "groups"),
    ("groups-33", {"groups": 33}, E_SHAPE, "groups"),
    ("alpha_slots-without-alpha", {"alpha_slots": P(62)}, E_ARG, "alpha_slots"),
    ("alpha_slots-without-dalpha", {"alpha_slots": P(62), "alpha": P(63)}, E_ARG, "alpha_slots"),
])
CASES += _rows("act_bwd_apply", _nulls(["x", "g", "coef", "dx"]) + [
    ("C-not-vector", {"C": 12}, E_SHAPE, ""),
    ("odd-H-with-pixel-shuffle", {"H": 7, "out_mode": OUT_PIXEL_SHUFFLE2}, E_SHAPE, "odd dims"),
    ("dbias-without-pixel-shuffle", {"dbias": P(66)}, E_UNSUPPORTED, "dbias"),
    ("dtype-7", {"dtype": 7}, E_DTYPE, "dtype"),
    ("dtype-7-pixel-shuffle", {"dtype": 7, "out_mode": OUT_PIXEL_SHUFFLE2, "dbias": P(66)}, E_DTYPE, "dtype"),
])


def _apply(a, defect):
    for path, v in defect.items():
        *head, leaf = path.split(".")
        obj = a
        for h in head:
            obj = getattr(obj, h)
        assert hasattr(obj, leaf), path
        setattr(obj, leaf, v)


@pytest.mark.parametrize("entry,defect,rc,word", CASES)
def test_one_defect_is_refused_before_any_launch(entry, defect, rc, word):
    assert rc in (E_ARG, E_SHAPE, E_DTYPE, E_UNSUPPORTED) and defect       # never the valid call, never one that reaches a launch
    lib = _lib.load()
    a = _base()
    _apply(a, ENTRY_BASE.get(entry, {}))
    _apply(a, defect)
    got = CALLS[entry](lib, a)
    msg = lib.mrisr_last_error().decode()
    assert got == rc, (got, msg)
    assert msg.startswith(entry + ":") and word in msg, msg


def _consumers(*specs):
    arr = (Consumer * 2)()
    for k, s in enumerate(specs):
        arr[k] = Consumer(**{"da": P(20 + k), "C_total": 16, "c_off": 0, "H": 8, "W": 8, "spatial": SP_NONE, **s})
    return arr


PLAIN, POOLED = {}, {"spatial": SP_POOL2, "H": 4, "W": 4}


@pytest.mark.parametrize("dtype,cons,N,H,W,C,want", [
    (BF16, [PLAIN], 2, 8, 8, 16, 1),
    (BF16, [PLAIN, PLAIN], 2, 8, 8, 16, 1),
    (_lib.F16, [POOLED], 2, 8, 8, 16, 2),
    (BF16, [PLAIN, POOLED], 2, 8, 8, 16, 2),
    (F32, [PLAIN], 2, 8, 8, 16, 0),
    (7, [PLAIN], 2, 8, 8, 16, 0),
    (BF16, [PLAIN], 0, 8, 8, 16, 0),
    (BF16, [PLAIN], 2, 8, 8, 24, 0),                              # C / 8 is no power of two
    (BF16, [PLAIN], 2, 8, 8, 12, 0),
    (BF16, [{"weight_mode": 1}], 2, 8, 8, 16, 0),
    (BF16, [{"off_x": 1}], 2, 8, 8, 16, 0),
    (BF16, [{"spatial": SP_UP2, "H": 16, "W": 16}], 2, 8, 8, 16, 0),
    (BF16, [{"spatial": SP_POOL2, "H": 3, "W": 4}], 2, 8, 8, 16, 0),
    (BF16, [POOLED], 2, 7, 8, 16, 0),
    (BF16, [POOLED, POOLED], 2, 8, 8, 16, 0),
    (BF16, [{"H": 512, "W": 512}], 1, 512, 512, 16, 1),           # 256 blocks per image: the most the barrier takes
    (BF16, [{"H": 514, "W": 512}], 1, 514, 512, 16, 0),           # 257
    (BF16, [{"H": 512, "W": 512}, {"spatial": SP_POOL2, "H": 256, "W": 256}], 1, 512, 512, 16, 2),      # 256 blocks of windows
    (BF16, [{"H": 514, "W": 512}, {"spatial": SP_POOL2, "H": 257, "W": 256}], 1, 514, 512, 16, 0),
])
def test_onepass_ok(dtype, cons, N, H, W, C, want):
    lib = _lib.load()
    assert lib.mrisr_act_bwd_onepass_ok(dtype, len(cons), _consumers(*cons), N, H, W, C) == want
    assert lib.mrisr_act_bwd_onepass_ok(dtype, 0, _consumers(*cons), N, H, W, C) == 0
    assert lib.mrisr_act_bwd_onepass_ok(dtype, 3, _consumers(*cons), N, H, W, C) == 0
    assert lib.mrisr_act_bwd_onepass_ok(dtype, len(cons), None, N, H, W, C) == 0


@pytest.mark.parametrize("dtype,N,H,W,C,want", [
    (BF16, 2, 8, 8, 16, 1), (_lib.F16, 1, 2, 2, 8, 1), (BF16, 65535, 8, 8, 2048, 1),
    (F32, 2, 8, 8, 16, 0), (7, 2, 8, 8, 16, 0), (BF16, 0, 8, 8, 16, 0), (BF16, 65536, 8, 8, 16, 0),
    (BF16, 2, 7, 8, 16, 0), (BF16, 2, 8, 0, 16, 0), (BF16, 2, 8, 8, 12, 0), (BF16, 2, 8, 8, 0, 0), (BF16, 2, 8, 8, 2056, 0),
])
def test_blend_ok(dtype, N, H, W, C, want):
    assert _lib.load().mrisr_act_bwd_blend_ok(dtype, N, H, W, C) == want
