"""Per-plane parity, outlier probes and launch-form coverage for the InstanceNorm / MAT kernels (csrc/norm.hip).  DESIGN.md 6b.20.

REFERENCE: float64 closed forms of the stored (already rounded) operands, per plane (n, c), eps = ops.IN_EPS:
    m, biased var, r = 1 / sqrt(var + eps), xh = (x - m) r, gg = 1 + g_img + g_st, bb = b_img + b_st, v = xh gg + bb, y = act(v)
    dv = da act', dxh = dv gg, dx = r (dxh - mean_p dxh - xh mean_p(dxh xh)) [+ res]
    dgamma_img = dv xh, dbeta_img = dv, dgamma_st = sum_p dv xh, dbeta_st = sum_p dv
test_closed_forms_match_autograd proves them against float64 autograd through F.instance_norm (1e-12, planes of >= 2 pixels;
F.instance_norm refuses HW = 1, the closed forms do not).

BRANCHES (branch-controlled comparison): one relu / lrelu branch taken differently from float64 moves the plane
sums and with them every dx of the plane by ~1/HW, so the reference backward takes mask = (y_kernel > 0) from the HIP forward of the
same call sequence; the test asserts mask == (v > 0) wherever |v| > delta_y and prints how many elements lie inside that band.

BOUNDS, every element, `<=`; c32 = 1e-5 is TOL[torch.float32] of test_kernels_gpu, applied per plane instead of per tensor:
    y          A = max_p(|xh gg| + |bb|)                                         delta = c32 A + a_act
    dx         B = r max_p(|dxh| + mean_p|dxh| + |xh| mean_p|dxh xh|)            delta = 2 c32 B   (+ 2^-24 |ref| with res)
    dgamma_img                                                                    delta = c32 max_p|dv xh|
    dbeta_img                                                                     delta = 2^-23 |ref|
    dgamma_st                                                                     delta = (2 (HW + 1) 2^-24 + c32) sum_p|dv xh|
    dbeta_st                                                                      delta = 2 (HW + 1) 2^-24 sum_p|dv|
    fp32 tensors: tol = delta;   bf16 tensors: tol = delta + hu(|ref| + delta),   hu(v) = 2^(floor(log2 v) - 8)
a_act = 0 for none / relu / lrelu, 2^-20 for tanh (test_thin_conv_layers_gpu derives both it and hu); swish: c32 A times its Lipschitz
constant 1.1, and a_act = 4 x the largest deviation, over the case's v, of torch's fp32 v * sigmoid(v) on the CPU from float64 (margin 4
as for Adam in DESIGN.md section 4).  2 (HW + 1) 2^-24 is the any-order fp32 summation bound.  The bounds are stated against the sum of
the absolute terms, never against the result: on a 2-pixel plane dx is analytically ~0.  Planes of fewer than 16 pixels carry no
offset, their sample mean included (x - m cancels: with an 8 sigma offset at HW = 2 plain two-pass fp32 arithmetic is outside the forward
bound, and so are two draws that happen to lie close together: 1.28 x on one plane of 204).  The slope is the fp32 number the kernels get.

ADMISSION (test_reference_admits_fp32, CPU): the same formulas in fp32 with torch stay within 0.5 delta at every element of every
case of at most 2M elements; rounded once to bf16 (the bf16 cases) they lie inside tol at every element.  (After the store the ratio
cannot stay under 0.5: a correctly rounded bf16 store alone errs by up to hu, which is the whole store term.)

DATA.  scaled: plane (n, c) has std 2^((c + n) mod 13 - 6) and, where HW >= 16, mean std ((c + 3 n) mod 17 - 8); da randn; gamma /
beta maps and the state affine 0.5 randn; everything rounded to the dtype first.  probe: scaled without offsets, plane q = n C + c
carries one 64 std at pixel POS[q mod len(POS)] of x and one 64 at that pixel + HW // 2 (mod HW) of da; POS is every pixel when the
case has at least HW planes (N is raised to ceil(HW / C) where that keeps the case under 4M elements), otherwise the first and the
last chunk row, every register-slot boundary +- 1 and every split boundary +- 1 of the kernels the case runs.  A pixel dropped from,
or counted twice in, the statistics changes the plane's rstd by a factor (HW 441: variance 1 vs 10.3); one dropped from a backward sum
changes every dx of the plane by ~0.15.

WHICH KERNEL RAN is unpinned but for the header of the statistics buffer ({1, HW, 0, 0} after a fused launch, {S, rows, 0, 0} after the
pair): test_case_geometry restates stats_splits, small_plane, the large-plane slab choice and the apply split in Python and asserts each
named case's figures; test_form_rule_matches_library compares the restated form rule with the library's own (s2p_in_norm_form).
Every call is made twice: outputs and the statistics buffer must be bit-identical.  Every output sits in a sentinel-filled allocation
with 8 KiB bands (fp32 side buffers: guard_region.Region); pad columns and bands must keep the sentinel; input pads hold NaN.

Worst |err| / tol on an MI355X per launch form: DESIGN.md section 6b.20 (printed by test_zz_report)."""
import functools
import math
import types
import zlib
from typing import NamedTuple

import pytest
import torch
import torch.nn.functional as F

from guard_region import Region
from s2p_amd import _lib, ops
from s2p_amd._lib import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_SWISH, ACT_TANH, chunk_elems, dtype_id
from test_kernels_gpu import TOL

BF, F32 = torch.bfloat16, torch.float32
C32 = TOL[torch.float32]
U24 = 2.0 ** -24
A_TANH = 2.0 ** -20
SLOPE = float(torch.tensor(0.2, dtype=torch.float32))       # the slope as the kernels receive it: a float argument
EPS = ops.IN_EPS
ACT_NAME = {ACT_NONE: "none", ACT_RELU: "relu", ACT_LRELU: "lrelu", ACT_TANH: "tanh", ACT_SWISH: "swish"}
SIMPLE = (ACT_NONE, ACT_RELU, ACT_LRELU)
WORST, INBAND, SWISH_A = {}, {}, {}


def cdiv(a, b):
    return -(-a // b)


# ---- the launch rules of norm.hip, restated -----------------------------------------------------------------------------------------
def stats_splits(N, HW, C):
    """(S, rows per split) of in_stats / in_bwd_reduce: >= 1024 workgroups, >= 128 pixels per split."""
    ps = max(1, min(cdiv(1024, cdiv(C, 64) * N), cdiv(HW, 128)))
    rows = cdiv(HW, ps)
    return cdiv(HW, rows), rows


def apply_splits(N, HW, C):
    """(splits, rows per split) of the apply kernels: >= 64 pixels per split."""
    ps = max(1, min(cdiv(1024, cdiv(C, 64) * N), cdiv(HW, 64)))
    rows = cdiv(HW, ps)
    return cdiv(HW, rows), rows


def small_plane(dtype, HW, gb):
    lim = 128 if dtype == F32 else 256
    return 0 if gb else (256 if HW <= lim else (512 if HW <= 2 * lim else 0))


def fwd_form(dtype, N, HW, C, gb, act):
    maxhw = 256 if dtype == F32 else 512
    if dtype == BF and HW > maxhw and act in SIMPLE and not gb:
        cs = 64 if (HW <= 28 * 64 and C % 64 == 0) else (16 if (HW <= 28 * 256 and C % 16 == 0) else 0)
        if cs == 64 and HW <= 14 * 128 and C % 32 == 0 and N * (C // 64) < 256:
            cs = 32
        if cs and N * (C // cs) >= 64:
            return {64: "L64x28", 32: "L32x14", 16: "L16x28"}[cs]
    if HW > maxhw or act not in SIMPLE:
        return "pair"
    return "f%d" % (small_plane(dtype, HW, gb) or 1024)


def bwd_form(dtype, HW, gb, act):
    if HW > (256 if dtype == F32 else 512) or act not in SIMPLE:
        return "pair"
    return "f%d" % (small_plane(dtype, HW, gb) or 1024)           # (dgb_img is requested exactly where gb_img is given)


FORM_NAME = {_lib.NORM_FORM_PAIR: "pair", _lib.NORM_FORM_F256: "f256", _lib.NORM_FORM_F512: "f512", _lib.NORM_FORM_F1024: "f1024",
             _lib.NORM_FORM_L64X28: "L64x28", _lib.NORM_FORM_L32X14: "L32x14", _lib.NORM_FORM_L16X28: "L16x28"}


def lib_form(dtype, N, HW, C, gb, act, backward):
    """The library's own answer (s2p_in_norm_form: no launch, no device).  dgb_img is requested exactly where gb_img is given."""
    return FORM_NAME[_lib.lib().s2p_in_norm_form(dtype_id(dtype), N, HW, C, int(gb), int(gb), act, int(backward))]


def chunk_rows(dtype, form):
    """Pixel rows a workgroup of `form` has in flight (PR) and its register slots per thread (0: a strided loop)."""
    ce = chunk_elems(dtype)
    if form == "pair":
        return 256 // (64 // ce), 0
    if form[0] == "L":
        cs, mp = {"L64x28": (64, 28), "L32x14": (32, 14), "L16x28": (16, 28)}[form]
        return 512 // (cs // ce), mp
    th = int(form[1:])
    pr = th // (64 // ce)
    return pr, ((512 if dtype == BF else 256) // pr if th == 1024 else 8)


# ---- cases -------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    dtype: torch.dtype
    N: int
    HW: int
    C: int
    data: str
    act: int
    gb: bool = False
    st: bool = False
    bwd: bool = True
    res: bool = False
    how: str = "norm"        # norm: s2p_in_norm_fwd + s2p_in_norm_bwd_res;  pair: in_stats + in_apply_fwd, in_bwd_reduce + in_bwd_apply
    pitched: bool = False


CASES = {}


def _add(sec, dtype, N, HW, C, data, act, **kw):
    if data == "probe" and N * C < HW and cdiv(HW, C) * HW * C <= 4 << 20:
        N = cdiv(HW, C)                                   # every pixel position probed in at least one plane
    cs = Case(dtype, N, HW, C, data, act, **kw)
    cid = "%s-%s-n%d-hw%d-c%d-%s-%s%s%s%s%s" % (sec, "bf16" if dtype == BF else "fp32", N, HW, C, data, ACT_NAME[act], "-gb" if cs.gb else "",
                                               "-st" if cs.st else "", "-res" if cs.res else "", "-pitched" if cs.pitched else "")
    assert cid not in CASES
    CASES[cid] = cs
    return cid


for _dt, _hws, _cs in ((BF, (1, 2, 31, 32, 33, 255, 256, 257, 511, 512), (8, 72)), (F32, (1, 2, 15, 16, 17, 127, 128, 129, 255, 256), (4, 68))):
    for _hw in _hws:                                      # a. fused small-plane forms (256 / 512 threads), plain
        for _c in _cs:
            for _data in ("scaled", "probe"):
                for _act in (ACT_NONE, ACT_LRELU):
                    _add("a", _dt, 3, _hw, _c, _data, _act)
    _add("a", _dt, 3, _hws[7], _cs[1], "scaled", ACT_LRELU, st=True)        # gb_st only: stays on the small form (512 threads), writes dgb_st
    _add("a", _dt, 3, _hws[4], _cs[1], "probe", ACT_LRELU, st=True)         # the same on the 256-thread form
for _dt, _hws, _cs in ((BF, (127, 128, 129, 512), (64, 72)), (F32, (63, 64, 65, 256), (64, 68))):
    for _hw in _hws:                                      # b. 1024-thread modulated form
        for _c in _cs:
            for _act in (ACT_RELU, ACT_LRELU):
                _add("b", _dt, 3, _hw, _c, "scaled", _act, gb=True)
                _add("b", _dt, 3, _hw, _c, "scaled", _act, gb=True, st=True)
        _add("b", _dt, 3, _hw, _cs[1], "probe", ACT_LRELU, gb=True, st=True)
    _add("b", _dt, 3, _hws[3], 64, "scaled", ACT_LRELU, gb=True, st=True, res=True)
    _add("b", _dt, 3, _hws[2], _cs[1], "scaled", ACT_LRELU, gb=True, st=True, pitched=True)     # f. pitches
    _add("a", _dt, 3, _hws[2] // 4 + 1, _cs[1], "scaled", ACT_LRELU, st=True, pitched=True)
for _data in ("scaled", "probe"):                         # c. the pair path
    _add("c", BF, 2, 513, 72, _data, ACT_LRELU, gb=True, how="pair")
    _add("c", BF, 2, 1025, 72, _data, ACT_LRELU, gb=True, how="pair")
    _add("c", F32, 2, 257, 68, _data, ACT_LRELU, how="pair")
for _dt, _c in ((BF, 72), (F32, 68)):
    _add("c", _dt, 2, 49, _c, "scaled", ACT_TANH, how="pair")
    _add("c", _dt, 2, 600, _c, "scaled", ACT_TANH, how="pair")
    _add("c", _dt, 2, 600, _c, "probe", ACT_TANH, st=True, how="pair")
    _add("c", _dt, 2, 49, _c, "scaled", ACT_SWISH, bwd=False, how="pair")
_add("c", BF, 2, 513, 72, "scaled", ACT_LRELU, gb=True, st=True, how="pair", pitched=True)      # f. pitches on the pair
_add("c", F32, 2, 257, 68, "scaled", ACT_LRELU, gb=True, st=True, how="pair", pitched=True)
for _data in ("scaled", "probe"):                         # d. large-plane forwards (bf16, plain, lrelu)
    _add("d", BF, 2, 513, 1024, _data, ACT_LRELU, bwd=False)
    _add("d", BF, 2, 1792, 1024, _data, ACT_LRELU, bwd=False)
    _add("d", BF, 4, 513, 4096, _data, ACT_LRELU, bwd=False)
    _add("d", BF, 8, 1793, 128, _data, ACT_LRELU, bwd=False)
    _add("d", BF, 8, 7056, 128, _data, ACT_LRELU, bwd=False)
    _add("d", BF, 8, 7168, 128, _data, ACT_LRELU, bwd=False)
    _add("d", BF, 13, 600, 80, _data, ACT_LRELU, bwd=False)
    _add("d", BF, 8, 7169, 128, _data, ACT_LRELU, bwd=False)
    _add("d", BF, 2, 600, 64, _data, ACT_LRELU, bwd=False)
    _add("d", BF, 2, 1793, 64, _data, ACT_LRELU)
_add("d", BF, 4, 1792, 4096, "scaled", ACT_LRELU, bwd=False)                 # the one large case: the full_rows copy of the 64-channel form
_add("d", BF, 13, 600, 80, "scaled", ACT_LRELU, bwd=False, pitched=True)
IDS = list(CASES)
CPU_IDS = [c for c in IDS if CASES[c].N * CASES[c].HW * CASES[c].C <= 2 << 20]

# launch-rule figures of the named cases: (forward form, backward form, S of the pair's statistics, rows per split, rows of the last split)
GEOM = {
    "c-bf16-n2-hw513-c72-scaled-lrelu-gb": ("pair", "pair", 5, 103, 101),
    "c-bf16-n8-hw513-c72-probe-lrelu-gb": ("pair", "pair", 5, 103, 101),
    "c-bf16-n2-hw1025-c72-scaled-lrelu-gb": ("pair", "pair", 9, 114, 113),
    "c-bf16-n15-hw1025-c72-probe-lrelu-gb": ("pair", "pair", 9, 114, 113),
    "c-fp32-n2-hw257-c68-scaled-lrelu": ("pair", "pair", 3, 86, 85),
    "c-fp32-n4-hw257-c68-probe-lrelu": ("pair", "pair", 3, 86, 85),
    "c-bf16-n2-hw49-c72-scaled-tanh": ("pair", "pair", 1, 49, 49),
    "c-bf16-n2-hw600-c72-scaled-tanh": ("pair", "pair", 5, 120, 120),
    "c-fp32-n2-hw49-c68-scaled-swish": ("pair", None, 1, 49, 49),
    "d-bf16-n2-hw513-c1024-scaled-lrelu": ("L32x14", None, 5, 103, 101),
    "d-bf16-n2-hw1792-c1024-scaled-lrelu": ("L32x14", None, 14, 128, 128),
    "d-bf16-n4-hw513-c4096-scaled-lrelu": ("L64x28", None, 4, 129, 126),
    "d-bf16-n4-hw1792-c4096-scaled-lrelu": ("L64x28", None, 4, 448, 448),
    "d-bf16-n8-hw1793-c128-scaled-lrelu": ("L16x28", None, 15, 120, 113),
    "d-bf16-n15-hw1793-c128-probe-lrelu": ("L16x28", None, 15, 120, 113),
    "d-bf16-n8-hw7056-c128-scaled-lrelu": ("L16x28", None, 56, 126, 126),
    "d-bf16-n8-hw7168-c128-scaled-lrelu": ("L16x28", None, 56, 128, 128),
    "d-bf16-n13-hw600-c80-scaled-lrelu": ("L16x28", None, 5, 120, 120),
    "d-bf16-n8-hw7169-c128-scaled-lrelu": ("pair", None, 57, 126, 113),
    "d-bf16-n2-hw600-c64-scaled-lrelu": ("pair", None, 5, 120, 120),
    "d-bf16-n10-hw600-c64-probe-lrelu": ("pair", None, 5, 120, 120),
    "d-bf16-n2-hw1793-c64-scaled-lrelu": ("pair", "pair", 15, 120, 113),
    "d-bf16-n29-hw1793-c64-probe-lrelu": ("L16x28", "pair", 15, 120, 113),
}


def _forms(cs):
    return fwd_form(cs.dtype, cs.N, cs.HW, cs.C, cs.gb, cs.act), (bwd_form(cs.dtype, cs.HW, cs.gb, cs.act) if cs.bwd else None)


def _probe_positions(cs):
    """The pixel positions the planes of a probe case cycle through (module docstring)."""
    if cs.N * cs.C >= cs.HW:
        return list(range(cs.HW))
    pos = []
    forms = [f for f in _forms(cs) if f]
    prs = [chunk_rows(cs.dtype, f) for f in forms]
    top = max(pr for pr, _ in prs)
    pos += list(range(top)) + list(range(cs.HW - top, cs.HW))
    for pr, slots in prs:
        for k in range(1, slots):
            pos += [k * pr - 1, k * pr, k * pr + 1]
    if "pair" in forms:
        for rows in (stats_splits(cs.N, cs.HW, cs.C)[1], apply_splits(cs.N, cs.HW, cs.C)[1]):
            for b in range(1, cdiv(cs.HW, rows)):
                pos += [b * rows - 1, b * rows, b * rows + 1]
    return list(dict.fromkeys(p for p in pos if 0 <= p < cs.HW))


def test_case_geometry():
    """Host only: every case's launch form from the restated rules, the literal figures of the named cases, probe coverage."""
    for cid, want in GEOM.items():
        cs = CASES[cid]
        S, rows = stats_splits(cs.N, cs.HW, cs.C)
        assert _forms(cs) + (S, rows, cs.HW - (S - 1) * rows) == want, (cid, _forms(cs), S, rows)
    seen = set()
    for cid, cs in CASES.items():
        f, b = _forms(cs)
        seen.update(("fwd-" + f, "bwd-" + str(b)))
        lim = 128 if cs.dtype == F32 else 256
        if cid[0] == "a":
            want = "f256" if cs.HW <= lim else "f512"
            assert (f, b) == (want, want), cid
        elif cid[0] == "b":
            assert (f, b) == ("f1024", "f1024") and cs.HW <= 2 * lim, cid
        elif cid[0] == "c":
            assert f == "pair" and b in ("pair", None), cid
        else:
            assert cs.data == "probe" or cid.replace("-pitched", "") in GEOM, cid
        assert cs.N * cs.HW * cs.C < 10e6 or cid == "d-bf16-n4-hw1792-c4096-scaled-lrelu", cid
        if cs.data == "probe":
            pos = _probe_positions(cs)
            assert len(pos) <= cs.N * cs.C, (cid, len(pos))                 # every listed position is carried by some plane
            pr = max(chunk_rows(cs.dtype, x)[0] for x in (f, b) if x)
            assert set(range(min(pr, cs.HW))) <= set(pos) and set(range(max(0, cs.HW - pr), cs.HW)) <= set(pos), cid
    assert seen >= {"fwd-f256", "fwd-f512", "fwd-f1024", "fwd-L64x28", "fwd-L32x14", "fwd-L16x28", "fwd-pair",
                    "bwd-f256", "bwd-f512", "bwd-f1024", "bwd-pair"}
    # the full_rows copy of second_moment (28-chunk forms only): HW == slots * rows in flight exactly
    assert chunk_rows(BF, "L64x28") == (64, 28) and 64 * 28 == 1792 and chunk_rows(BF, "L16x28") == (256, 28) and 256 * 28 == 7168
    # the batch prefix of test_batch_prefix, and the fused statistics of test_stats_across_forms
    assert stats_splits(64, 257, 512) == (2, 129) and stats_splits(32, 257, 512) == (3, 86)
    assert fwd_form(BF, 3, 400, 72, False, ACT_LRELU) == "f512" and stats_splits(3, 400, 72) == (4, 100)


def test_form_rule_matches_library():
    """Host only: the restated rule (fwd_form / bwd_form) against s2p_in_norm_form, for every case of the table and over a sweep with HW
    on and either side of every threshold of the rule; what the query refuses."""
    for cid, cs in CASES.items():
        f, b = _forms(cs)
        assert lib_form(cs.dtype, cs.N, cs.HW, cs.C, cs.gb, cs.act, False) == f, cid
        if cs.bwd:
            assert lib_form(cs.dtype, cs.N, cs.HW, cs.C, cs.gb, cs.act, True) == b, cid
    n = 0
    for dtype in (BF, F32):
        for HW in [t + d for t in (128, 256, 512, 1792, 7168) for d in (-1, 0, 1)]:
            for C in (8, 16, 32, 64, 72, 128, 1024, 4096):
                for N in (1, 2, 4, 8, 64):
                    for gb in (False, True):
                        for act in ACT_NAME:
                            key = (dtype, N, HW, C, gb, ACT_NAME[act])
                            assert lib_form(dtype, N, HW, C, gb, act, False) == fwd_form(dtype, N, HW, C, gb, act), key
                            assert lib_form(dtype, N, HW, C, gb, act, True) == bwd_form(dtype, HW, gb, act), key
                            n += 1
    assert n == 2 * 15 * 8 * 5 * 2 * 5
    L = _lib.lib()
    for bad in [(7, 2, 100, 64), (_lib.BF16, 0, 100, 64), (_lib.BF16, -1, 100, 64), (_lib.BF16, 2, 0, 64), (_lib.BF16, 2, -5, 64),
                (_lib.BF16, 2, 100, 68), (_lib.F32, 2, 100, 6)]:
        for backward in (0, 1):
            assert L.s2p_in_norm_form(*bad, 0, 0, ACT_NONE, backward) == -1, bad
            assert "s2p_in_norm_form" in L.s2p_last_error().decode(), bad
    assert L.s2p_in_norm_form(_lib.F32, 2, 100, 68, 0, 0, ACT_NONE, 0) == _lib.NORM_FORM_F256


# ---- operands, closed forms, bounds --------------------------------------------------------------------------------------------------
def _inputs(cid, cs):
    g = torch.Generator().manual_seed(zlib.crc32(cid.encode()))
    N, HW, C = cs.N, cs.HW, cs.C
    n, c = torch.arange(N)[:, None], torch.arange(C)[None, :]
    std = torch.exp2(((c + n) % 13 - 6).float())                           # [N, C]
    x = torch.randn(N, HW, C, generator=g) * std[:, None, :]
    da = torch.randn(N, HW, C, generator=g)
    if cs.data == "scaled" and HW >= 16:
        x += (std * ((c + 3 * n) % 17 - 8).float())[:, None, :]
    if 2 <= HW < 16:
        x -= x.mean(1, keepdim=True)                                       # no offset, the sample's own included (conditioning: module docstring)
    if cs.data == "probe":
        pos = torch.tensor(_probe_positions(cs))
        p = pos[(n * C + c) % len(pos)]                                    # [N, C]
        x.scatter_(1, p[:, None, :], (64 * std)[:, None, :])
        da.scatter_(1, ((p + HW // 2) % HW)[:, None, :], torch.full((N, 1, C), 64.0))
    inp = types.SimpleNamespace(x=x.to(cs.dtype), da=da.to(cs.dtype), gam=None, bet=None, st=None, res=None)
    if cs.gb:
        inp.gam = (0.5 * torch.randn(N, HW, C, generator=g)).to(cs.dtype)
        inp.bet = (0.5 * torch.randn(N, HW, C, generator=g)).to(cs.dtype)
    if cs.st:
        inp.st = 0.5 * torch.randn(N, 2 * C, generator=g)
    if cs.res:
        inp.res = torch.randn(N, HW, C, generator=g).to(cs.dtype)
    return inp


def _act(v, act):
    if act == ACT_RELU:
        return torch.relu(v)
    if act == ACT_LRELU:
        return torch.where(v > 0, v, SLOPE * v)
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_SWISH:
        return v * torch.sigmoid(v)
    return v


def _forward(inp, cs, ft):
    """The closed forms of the forward in floating type `ft`."""
    C = cs.C
    x = inp.x.to(ft)
    xc = x - x.mean(1, keepdim=True)
    r = 1.0 / torch.sqrt((xc * xc).mean(1, keepdim=True) + EPS)
    xh = xc.mul_(r)
    gg, bb = torch.ones(1, 1, 1, dtype=ft), torch.zeros(1, 1, 1, dtype=ft)
    if cs.gb:
        gg, bb = gg + inp.gam.to(ft), bb + inp.bet.to(ft)
    if cs.st:
        gg, bb = gg + inp.st[:, None, :C].to(ft), bb + inp.st[:, None, C:].to(ft)
    v = xh * gg + bb
    return types.SimpleNamespace(r=r, xh=xh, gg=gg, bb=bb, v=v, y=_act(v, cs.act))


def _backward(inp, cs, f, mask, ft, bounds=False):
    """The closed forms of the backward in `ft` given the forward `f` and the relu / lrelu branch mask; with `bounds` (float64) the
    delta of every quantity as well."""
    if cs.act == ACT_RELU:
        d = mask.to(ft)
    elif cs.act == ACT_LRELU:
        d = torch.where(mask, torch.ones((), dtype=ft), torch.full((), SLOPE, dtype=ft))
    elif cs.act == ACT_TANH:
        d = 1.0 - torch.tanh(f.v) ** 2
    else:
        d = torch.ones((), dtype=ft)
    dv = inp.da.to(ft) * d
    dxh = dv * f.gg
    q = dxh * f.xh
    dx = f.r * (dxh - dxh.mean(1, keepdim=True) - f.xh * q.mean(1, keepdim=True))
    if cs.res:
        dx = dx + inp.res.to(ft)
    g = dv * f.xh
    out = dict(dx=dx)
    if cs.gb:
        out.update(dgi=g, dbi=dv.expand_as(g))
    if cs.st:
        out.update(dgs=g.sum(1), dbs=dv.expand_as(g).sum(1))
    if not bounds:
        return out
    HW = cs.HW
    B = f.r * (dxh.abs() + dxh.abs().mean(1, keepdim=True) + f.xh.abs() * q.abs().mean(1, keepdim=True)).amax(1, keepdim=True)
    delta = dict(dx=(2 * C32 * B).expand_as(dx) + (U24 * dx.abs() if cs.res else 0.0))
    if cs.gb:
        delta.update(dgi=(C32 * g.abs().amax(1, keepdim=True)).expand_as(g), dbi=2 * U24 * dv.abs().expand_as(g))
    if cs.st:
        delta.update(dgs=(2 * (HW + 1) * U24 + C32) * g.abs().sum(1), dbs=2 * (HW + 1) * U24 * dv.abs().expand_as(g).sum(1))
    return out, delta


def _delta_y(cid, cs, f):
    A = (f.xh * f.gg).abs().add_(f.bb.abs()).amax(1, keepdim=True)
    a_act = A_TANH if cs.act == ACT_TANH else 0.0
    lip = 1.0
    if cs.act == ACT_SWISH:
        v32 = f.v.float()
        SWISH_A[cid] = a_act = 4 * float(((v32 * torch.sigmoid(v32)).double() - f.y).abs().max())
        lip = 1.1
    return (C32 * lip * A + a_act).expand_as(f.y)


def _hu(v):
    """Half a unit in the last place of bf16 in the binade of v >= 0: 2^(floor(log2 v) - 8); 0 at 0."""
    return torch.exp2(torch.floor(torch.log2(v)) - 8)


def _tol(ref, delta, dtype):
    return delta if dtype == F32 else delta + _hu(ref.abs() + delta)


OUT_DTYPE = lambda cs, qty: F32 if qty in ("dgs", "dbs") else cs.dtype


@functools.lru_cache(maxsize=1)
def _case(cid):
    """Operands of a case, its float64 forward and the forward bound: computed once, shared by the tests, never modified."""
    cs = CASES[cid]
    inp = _inputs(cid, cs)
    f = _forward(inp, cs, torch.float64)
    return types.SimpleNamespace(inp=inp, f=f, dy=_delta_y(cid, cs, f))


def _check(where, form, cid, qty, got, ref, tol, limit=1.0):
    """|got - ref| <= limit * tol at EVERY element; notes and prints the worst |err| / tol."""
    err = (got.double() - ref).abs()
    bad = (~(err <= limit * tol)).nonzero()                 # (a NaN is outside every bound)
    r = err / tol.clamp_min(1e-300)
    ratio = float(r.max()) if bool(torch.isfinite(r).all()) else math.inf
    key = (where, form, "fp32" if "-fp32-" in cid else "bf16", qty)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print("%s %-7s %-46s %-3s worst |err| / tol %.3g (max |err| %.3e, max |ref| %.3e)" % (
        where, form, cid, qty, ratio, float(err.max()), float(ref.abs().max())))
    assert len(bad) == 0, "%s %s: %d of %d elements outside %g x the bound, the first at %s: got %r, ref %r, tol %.3e; worst |err| / tol %.3f" % (
        cid, qty, len(bad), err.numel(), limit, bad[0].tolist(), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])]),
        float(tol[tuple(bad[0])]), ratio)
    return ratio


def _mask_check(cid, cs, k, y_got):
    """The branch mask of the reference backward, from the produced forward; it may differ from float64 only inside the forward bound."""
    if cs.act not in (ACT_RELU, ACT_LRELU):
        return None
    mask = y_got > 0
    band = k.f.v.abs() <= k.dy
    assert bool(((mask == (k.f.v > 0)) | band).all()), "%s: an activation branch differs from float64 outside delta_y" % cid
    INBAND[cid] = int(band.sum())
    print("%s: %d of %d elements inside the branch band |v| <= delta_y" % (cid, INBAND[cid], band.numel()))
    return mask


# ---- CPU: the closed forms, and the bounds admit fp32 arithmetic -------------------------------------------------------------------------
@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH], ids=lambda a: ACT_NAME[a])
@pytest.mark.parametrize("HW", [2, 3, 49])
def test_closed_forms_match_autograd(HW, act):
    cs = Case(F32, 3, HW, 8, "scaled", act, gb=True, st=True, res=True)
    g = torch.Generator().manual_seed(5 + HW)
    t = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    inp = types.SimpleNamespace(x=t(3, HW, 8) * 2 + 0.5, da=t(3, HW, 8), gam=0.5 * t(3, HW, 8), bet=0.5 * t(3, HW, 8), st=0.5 * t(3, 16), res=t(3, HW, 8))
    f = _forward(inp, cs, torch.float64)
    got = _backward(inp, cs, f, f.v > 0, torch.float64)
    x, gam, bet, st = [a.clone().requires_grad_(True) for a in (inp.x, inp.gam, inp.bet, inp.st)]
    xn = F.instance_norm(x.permute(0, 2, 1), eps=EPS).permute(0, 2, 1)                       # [N, C, HW] planes
    y = _act(xn * (1 + gam + st[:, None, :8]) + bet + st[:, None, 8:], act)
    y.backward(inp.da)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert close(f.y, y.detach())
    assert close(got["dx"], x.grad + inp.res) and close(got["dgi"], gam.grad) and close(got["dbi"], bet.grad)
    assert close(torch.cat([got["dgs"], got["dbs"]], 1), st.grad)


@pytest.mark.parametrize("cid", CPU_IDS)
def test_reference_admits_fp32(cid):
    """The same formulas in fp32 stay within HALF of every delta; rounded once to the case's dtype they lie inside every tol."""
    cs, k = CASES[cid], _case(cid)
    f32 = _forward(k.inp, cs, torch.float32)
    todo = [("y", f32.y, k.f.y, k.dy)]
    if cs.bwd:
        mask = _mask_check(cid, cs, k, f32.y.to(cs.dtype))
        ref, delta = _backward(k.inp, cs, k.f, mask, torch.float64, bounds=True)
        g32 = _backward(k.inp, cs, f32, mask, torch.float32)
        todo += [(q, g32[q], ref[q], delta[q]) for q in ref]
    for qty, got, ref, delta in todo:
        assert _check("cpu-fp32", "all", cid, qty, got, ref, delta, limit=0.5) <= 0.5
        dt = OUT_DTYPE(cs, qty)
        if dt == BF:
            _check("cpu-bf16", "all", cid, qty, got.to(BF), ref, _tol(ref, delta, BF))


# ---- device side -----------------------------------------------------------------------------------------------------------------------
SENT = -7.5


class _Out:
    """A [rows, pitch] tensor in the middle of a sentinel-filled allocation with 8 KiB bands; the kernel owns columns [off, off + width)."""

    def __init__(self, rows, pitch, dtype, off, width):
        self.G = 8192 // (2 if dtype == BF else 4)
        self.rows, self.pitch, self.off, self.width = rows, pitch, off, width
        self.buf = torch.full((rows * pitch + 2 * self.G,), SENT, dtype=dtype, device="cuda")
        self.ptr = self.buf.data_ptr() + (self.G + off) * self.buf.element_size()
        assert self.ptr % 16 == 0

    def get(self, what):
        """The owned columns (CPU), after checking that pad columns and bands still hold the sentinel."""
        torch.cuda.synchronize()
        full = self.buf.cpu()
        body = full[self.G:self.G + self.rows * self.pitch].view(self.rows, self.pitch)
        val = body[:, self.off:self.off + self.width].clone()
        body[:, self.off:self.off + self.width] = SENT
        assert bool((full == SENT).all()), "pad columns or guard bands overwritten: " + what
        return val


def _padded(t, pitch, off=0):
    """t [..., W] on the device inside rows of `pitch` elements at column `off`; the pad columns hold NaN."""
    out = torch.full(t.shape[:-1] + (pitch,), float("nan"), dtype=t.dtype)
    out[..., off:off + t.shape[-1]] = t
    return out.cuda()


def _upload(inp, cs):
    ce, C = chunk_elems(cs.dtype), cs.C
    es = 2 if cs.dtype == BF else 4
    d = types.SimpleNamespace(cs=cs, xp=C + 3 * ce if cs.pitched else C, gb=None, gbp=0, gptr=None, goff=0, st=None, stp=0, sptr=None,
                              soff=0, res=None)
    d.x, d.da = _padded(inp.x, d.xp), _padded(inp.da, d.xp)
    if cs.gb:
        d.gbp, d.goff = (2 * C + 2 * ce, ce) if cs.pitched else (2 * C, 0)
        d.gb = _padded(torch.cat([inp.gam, inp.bet], 2), d.gbp, d.goff)
        d.gptr = d.gb.data_ptr() + d.goff * es
    if cs.st:
        d.stp, d.soff = (2 * C + 8, 4) if cs.pitched else (2 * C, 0)
        d.st = _padded(inp.st, d.stp, d.soff)
        d.sptr = d.st.data_ptr() + d.soff * 4
    if cs.res:
        d.res = inp.res.cuda()
    return d


def _ok(rc, what):
    _lib.check(rc, what)


def _run_fwd(d, how, stats=None, N=None):
    """how: norm (s2p_in_norm_fwd), pair (s2p_in_stats + s2p_in_apply_fwd) or apply (s2p_in_apply_fwd on `stats`).  -> (y [N, HW, C], stats)"""
    L, cs, st = _lib.lib(), d.cs, _lib.stream()
    N = N or cs.N
    HW, C, dt = cs.HW, cs.C, dtype_id(cs.dtype)
    y = _Out(N * HW, d.xp, cs.dtype, 0, C)
    if stats is None:
        stats = Region(1, L.s2p_in_stats_floats(N, HW, C))
    if how == "norm":
        _ok(L.s2p_in_norm_fwd(dt, d.x.data_ptr(), N, HW, C, d.xp, d.gptr, d.gbp, d.sptr, d.stp, cs.act, SLOPE, EPS, y.ptr, d.xp, stats.ptr, st),
            "s2p_in_norm_fwd")
    else:
        if how == "pair":
            _ok(L.s2p_in_stats(dt, d.x.data_ptr(), N, HW, C, d.xp, EPS, stats.ptr, st), "s2p_in_stats")
        _ok(L.s2p_in_apply_fwd(dt, d.x.data_ptr(), N, HW, C, d.xp, stats.ptr, d.gptr, d.gbp, d.sptr, d.stp, cs.act, SLOPE, EPS, y.ptr, d.xp, st),
            "s2p_in_apply_fwd")
    return y.get("y").view(N, HW, C), stats


def _run_bwd(d, how, stats, N=None):
    """how: norm (s2p_in_norm_bwd_res) or pair (s2p_in_bwd_reduce + s2p_in_bwd_apply).  -> dict of the produced quantities (CPU)"""
    L, cs, st = _lib.lib(), d.cs, _lib.stream()
    N = N or cs.N
    HW, C, dt = cs.HW, cs.C, dtype_id(cs.dtype)
    dx = _Out(N * HW, d.xp, cs.dtype, 0, C)
    dgb = _Out(N * HW, d.gbp, cs.dtype, d.goff, 2 * C) if cs.gb else None
    dst = Region(N, 2 * C, pitch=d.stp, off=d.soff) if cs.st else None
    sums = Region(1, L.s2p_in_bwd_sums_floats(N, HW, C))
    common = (dt, d.da.data_ptr(), d.xp, d.x.data_ptr(), N, HW, C, d.xp, stats.ptr, d.gptr, d.gbp, d.sptr, d.stp, cs.act, SLOPE, EPS, sums.ptr)
    outs = (dx.ptr, d.xp, dgb.ptr if dgb else None, d.gbp, dst.ptr if dst else None, d.stp)
    if how == "norm":
        _ok(L.s2p_in_norm_bwd_res(*common, *outs, d.res.data_ptr() if cs.res else None, C if cs.res else 0, st), "s2p_in_norm_bwd_res")
    else:
        assert not cs.res
        _ok(L.s2p_in_bwd_reduce(*common, st), "s2p_in_bwd_reduce")
        _ok(L.s2p_in_bwd_apply(*common, *outs, st), "s2p_in_bwd_apply")
    got = dict(dx=dx.get("dx").view(N, HW, C))
    if dgb:
        g = dgb.get("dgb_img").view(N, HW, 2 * C)
        got.update(dgi=g[..., :C], dbi=g[..., C:])
    if dst:
        s = dst.bits("dgb_st")
        got.update(dgs=s[:, :C], dbs=s[:, C:])
    sums.get("sums")
    return got


def _word0(stats):
    return int(stats.bits("stats").view(torch.int32)[0, 0])


def _judge_bwd(cid, cs, form, inp, f, mask, got):
    ref, delta = _backward(inp, cs, f, mask, torch.float64, bounds=True)
    assert set(ref) == set(got)
    for q in ref:
        _check("gpu", form, cid, q, got[q], ref[q], _tol(ref[q], delta[q], OUT_DTYPE(cs, q)))


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_parity(hip_device, cid):
    cs, k = CASES[cid], _case(cid)
    ff, bf = _forms(cs)
    d = _upload(k.inp, cs)
    y, stats = _run_fwd(d, cs.how)
    y2, stats2 = _run_fwd(d, cs.how)
    assert torch.equal(y, y2) and torch.equal(stats.bits("stats"), stats2.bits("stats")), "forward not bit-identical on a second call"
    S = stats_splits(cs.N, cs.HW, cs.C)[0]
    if S > 1 or ff == "pair":
        assert _word0(stats) == (S if ff == "pair" else 1), (cid, ff, S)
    # the whole header, against the library's own answer for the case: {1, HW, 0, 0} exactly when its forward form is not the pair
    fused = cs.how == "norm" and lib_form(cs.dtype, cs.N, cs.HW, cs.C, cs.gb, cs.act, False) != "pair"
    hdr = stats.bits("stats").view(torch.int32)[0, :4].tolist()
    assert hdr == ([1, cs.HW, 0, 0] if fused else list(stats_splits(cs.N, cs.HW, cs.C)) + [0, 0]), (cid, hdr)
    _check("gpu", ff, cid, "y", y, k.f.y, _tol(k.f.y, k.dy, cs.dtype))
    if not cs.bwd:
        return
    mask = _mask_check(cid, cs, k, y)
    got = _run_bwd(d, cs.how, stats)
    got2 = _run_bwd(d, cs.how, stats)
    assert all(torch.equal(got[q], got2[q]) for q in got), "backward not bit-identical on a second call"
    _judge_bwd(cid, cs, bf, k.inp, k.f, mask, got)


@pytest.mark.gpu
def test_batch_prefix(hip_device):
    """The G step's "fake half of the D batch": forward apply and backward on the first 32 images of a 64-image statistics buffer (S = 2;
    the consumer's own launch geometry is S = 3), and with statistics of the 32 images alone: both inside the per-plane bounds."""
    cid = "e-prefix-fp32-n64-hw257-c512"
    cs64 = Case(F32, 64, 257, 512, "scaled", ACT_LRELU, how="pair")
    cs = cs64._replace(N=32)
    inp = _inputs(cid, cs64)
    d = _upload(inp, cs64)
    L = _lib.lib()
    full = Region(1, L.s2p_in_stats_floats(64, 257, 512))
    _ok(L.s2p_in_stats(dtype_id(F32), d.x.data_ptr(), 64, 257, 512, 512, EPS, full.ptr, _lib.stream()), "s2p_in_stats")
    assert _word0(full) == 2
    inp.x, inp.da = inp.x[:32], inp.da[:32]
    f = _forward(inp, cs, torch.float64)
    k = types.SimpleNamespace(inp=inp, f=f, dy=_delta_y(cid, cs, f))
    d.cs = cs
    for tag, stats in (("prefix-of-64", full), ("own-32", None)):
        y, stats = _run_fwd(d, "pair" if stats is None else "apply", stats)
        assert _word0(stats) == (2 if tag == "prefix-of-64" else 3)
        _check("gpu", "pair", cid + "-" + tag, "y", y, f.y, k.dy)
        mask = _mask_check(cid + "-" + tag, cs, k, y)
        _judge_bwd(cid + "-" + tag, cs, "pair", inp, f, mask, _run_bwd(d, "norm", stats))


@pytest.mark.gpu
def test_stats_across_forms(hip_device):
    """Statistics written by the fused s2p_in_norm_fwd (header {1, HW}) consumed by s2p_in_apply_fwd and by the explicit reduce + apply pair,
    whose own launch geometry would be S = 4."""
    cid = "e-cross-bf16-n3-hw400-c72"
    cs = Case(BF, 3, 400, 72, "scaled", ACT_LRELU)
    inp = _inputs(cid, cs)
    f = _forward(inp, cs, torch.float64)
    k = types.SimpleNamespace(inp=inp, f=f, dy=_delta_y(cid, cs, f))
    d = _upload(inp, cs)
    y0, stats = _run_fwd(d, "norm")
    hdr = stats.bits("stats").view(torch.int32)[0, :4].tolist()
    assert hdr == [1, 400, 0, 0], hdr
    tol = _tol(f.y, k.dy, BF)
    _check("gpu", "f512", cid, "y", y0, f.y, tol)
    y, _ = _run_fwd(d, "apply", stats)
    y2, _ = _run_fwd(d, "apply", stats)
    assert torch.equal(y, y2)
    _check("gpu", "pair", cid + "-apply", "y", y, f.y, tol)
    mask = _mask_check(cid, cs, k, y)
    got, got2 = _run_bwd(d, "pair", stats), _run_bwd(d, "pair", stats)
    assert all(torch.equal(got[q], got2[q]) for q in got)
    _judge_bwd(cid + "-pair", cs, "pair", inp, f, mask, got)


@pytest.mark.gpu
def test_empty_problems_and_null_pointers_are_refused(hip_device):
    """s2p_in_apply_fwd, s2p_in_bwd_reduce, s2p_in_bwd_apply and s2p_in_norm_bwd_res refuse N <= 0, HW <= 0 and a NULL required pointer before
    any launch (include/s2p_hip.h): return code -1 and a message; the outputs keep their sentinel."""
    L, st = _lib.lib(), _lib.stream()
    N, HW, C = 2, 9, 8
    t = lambda *s: torch.zeros(*s, device="cuda")
    x, da, stats, sums = t(N, HW, C), t(N, HW, C), t(64), t(256)
    out = _Out(N * HW, C, F32, 0, C)
    X, DA, ST, SM, O = x.data_ptr(), da.data_ptr(), stats.data_ptr(), sums.data_ptr(), out.ptr

    def fwd(x=X, stats=ST, y=O, N=N, HW=HW):
        return L.s2p_in_apply_fwd(0, x, N, HW, C, C, stats, None, 0, None, 0, ACT_NONE, SLOPE, EPS, y, C, st)

    def head(da, x, stats, sums, N, HW):
        return (0, da, C, x, N, HW, C, C, stats, None, 0, None, 0, ACT_NONE, SLOPE, EPS, sums)

    def reduce(da=DA, x=X, stats=ST, sums=SM, N=N, HW=HW):
        return L.s2p_in_bwd_reduce(*head(da, x, stats, sums, N, HW), st)

    def apply(da=DA, x=X, stats=ST, sums=SM, dx=O, N=N, HW=HW):
        return L.s2p_in_bwd_apply(*head(da, x, stats, sums, N, HW), dx, C, None, 0, None, 0, st)

    def both(da=DA, x=X, stats=ST, sums=SM, dx=O, N=N, HW=HW):
        return L.s2p_in_norm_bwd_res(*head(da, x, stats, sums, N, HW), dx, C, None, 0, None, 0, None, 0, st)

    calls = [(fwd, "s2p_in_apply_fwd", ("x", "stats", "y")), (reduce, "s2p_in_bwd_reduce", ("da", "x", "stats", "sums")),
             (apply, "s2p_in_bwd_apply", ("da", "x", "stats", "sums", "dx")), (both, "s2p_in_norm_bwd", ("da", "x", "stats", "dx"))]
    for fn, who, ptrs in calls:
        for kw in [dict(N=0), dict(N=-1), dict(HW=0), dict(HW=-3)] + [{p: None} for p in ptrs]:
            assert fn(**kw) == -1, (who, kw)
            msg = L.s2p_last_error().decode()
            assert who in msg and "null pointer / empty problem" in msg, (who, kw, msg)
    out.get("a refused call wrote")
    assert bool((sums == 0).all())


@pytest.mark.gpu
def test_zz_report(hip_device):
    print("\nworst |err| / tol per (launch form, quantity) on the device:")
    rows = {k: v for k, v in WORST.items() if k[0] == "gpu"}
    for key in sorted(rows):
        print("  %-7s %-4s %-4s %.3g" % (key[1], key[2], key[3], rows[key]))
    print("elements inside the branch band, all cases: %d (largest: %s)" % (sum(INBAND.values()), sorted(INBAND.items(), key=lambda kv: -kv[1])[:3]))
    print("swish a_act: %s" % SWISH_A)
    assert rows, "no parity case ran in this process: the table is filled by test_parity"
    assert all(v <= 1.0 for v in rows.values()), {k[1:]: v for k, v in rows.items() if not v <= 1.0}
