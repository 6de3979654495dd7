"""Op-level parity, per element, and exact impulse tests of the convs with a thin side: the generator stem (3 -> 64, 7x7 reflect), the
generator output conv (64 -> 3, 7x7 reflect, tanh), the conditioning conv (3 -> 1536), VGG conv1_1, the PatchGAN first layer and the
PatchGAN logit head -- the hand-written bf16 kernels of csrc/thin_conv.hip, csrc/thin_rows.hip and csrc/wgrad_head.hip.  The rows of
CONV_CASES in tests/test_kernels_gpu.py run these layers at batch <= 3, without an activation, in the max norm at 2e-2: every one of
them runs the row-streaming kernel with band = KS and no persistent wave walks a second tile.  The cases below are sized from the launch
rules so that the forms the train step runs are the forms the tests run.

CASES AND THE LAUNCH RULES THEY ARE PICKED FROM (restated in `rows_plan`, `walk`; test_case_geometry asserts the figures below from
those restatements, so a constant that moves in the library has to be moved there and names the case to re-pick):

  row-streaming kernel (thin_rows.hip: rows_launch): OPW = 32 - (KS - 1) outputs per wave, nw = min(cdiv(Wo, OPW), 4) waves,
  strip_out = OPW * nw, nstrips = cdiv(Wo, strip_out), band = cdiv(Ho, max(1, cdiv(256, N * nstrips))) raised to min(KS, Ho) when
  smaller, nq = cdiv(band + KS - 1, KS) rotations of the accumulator ring.
  persistent kernels: tiles = cdiv(pixels, 32); thin4_fwd_kernel (thin4_launch) runs 8 * min(cdiv(tiles, 8), max(256 / ncb, 32))
  waves, thin_cin_fwd_kernel (s2p_thin_cin_fwd) 4 * min(cdiv(tiles, 4), max(768 / ncb, 32)), ncb = cdiv(Cout, 64); wave v walks the
  tiles v, v + waves, v + 2 waves, ... and prefetches the next one (`cur = nxt`).
  7x7 64 -> 3 weight gradient (thin_conv.hip: s2p_thin_wgrad): H * W >= 1024 (tiled_applicable): thin_rows7_wgrad_kernel in
  cdiv(H, cdiv(H + 22, 23)) row bands when W + 6 <= 96 and H >= 7, thin_tiled_wgrad_kernel<25, 7, 64> when wider; below 1024 pixels
  thin_wgrad_kernel (fp32 atomics: no repeated-bits check there).

  id            layer (call form)                    N, H x W      what it reaches
  out-prod      64 -> 3 k7 reflect, bias, tanh       64, 84 x 30   rows fwd: band 21, 4 bands, nq 4, two waves.  Thin4 dgrad: 64 * 90 * 36 px =
                                                                   6480 tiles on 2048 waves.  wgrad: thin_rows7_wgrad_kernel, 4 bands of 21
  out-strips    same                                 22, 43 x 110  rows fwd: 2 strips (the second 6 columns wide), band 8, 6 bands, the last 3
                                                                   rows.  wgrad: W + 6 > 96, thin_tiled_wgrad_kernel<25, 7, 64>
  out-zero      64 -> 3 k7 zero pad, bias, lrelu 0.2 128, 30 x 27  rows fwd: band 15, 2 bands, nq 3, out-of-range loads.  wgrad: 810 px,
                                                                   thin_wgrad_kernel
  out-oneband   64 -> 3 k7 reflect, tanh (no bias)   256, 10 x 8   one band of 10 rows, nq 3.  wgrad: thin_wgrad_kernel
  out-tiny      same                                 3, 4 x 5      H < KS: band = H (pad 3 < 4 is the reflect limit).  wgrad: thin_wgrad_kernel
  stem-prod     3 -> 64 k7 reflect, bias, no act     19, 84 x 84   Thin4 fwd: 4190 tiles on 2048 waves (3 tiles for 94 waves, the last tile half
                                                                   full).  wgrad: s2p_stem_wgrad, 4 bands of 23 padded rows
  stem-small    same                                 3, 9 x 12     one (partial) tile per wave, reflect at H < 2 * pad + 4
  shared-prod   3 -> 1536 k3 p1, bias, relu          32, 21 x 21   ThinCin: 441 tiles, 24 channel blocks, 128 waves: 3-4 tiles per wave
  vgg11-prod    3 -> 64 k3 p1, bias, relu            64, 84 x 40   ThinCin: 6720 tiles on 3072 waves.  ThinRows dgrad (KS 3, flipped taps):
                                                                   band 21, nq 8, two waves
  vgg11-wide    same                                 128, 20 x 95  ThinRows dgrad: 4 waves, band 10
  d0            6 -> 64 k4 s2 p2, bias, lrelu 0.2    64, 84 x 70   ThinCin 4x4 stride 2: 3096 tiles on 3072 waves
  head-mfma     512 -> 1 k4 p2, bias, no act         3, 13 x 13    head_fwd_mfma_kernel (H * W <= 256)
  head-shfl     same                                 3, 16 x 17    head_fwd_kernel (H * W = 272, H <= 16)
  head-lanes    same                                 2, 17 x 17    thin_fwd_kernel<64> (H > 16)
  lanes-ragged  24 -> 4 k3 s2 p1, bias, relu         3, 11 x 9     thin_fwd_kernel<4> with 3 of 4 lanes live, stride 2
  tiled-static  64 -> 2 k7 reflect, bias, tanh       1, 33 x 37    thin_tiled_fwd_kernel<7, 64>, ragged edge tiles (16 x 8 tiles: 3 x 5 of them)

tiled-static has two output channels: with four, the 7x7 64-channel halo tile (22 * 14 * 144 B) plus the weights (4 * 49 * 128 B) plus the
output strip (2 KiB) is 71 488 B, over the 64 KiB of tiled_applicable, and the lanes-per-pixel kernel runs; with three it is the
row-streaming shape.  One or two output channels are what reaches thin_tiled_fwd_kernel<7, 64>.

Directions, as the model calls them: out: forward, plain dgrad (ops.conv_dgrad with its reflect fold), conv_wgrad(db=...); stem and
conditioning conv: forward and wgrad (their packs have need_bwd=False); conv1_1: forward and dgrad (VGG is frozen); d0: all three; head:
forward, dgrad, and the weight gradient through conv_wgrad_batched as ConvLayer.wgrad does; lanes-ragged, tiled-static: forward.

PATHS (test_paths, host only): the literal table PATHS of (forward, dgrad) answers of s2p_conv2d_path, the thin kind included
(_lib.thin_path), and every production shape -- bs 64 at 84 x 84 for G, D and VGG (conditioning conv: 21 x 21), bs 16 at 256 x 256 for the
rollout -- against the case that stands for it (STANDS_FOR).  The query plans with ACT_NONE; none of these layers uses swish.
The weight-gradient dispatcher has no query: the kernels named in the table above for the wgrad are read from the launch rules and
UNPINNED; the tests check the result, not the kernel's identity.

PARITY (test_parity): operands randn rounded to bf16, weights / sqrt(cin k^2), fp32 bias; reference F.conv2d in float64 (F.pad reflect
where the layer reflects), autograd for dx, dw, db, the activation in float64.  EVERY element must satisfy |got - ref| <= tol with
    P     = the same conv of |x|, |w| (+ |b|)            (the sum of the absolute terms of the element)
    K     = products per element: k^2 cin forward, k^2 cout dgrad, N Ho Wo for dw and db
    delta = 2 (K + 1) 2^-24 P + a_act
    tol   = delta + hu(|ref| + delta)      for the bf16 tensors,    tol = delta   for the fp32 dw / db,
    hu(v) = 2^(floor(log2 v) - 8), half a unit in the last place of bf16 in the binade of v.
(K + 1) 2^-24 sum|terms| is the any-order fp32 summation bound of DESIGN.md section 4, doubled to a whole ulp per addition because
the rounding inside one bf16 MFMA instruction is not documented; hu is one round-to-nearest-even bf16 store of a value within delta
of the truth; relu, lrelu (slope <= 1) and tanh are 1-Lipschitz, so delta passes through them; a_act = 2^-20 for tanh (1 - 2 rcp(1 +
exp(2x)): four fp32 operations on values <= 2, each within about 2 ulp; tanhf is tighter), 0 otherwise.  Nothing is measured into it.
WHY THE STORE TERM IS hu AND NOT 2^-9 (|ref| + delta), the form that reads naturally as "half an ulp".  bf16 keeps 8 significant bits:
half a unit in the last place is 2^-9 of the TOP of a binade and 2^-8 of its bottom, so a correctly rounded store of v = 2^e (1 + eps)
errs by up to 2^-8 |v|, twice that term.  test_reference_admits_fp32_accumulation shows it without a GPU: torch's own fp32 conv rounded
once to bf16 reaches 1.99 x the bound with the 2^-9 term (stem-small forward 1.88, head-mfma dgrad 1.99, out-tiny dgrad 1.51 with 70
of 3840 elements outside) and 0.999 x the bound with hu, which is exact for the number format and never above 2^-8 (|ref| + delta).
Every check prints its worst ratio against both forms; the assertion uses hu.
Reflect dgrad: the kernel produces the PADDED grid in bf16 (each element with the bf16 tol above, K = k^2 cout), and
s2p_reflect_pad_bwd (misc.hip: reflect_fold_kernel) reads the <= 3 x 3 padded elements that reflect onto an element as bf16, adds them
in fp32 and rounds once to bf16 at its store: delta_fold = fold(tol_pad) + 2 * 9 * 2^-24 fold(|ref_pad| + tol_pad), tol = delta_fold +
hu(|ref| + delta_fold), `fold` being the adjoint of F.pad(mode="reflect").
Besides: padded output channels are zeros; a second identical call gives the same bits (forward, dgrad, and the weight gradients that
reduce in a fixed order); the forward writes through `out=` into the middle of a sentinel-filled allocation (8 KiB on each side) and
leaves the sentinels alone.

ADMISSION (test_reference_admits_fp32_accumulation, CPU): at the cases with N <= 3, F.conv2d in fp32 + the activation in fp32 + one
bf16 rounding (and the fp32 autograd of dx, dw, db, the reflect dgrad through a bf16 padded grid) lies inside tol at every element: the
bound admits a correct fp32-accumulating implementation.  Worst ratio on the CPU: forward 0.988 (stem-small), dgrad 0.999 (the heads),
dw 0.008 (out-tiny), db 1e-4.

IMPULSE (test_impulse_*): exact, no tolerance.  One 1.0 per image; weights and bias non-zero integers in [-32, 32] / 64.  Every partial
sum is an integer below 2^24 in units of 2^-6: exact in fp32 in any order; the one bf16 store rounds the same exact number as the
float64 reference cast to bf16.  relu stays (exact), tanh / lrelu layers run with ACT_NONE.  Positions per case, from its geometry:
corners, (1, 1), (H-2, W-2), edge midpoints, centre; the rows j band - 1, j band of every band boundary; the columns OPW - 1, OPW,
strip_out - 1, strip_out; the 16 x 8 tile edges of the tiled kernel; for the persistent kernels the first and last pixel of the first
tile of a wave's second and third walk (pinned to the image they fall in).  Channels 0, 7, 8, 63, last.  Batches smaller than the
list take rounds.  fp32 (the generic kernel: a check of the reference's indexing) runs at the cases with N <= 3.

Worst observed |err| / tol on an MI355X: DESIGN.md section 6b.16 (printed by test_zz_report)."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from s2p_amd import _lib, ops
from s2p_amd._lib import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_TANH, chunk_elems
from test_kernels_gpu import nchw, nhwc, pack_bwd, pack_fwd

BF = torch.bfloat16
U24, U9, A_TANH = 2.0 ** -24, 2.0 ** -9, 2.0 ** -20
SLOPE = 0.2

# name -> (cin, cout, k, stride, pad, reflect, act, bias, dgrad, wgrad: None | "fused" (conv_wgrad(db=)) | "batched")
LAYERS = {
    "out": (64, 3, 7, 1, 3, True, ACT_TANH, True, True, "fused"),
    "out-nobias": (64, 3, 7, 1, 3, True, ACT_TANH, False, True, "fused"),
    "out-zero": (64, 3, 7, 1, 3, False, ACT_LRELU, True, True, "fused"),
    "stem": (3, 64, 7, 1, 3, True, ACT_NONE, True, False, "fused"),
    "shared": (3, 1536, 3, 1, 1, False, ACT_RELU, True, False, "fused"),
    "vgg11": (3, 64, 3, 1, 1, False, ACT_RELU, True, True, None),
    "d0": (6, 64, 4, 2, 2, False, ACT_LRELU, True, True, "fused"),
    "head": (512, 1, 4, 1, 2, False, ACT_NONE, True, True, "batched"),
    "ragged": (24, 4, 3, 2, 1, False, ACT_RELU, True, False, None),
    "tiled": (64, 2, 7, 1, 3, True, ACT_TANH, True, False, None),
}
# id -> (layer, N, H, W)
CASES = {
    "out-prod": ("out", 64, 84, 30), "out-strips": ("out", 22, 43, 110), "out-zero": ("out-zero", 128, 30, 27),
    "out-oneband": ("out-nobias", 256, 10, 8), "out-tiny": ("out-nobias", 3, 4, 5),
    "stem-prod": ("stem", 19, 84, 84), "stem-small": ("stem", 3, 9, 12), "shared-prod": ("shared", 32, 21, 21),
    "vgg11-prod": ("vgg11", 64, 84, 40), "vgg11-wide": ("vgg11", 128, 20, 95), "d0": ("d0", 64, 84, 70),
    "head-mfma": ("head", 3, 13, 13), "head-shfl": ("head", 3, 16, 17), "head-lanes": ("head", 2, 17, 17),
    "lanes-ragged": ("ragged", 3, 11, 9), "tiled-static": ("tiled", 1, 33, 37),
}
IDS = list(CASES)
SMALL = [c for c in IDS if CASES[c][1] <= 3]
BWD = [c for c in IDS if LAYERS[CASES[c][0]][8] or LAYERS[CASES[c][0]][9]]
# weight gradients that reduce in a fixed order (partial tiles + s2p_partial_reduce, or one workgroup per element); the others are
# thin_wgrad_kernel's fp32 atomics over many workgroups
WGRAD_FIXED_ORDER = {"out-prod", "out-strips", "stem-prod", "stem-small", "shared-prod", "d0", "head-mfma", "head-shfl", "head-lanes"}

_T = _lib.thin_path
_ROWS, _LANES = _T(_lib.THIN_ROWS), _T(_lib.THIN_LANES)
_T4, _CIN, _TR, _G = _lib.PATH_THIN4, _lib.PATH_THIN_CIN, _lib.PATH_THIN_ROWS, _lib.PATH_GENERIC
# case -> (forward, dgrad) answer of s2p_conv2d_path for the bf16 call; None: that direction is not run
PATHS = {
    "out-prod": (_ROWS, _T4), "out-strips": (_ROWS, _T4), "out-zero": (_ROWS, _T4), "out-oneband": (_ROWS, _T4), "out-tiny": (_ROWS, _T4),
    "stem-prod": (_T4, None), "stem-small": (_T4, None), "shared-prod": (_CIN, None),
    "vgg11-prod": (_CIN, _TR), "vgg11-wide": (_CIN, _TR), "d0": (_CIN, _G),
    "head-mfma": (_T(_lib.THIN_HEAD_MFMA), _G), "head-shfl": (_T(_lib.THIN_HEAD), _G), "head-lanes": (_LANES, _G),
    "lanes-ragged": (_LANES, None), "tiled-static": (_T(_lib.THIN_TILED), None),
}
# production launch (tests/test_host_logic.py::_step_conv_descs: the bs-64 84 x 84 step, the bs-16 256 x 256 rollout generator) -> its case
STANDS_FOR = {
    "G84/out": "out-prod", "G256/out": "out-strips", "G84/stem": "stem-prod", "G256/stem": "stem-prod",
    "G84/shared": "shared-prod", "G256/shared": "shared-prod", "VGG/conv1_1": "vgg11-prod",
    "D0/model0": "d0", "D1/model0": "d0", "D0/model4": "head-mfma", "D1/model4": "head-mfma",
}
# ... and, restated, the logit heads of a 256 x 256 discriminator (256 -> 129 -> 65 -> 33 -> 34 at scale 0, 128 -> ... -> 18 at scale 1)
HEADS_256 = [(16, 34, 34), (16, 18, 18)]
assert set(PATHS) == set(CASES)
WORST = {}


def _name(path):
    names = {v: k for k, v in vars(_lib).items() if k.startswith("PATH_")}
    kinds = {v: k for k, v in vars(_lib).items() if k.startswith("THIN_")}
    return "-1" if path < 0 else names[path & 0xff] + (":" + kinds[path >> 8] if path & 0xff == _lib.PATH_THIN else "")


def _geom(layer):
    cin, cout, k, s, p, refl = LAYERS[layer][:6]
    return ops.ConvGeom(cin, cout, k, s, p, reflect=refl)


def _out_hw(cid):
    layer, N, H, W = CASES[cid]
    return _geom(layer).out_hw(H, W)


def _plan(cid, dgrad, dtype=BF):
    layer, N, H, W = CASES[cid]
    cin_pad = ops.pad_to(LAYERS[layer][0], chunk_elems(dtype))
    return ops.conv_path(_geom(layer), dtype, (N, H, W, cin_pad), cin_pad, dgrad=dgrad)


# ---- the launch rules, restated ----------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def rows_plan(KS, N, Ho, Wo):
    """thin_rows.hip: rows_launch."""
    opw = 32 - (KS - 1)
    nw = min(cdiv(Wo, opw), 4)
    strip_out = opw * nw
    nstrips = cdiv(Wo, strip_out)
    band = cdiv(Ho, max(1, cdiv(256, N * nstrips)))
    if band < KS:
        band = min(KS, Ho)
    return dict(opw=opw, nw=nw, strip_out=strip_out, nstrips=nstrips, band=band, nbands=cdiv(Ho, band), nq=cdiv(band + KS - 1, KS))


def walk(kind, pixels, cout):
    """(tiles, waves) of the persistent thin-input kernels: thin4_launch / s2p_thin_cin_fwd."""
    tiles, ncb = cdiv(pixels, 32), cdiv(cout, 64)
    if kind == "thin4":
        return tiles, 8 * min(cdiv(tiles, 8), max(256 // ncb, 32))
    return tiles, 4 * min(cdiv(tiles, 4), max(768 // ncb, 32))


def r7_bands(H):
    """thin_conv.hip: r7_nbands, r7_band."""
    nb = (H + 22) // 23
    return nb, cdiv(H, nb)


def test_case_geometry():
    """The figures of the module docstring's case table, from the restated launch rules."""
    R = lambda cid, KS=7: rows_plan(KS, CASES[cid][1], *_out_hw(cid))
    r = R("out-prod")
    assert (r["band"], r["nbands"], r["nq"], r["nw"], r["nstrips"]) == (21, 4, 4, 2, 1)
    r = R("out-strips")
    assert (r["band"], r["nbands"], r["nstrips"], r["strip_out"], 43 - 5 * r["band"], 110 - r["strip_out"]) == (8, 6, 2, 104, 3, 6)
    r = R("out-zero")
    assert (r["band"], r["nbands"], r["nq"]) == (15, 2, 3)
    r = R("out-oneband")
    assert (r["band"], r["nbands"], r["nq"]) == (10, 1, 3)
    r = R("out-tiny")
    assert (r["band"], r["nbands"]) == (4, 1)
    r = R("vgg11-prod", 3)
    assert (r["band"], r["nq"], r["nw"]) == (21, 8, 2)
    r = R("vgg11-wide", 3)
    assert (r["band"], r["nw"]) == (10, 4)
    assert walk("thin4", 64 * 90 * 36, 64) == (6480, 2048)                     # the output conv's dgrad on the padded grid
    assert walk("thin4", 19 * 84 * 84, 64) == (4190, 2048) and 19 * 84 * 84 % 32 == 16 and 4190 - 2 * 2048 == 94
    assert walk("thin4", 3 * 9 * 12, 64) == (11, 16)
    assert walk("cin", 32 * 21 * 21, 1536) == (441, 128)
    assert walk("cin", 64 * 84 * 40, 64) == (6720, 3072)
    assert _out_hw("d0") == (43, 36) and walk("cin", 64 * 43 * 36, 64) == (3096, 3072)
    assert r7_bands(84) == (4, 21) and r7_bands(90) == (4, 23) and 110 + 6 > 96 and 30 * 27 < 1024 <= 43 * 110
    # tiled_applicable's LDS: halo tile + weights + output strip against 64 KiB, for 4 / 3 / 2 output channels of the 7x7 64-channel conv
    lds = lambda cout: 22 * 14 * (64 * 2 + 16) + cout * 49 * 64 * 2 + 16 * 8 * 16
    assert lds(4) == 71488 > 65536 >= lds(3) > lds(2) and 33 * 37 >= 1024 and (cdiv(33, 8), cdiv(37, 16)) == (5, 3)


# ---- (a) paths -------------------------------------------------------------------------------------------------------------------------
def test_paths():
    """Host only (s2p_conv2d_path launches nothing): the literal table, fp32 on the generic kernel, the layers against the networks' own
    constructors, and every production shape against the case that stands for it."""
    for cid, want in PATHS.items():
        for dgrad, direction in enumerate(("forward", "dgrad")):
            layer = CASES[cid][0]
            assert (want[dgrad] is not None) == (True if not dgrad else LAYERS[layer][8]), cid
            if want[dgrad] is not None:
                got = _plan(cid, bool(dgrad))
                assert got == want[dgrad], "%s %s: plans %s, the table says %s" % (cid, direction, _name(got), _name(want[dgrad]))
                if CASES[cid][1] <= 3:
                    assert _plan(cid, bool(dgrad), torch.float32) == _G, "%s %s, fp32" % (cid, direction)
    from test_host_logic import _step_conv_descs
    L = _lib.lib()
    descs = dict(_step_conv_descs())
    assert set(STANDS_FOR) <= set(descs)
    for name, cid in STANDS_FOR.items():
        d = descs[name]
        cin, cout, k, s, p, refl = LAYERS[CASES[cid][0]][:6]
        assert (d.cin_real, d.Cout, d.KH, d.KW, d.stride, d.pad, d.reflect) == (cin, cout, k, k, s, p, int(refl)), \
            "%s is not the layer of %s any more" % (name, cid)
        for dgrad, direction in enumerate(("forward", "dgrad")):
            want = PATHS[cid][dgrad]
            if want is not None:
                got = int(L.s2p_conv2d_path(ctypes.byref(d), dgrad, 1))
                assert got == want, ("%s %s: production plans %s, the case %s runs %s -- pick another case" %
                                     (name, direction, _name(got), cid, _name(want)))
    for N, H, W in HEADS_256:
        for dgrad in (0, 1):
            got = ops.conv_path(_geom("head"), BF, (N, H, W, 512), 512, dgrad=bool(dgrad))
            assert got == PATHS["head-lanes"][dgrad], "head at %d x %d x %d: plans %s, head-lanes runs %s" % (
                N, H, W, _name(got), _name(PATHS["head-lanes"][dgrad]))


# ---- references ----------------------------------------------------------------------------------------------------------------------
def _conv(layer, x, w, b=None, keep=None):
    """keep: a list that receives the reflect-padded input, its gradient retained (the padded grid of the dgrad)."""
    cin, cout, k, s, p, refl = LAYERS[layer][:6]
    if refl:
        xp = F.pad(x, (p, p, p, p), mode="reflect")
        if keep is not None:
            xp.retain_grad()
            keep.append(xp)
        return F.conv2d(xp, w, b, stride=s)
    return F.conv2d(x, w, b, stride=s, padding=p)


def _act(layer, t):
    act = LAYERS[layer][6]
    return torch.tanh(t) if act == ACT_TANH else F.relu(t) if act == ACT_RELU else F.leaky_relu(t, SLOPE) if act == ACT_LRELU else t


def _fold(t, p):
    """The adjoint of F.pad(mode="reflect"): the padded-grid tensor t folded onto the image."""
    z = torch.zeros(t.shape[0], t.shape[1], t.shape[2] - 2 * p, t.shape[3] - 2 * p, dtype=t.dtype, requires_grad=True)
    F.pad(z, (p, p, p, p), mode="reflect").backward(t)
    return z.grad


def _dw_layout(g):
    return g.permute(0, 2, 3, 1).reshape(g.shape[0], g.shape[2] * g.shape[3], g.shape[1])


def _half_ulp_bf16(v):
    """Half a unit in the last place of bf16 (8 significant bits) in the binade of v >= 0: 2^(floor(log2 v) - 8); 0 at 0."""
    return torch.exp2(torch.floor(torch.log2(v)) - 8)


def _tol_bf16(ref, delta, literal=False):
    """delta + one round-to-nearest-even bf16 store of a value within delta of ref.  literal: the store term as 2^-9 (|ref| + delta)."""
    return delta + (U9 * (ref.abs() + delta) if literal else _half_ulp_bf16(ref.abs() + delta))


@functools.lru_cache(maxsize=2)
def _operands(cid):
    """bf16-rounded operands of one case and, in float64, the references and the per-element tolerances of every quantity it runs:
    dict qty -> (ref, tol), plus the operands.  Computed once per case, shared by the tests that need it, never modified."""
    layer, N, H, W = CASES[cid]
    cin, cout, k, s, p, refl, act, has_bias, dgrad, wgrad = LAYERS[layer]
    g = torch.Generator().manual_seed(3000 + IDS.index(cid))
    rnd = lambda t: t.bfloat16().float()
    x = rnd(torch.randn(N, cin, H, W, generator=g))
    w = rnd(torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k))
    b = torch.randn(cout, generator=g) if has_bias else None
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    xa, wa = x.double().abs().requires_grad_(True), w.double().abs().requires_grad_(True)
    padded = []
    lin = _conv(layer, xr, wr, b.double() if has_bias else None, padded)
    lin_abs = _conv(layer, xa, wa, b.double().abs() if has_bias else None, padded)
    out = dict(x=x, w=w, b=b)
    delta = 2 * (k * k * cin + 1) * U24 * lin_abs.detach() + (A_TANH if act == ACT_TANH else 0.0)
    y_ref = _act(layer, lin.detach())
    out["fwd"] = (y_ref, _tol_bf16(y_ref, delta), _tol_bf16(y_ref, delta, True))
    if dgrad or wgrad:
        dy = rnd(torch.randn(lin.shape, generator=g))
        out["dy"] = dy
        lin.backward(dy.double())
        lin_abs.backward(dy.double().abs())
        if dgrad:
            K = k * k * cout
            if refl:
                pad_ref, pad_abs = padded[0].grad, padded[1].grad                           # the padded grid, (H + 2p) x (W + 2p)
                assert float((_fold(pad_ref, p) - xr.grad).abs().max()) < 1e-12
                tols = []
                for literal in (False, True):
                    tol_pad = _tol_bf16(pad_ref, 2 * (K + 1) * U24 * pad_abs, literal)
                    d_fold = _fold(tol_pad, p) + 2 * 9 * U24 * _fold(pad_ref.abs() + tol_pad, p)
                    tols.append(_tol_bf16(xr.grad, d_fold, literal))
                out["dgrad"] = (xr.grad, tols[0], tols[1])
            else:
                delta = 2 * (K + 1) * U24 * xa.grad
                out["dgrad"] = (xr.grad, _tol_bf16(xr.grad, delta), _tol_bf16(xr.grad, delta, True))
        if wgrad:
            K = N * lin.shape[2] * lin.shape[3]
            out["dw"] = (_dw_layout(wr.grad), 2 * (K + 1) * U24 * _dw_layout(wa.grad))
            out["db"] = (dy.double().sum((0, 2, 3)), 2 * (K + 1) * U24 * dy.double().abs().sum((0, 2, 3)))
    return out


def _check(cid, qty, got, ref, tol, tol_literal=None, where="gpu"):
    """|got - ref| <= tol at EVERY element; notes and prints the worst |err| / tol (and, for the record, against the bound with the
    store term written as 2^-9 (|ref| + delta): see the module docstring)."""
    err = (got.double() - ref).abs()
    bad = (~(err <= tol)).nonzero()          # a NaN or an infinity is outside every bound: `err > tol` would let a NaN through

    def worst(t):                            # (a NaN ratio counts as infinite: max() would drop it)
        r = err / t.clamp_min(1e-300)
        return float(r.max()) if bool(torch.isfinite(r).all()) else math.inf
    ratio = worst(tol)
    lit = worst(tol_literal) if tol_literal is not None else ratio
    WORST[(where, cid, qty)] = max(WORST.get((where, cid, qty), 0.0), ratio)
    WORST[(where + "-literal", cid, qty)] = max(WORST.get((where + "-literal", cid, qty), 0.0), lit)
    print("%s %-12s %-5s worst |err| / tol %.3g (with a 2^-9 store term %.3g; max |err| %.3e, max |ref| %.3e)" % (
        where, cid, qty, ratio, lit, float(err.max()), float(ref.abs().max())))
    assert len(bad) == 0, "%s %s: %d of %d elements outside the bound, the first at %s: got %r, ref %r, tol %.3e; worst |err| / tol %.3f" % (
        cid, qty, len(bad), err.numel(), bad[0].tolist(), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])]), float(tol[tuple(bad[0])]), ratio)


# ---- device helpers --------------------------------------------------------------------------------------------------------------------
GUARD = 4096           # elements on each side of a guarded output: 8 KiB of bf16


def _guarded(shape, dtype, dev):
    """A view of `shape` in the middle of a sentinel-filled allocation, 16-byte aligned, and the allocation."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), -7.5, dtype=dtype, device=dev)
    view = buf[GUARD:GUARD + n].view(shape)
    assert view.data_ptr() % 16 == 0 and GUARD * buf.element_size() >= 4096
    return view, buf


def _guards_intact(buf):
    return bool((buf[:GUARD] == -7.5).all()) and bool((buf[-GUARD:] == -7.5).all())


def _device_weights(layer, w, dtype, dev):
    cin, cout = LAYERS[layer][:2]
    ce = chunk_elems(dtype)
    cin_pad, cout_pad = ops.pad_to(cin, ce), ops.pad_to(cout, ce)
    return pack_fwd(w, cin_pad, dtype, dev), pack_bwd(w, cin_pad, cout_pad, dtype, dev), cin_pad, cout_pad


def _wgrad(layer, xd, dyd, cin_pad, dev):
    """dw, db as the model produces them: ConvLayer.wgrad -- the bias gradient fused into conv_wgrad, the logit head through the batched entry."""
    cin, cout, k = LAYERS[layer][:3]
    dw = torch.zeros((cout, k * k, cin), dtype=torch.float32, device=dev)
    db = torch.zeros(cout, dtype=torch.float32, device=dev)
    if LAYERS[layer][9] == "batched" and xd.dtype == BF:
        ops.conv_wgrad_batched(_geom(layer), [(xd, 0, dyd, 0, dw, db)], cin_pad, cin, cout)
    else:
        ops.conv_wgrad(_geom(layer), xd, dyd, dw, cin_pad, cin, cout, db=db)
    torch.cuda.synchronize()
    return dw.cpu(), db.cpu()


# ---- (b) parity, per element ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_parity(hip_device, cid):
    layer, N, H, W = CASES[cid]
    cin, cout, k, s, p, refl, act, has_bias, dgrad, wgrad = LAYERS[layer]
    dev = hip_device
    o = _operands(cid)
    geom = _geom(layer)
    Ho, Wo = geom.out_hw(H, W)
    wf, wb, cin_pad, cout_pad = _device_weights(layer, o["w"], BF, dev)
    xd = nhwc(o["x"], cin_pad, BF, dev)
    bd = o["b"].to(dev) if has_bias else None
    # forward, in the layer's own call form, into a guarded output
    y, buf = _guarded((N, Ho, Wo, cout_pad), BF, dev)
    assert ops.conv_fwd(geom, xd, wf, bd, cin_pad, act=act, slope=SLOPE, out=y) is y
    y2 = ops.conv_fwd(geom, xd, wf, bd, cin_pad, act=act, slope=SLOPE)
    torch.cuda.synchronize()
    assert _guards_intact(buf), "the forward wrote outside its output"
    _check(cid, "fwd", nchw(y, cout), *o["fwd"])
    assert torch.equal(y, y2), "two identical forward calls differ"
    if cout_pad > cout:
        assert float(y[..., cout:].float().abs().max()) == 0.0, "padded output channels are not zeros"
    if dgrad or wgrad:
        dyd = nhwc(o["dy"], cout_pad, BF, dev)
    if dgrad:
        dx = ops.conv_dgrad(geom, dyd, wb, tuple(xd.shape), cin_pad)
        dx2 = ops.conv_dgrad(geom, dyd, wb, tuple(xd.shape), cin_pad)
        torch.cuda.synchronize()
        _check(cid, "dgrad", nchw(dx, cin), *o["dgrad"])
        assert torch.equal(dx, dx2), "two identical dgrad calls differ"
        if cin_pad > cin:        # the padded input channels have zero rows in w_bwd
            assert float(dx[..., cin:].float().abs().max()) == 0.0, "padded channels of dx are not zeros"
    if wgrad:
        dw, db = _wgrad(layer, xd, dyd, cin_pad, dev)
        _check(cid, "dw", dw, *o["dw"])
        _check(cid, "db", db, *o["db"])
        if cid in WGRAD_FIXED_ORDER:
            dw2, db2 = _wgrad(layer, xd, dyd, cin_pad, dev)
            assert torch.equal(dw, dw2) and torch.equal(db, db2), "two identical weight-gradient calls differ"


# ---- (c) the bound admits fp32 accumulation (CPU) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", SMALL)
def test_reference_admits_fp32_accumulation(cid):
    """F.conv2d in fp32 on the same bf16-rounded operands, the activation in fp32, one rounding to bf16 -- and the fp32 autograd of dx
    (through a bf16 padded grid where the layer reflects), dw, db -- lie inside tol at every element.  Worst |err| / tol over the
    seven cases on the CPU: forward 0.988 (stem-small), dgrad 0.999 (the heads), dw 0.008 (out-tiny), db 1e-4; against the bound with
    the store term as 2^-9 (|ref| + delta): forward 1.88, dgrad 1.99 -- a correctly rounded bf16 store does not fit that form."""
    layer, N, H, W = CASES[cid]
    cin, cout, k, s, p, refl, act, has_bias, dgrad, wgrad = LAYERS[layer]
    o = _operands(cid)
    x, w = o["x"].clone().requires_grad_(True), o["w"].clone().requires_grad_(True)
    lin = _conv(layer, x, w, o["b"])
    _check(cid, "fwd", _act(layer, lin.detach()).bfloat16().float(), *o["fwd"], where="cpu")
    if dgrad or wgrad:
        lin.backward(o["dy"])
    if dgrad:
        if refl:
            pad = F.conv_transpose2d(o["dy"], o["w"]).bfloat16().float()
            dx = _fold(pad, p).bfloat16().float()
        else:
            dx = x.grad.bfloat16().float()
        _check(cid, "dgrad", dx, *o["dgrad"], where="cpu")
    if wgrad:
        _check(cid, "dw", _dw_layout(w.grad), *o["dw"], where="cpu")
        _check(cid, "db", o["dy"].sum((0, 2, 3)), *o["db"], where="cpu")


# ---- (d) exact impulse tests -----------------------------------------------------------------------------------------------------------
def _generic(H, W):
    e, f, mh, mw = H - 1, W - 1, H // 2, W // 2
    pos = [(0, 0), (0, f), (e, 0), (e, f), (1, 1), (H - 2, W - 2), (0, mw), (mh, 0), (mh, f), (e, mw), (mh, mw)]
    return [(r, c) for r, c in pos if 0 <= r < H and 0 <= c < W]


def _band_rows(band, H, W):
    cols = (0, W // 2, W - 1)
    rows = [r for j in range(1, cdiv(H, band)) for r in (j * band - 1, j * band)]
    return [(r, cols[i % 3]) for i, r in enumerate(rows) if 0 <= r < H]


def _strip_cols(plan, H, W):
    cols = [c for c in (plan["opw"] - 1, plan["opw"], plan["strip_out"] - 1, plan["strip_out"]) if c < W]
    rows = (H // 2, 0, H - 1, H // 3)
    return [(rows[i % 4], c) for i, c in enumerate(cols)]


def _walk_pins(kind, N, Hg, Wg, cout, to_pos):
    """First and last pixel of the first tile of a wave's second and third walk (tiles `waves` and 2 `waves`), as (image, row, col) with
    the (row, col) of the produced grid Hg x Wg mapped to the impulse tensor by `to_pos`."""
    M = N * Hg * Wg
    tiles, waves = walk(kind, M, cout)
    pins = []
    for t in (waves, 2 * waves):
        if t < tiles:
            for m in (32 * t, min(32 * t + 31, M - 1)):
                n, rr = divmod(m, Hg * Wg)
                pins.append((n,) + to_pos(*divmod(rr, Wg)))
    return pins


def _positions(cid, what):
    """(positions, pins) of the impulse tensor of `what`: "fwd" (an impulse in x), "dgrad", "wgrad" (an impulse in dy)."""
    layer, N, H, W = CASES[cid]
    cin, cout, k, s, p, refl = LAYERS[layer][:6]
    Ho, Wo = _out_hw(cid)
    base = layer.split("-")[0]
    clip = lambda v, n: max(0, min(n - 1, v))
    if what == "fwd":
        pos, pins = _generic(H, W), []
        if base == "out":
            plan = rows_plan(7, N, Ho, Wo)
            pos += _band_rows(plan["band"], H, W) + _strip_cols(plan, H, W)
        elif base == "stem":
            pins = _walk_pins("thin4", N, Ho, Wo, cout, lambda r, c: (r, c))
        elif base in ("shared", "vgg11", "d0"):
            pins = _walk_pins("cin", N, Ho, Wo, cout, lambda r, c: (clip(r * s, H), clip(c * s, W)))
        elif base == "tiled":
            pos += [(7, 15), (8, 16), (7, 16), (8, 15), (31, 31), (32, 32)]                # the 16 x 8 tile edges
        return pos, pins
    pos, pins = _generic(Ho, Wo), []
    if what == "dgrad":
        if base == "out":         # Thin4 over the produced grid: the padded one under reflect (image coordinate = padded - 3)
            e = 6 if refl else 0
            pins = _walk_pins("thin4", N, H + e, W + e, cin, lambda r, c: (clip(r - e // 2, Ho), clip(c - e // 2, Wo)))
        elif base == "vgg11":     # the row-streaming kernel over dy, producing H x W
            plan = rows_plan(3, N, H, W)
            pos += _band_rows(plan["band"], Ho, Wo) + _strip_cols(plan, Ho, Wo)
    else:
        if base == "out" and H >= 7:
            pos += _band_rows(r7_bands(H)[1], Ho, Wo)
        elif base == "stem":      # bands of the padded grid: padded row = image row + 3
            band = r7_bands(H + 6)[1]
            pos += [(r - 3, c) for r, c in _band_rows(band, H + 6, Wo) if 0 <= r - 3 < Ho]
    return pos, pins


def _channels(C):
    return list(dict.fromkeys(c for c in (0, 7, 8, 63, C - 1) if c < C))


def _rounds(N, pos, pins, centre):
    """Per round {image: (row, col)}: an image carries one position; pins keep their image, the list fills the others in order."""
    pos, pins, out = list(pos), list(pins), []
    while pos or pins:
        rnd, rest = {}, []
        for n, r, c in pins:
            if n in rnd:
                rest.append((n, r, c))
            else:
                rnd[n] = (r, c)
        pins = rest
        for n in range(N):
            if n not in rnd:
                rnd[n] = pos.pop(0) if pos else centre
        out.append(rnd)
    return out


def _impulses(N, C, H, W, rnd, first):
    t = torch.zeros(N, C, H, W)
    Cs = _channels(C)
    for n, (r, c) in rnd.items():
        t[n, Cs[(first + n) % len(Cs)], r, c] = 1.0
    return t


TAPS = lambda k: [(0, 0), (0, k - 1), (k // 2, k // 2), (k - 1, 0), (k - 1, k - 1)]


@functools.lru_cache(maxsize=2)
def _impulse_operands(cid):
    """Integer / 64 weights and bias and the float64 references of one case, shared by its dtypes: per round (x, y64) for the forward,
    (dy, dx64) for the dgrad and (x, dy, dw64, db64) for the weight gradient."""
    layer, N, H, W = CASES[cid]
    cin, cout, k, s, p, refl, act, has_bias, dgrad, wgrad = LAYERS[layer]
    Ho, Wo = _out_hw(cid)
    g = torch.Generator().manual_seed(4000 + IDS.index(cid))
    ints = lambda *shape: (torch.randint(1, 33, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float() / 64
    w, b = ints(cout, cin, k, k), ints(cout)
    relu = F.relu if act == ACT_RELU else (lambda t: t)
    fwd, dgr, wgr = [], [], []
    pos, pins = _positions(cid, "fwd")
    for i, rnd in enumerate(_rounds(N, pos, pins, (H // 2, W // 2))):
        x = _impulses(N, cin, H, W, rnd, i)
        with torch.no_grad():
            fwd.append((x, relu(_conv(layer, x.double(), w.double(), b.double()))))
    if dgrad:
        pos, pins = _positions(cid, "dgrad")
        for i, rnd in enumerate(_rounds(N, pos, pins, (Ho // 2, Wo // 2))):
            dy = _impulses(N, cout, Ho, Wo, rnd, i)
            xr = torch.zeros(N, cin, H, W, dtype=torch.float64, requires_grad=True)
            _conv(layer, xr, w.double()).backward(dy.double())
            dgr.append((dy, xr.grad))
    if wgrad:
        pos, pins = _positions(cid, "wgrad")
        into = (lambda v, n: max(0, min(n - 1, -v if v < 0 else 2 * n - 2 - v if v >= n else v))) if refl else (lambda v, n: max(0, min(n - 1, v)))
        for i, rnd in enumerate(_rounds(N, pos, pins, (Ho // 2, Wo // 2))):
            dy = _impulses(N, cout, Ho, Wo, rnd, i)
            # the impulse of x one tap away from the one of dy: tap n % 5 of five; a position outside the image is reflected where the
            # layer reflects (the tap stays) and clamped where it pads with zeros (another, valid tap: 0 <= pad - r s <= k - 1), so every
            # image lands in some dw element and images that share a position and a tap add up in one
            xpos = {n: (into(r * s - p + TAPS(k)[n % 5][0], H), into(c * s - p + TAPS(k)[n % 5][1], W)) for n, (r, c) in rnd.items()}
            x = _impulses(N, cin, H, W, xpos, i)
            wr = w.double().requires_grad_(True)
            _conv(layer, x.double(), wr).backward(dy.double())
            wgr.append((x, dy, _dw_layout(wr.grad), dy.double().sum((0, 2, 3))))
    return w, b, fwd, dgr, wgr


def _assert_same(got, ref64, dtype, what):
    """Equal as numbers to the float64 reference cast to the dtype."""
    want = ref64.to(dtype).float()
    bad = (got != want).nonzero()
    assert len(bad) == 0, "%s: %d elements differ, the first at %s: got %r, expected %r" % (
        what, len(bad), bad[0].tolist(), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))


def _dtypes(cid):
    return [torch.float32, BF] if CASES[cid][1] <= 3 else [BF]


IMPULSE = [(c, dt) for c in IDS for dt in _dtypes(c)]
IMPULSE_IDS = ["%s-%s" % (c, "bf16" if dt == BF else "fp32") for c, dt in IMPULSE]
IMPULSE_BWD = [(c, dt) for c, dt in IMPULSE if c in BWD]


@pytest.mark.gpu
@pytest.mark.parametrize("cid,dtype", IMPULSE, ids=IMPULSE_IDS)
def test_impulse_forward(hip_device, cid, dtype):
    layer, N, H, W = CASES[cid]
    cout, act = LAYERS[layer][1], LAYERS[layer][6]
    dev = hip_device
    w, b, fwd, _, _ = _impulse_operands(cid)
    wf, _, cin_pad, cout_pad = _device_weights(layer, w, dtype, dev)
    for x, y64 in fwd:
        assert float(y64.abs().max()) > 0
        y = ops.conv_fwd(_geom(layer), nhwc(x, cin_pad, dtype, dev), wf, b.to(dev), cin_pad, act=ACT_RELU if act == ACT_RELU else ACT_NONE)
        torch.cuda.synchronize()
        _assert_same(nchw(y, cout), y64, dtype, "%s forward, (n, c, y, x)" % cid)
        if cout_pad > cout:
            assert float(y[..., cout:].float().abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("cid,dtype", IMPULSE_BWD, ids=["%s-%s" % (c, "bf16" if dt == BF else "fp32") for c, dt in IMPULSE_BWD])
def test_impulse_dgrad_wgrad(hip_device, cid, dtype):
    """Plain dgrad of an impulse in dy: the weights laid out around it (summed where the reflect fold brings several onto one element).
    Weight gradient of an impulse in x and one in dy per image: dw counts the images whose impulses meet in one (tap, channel pair),
    db the impulses per channel -- small integers, exact."""
    layer, N, H, W = CASES[cid]
    cin, cout = LAYERS[layer][:2]
    dev = hip_device
    w, _, _, dgr, wgr = _impulse_operands(cid)
    _, wb, cin_pad, cout_pad = _device_weights(layer, w, dtype, dev)
    for dy, dx64 in dgr:
        assert float(dx64.abs().max()) > 0
        dx = ops.conv_dgrad(_geom(layer), nhwc(dy, cout_pad, dtype, dev), wb, (N, H, W, cin_pad), cin_pad)
        torch.cuda.synchronize()
        _assert_same(nchw(dx, cin), dx64, dtype, "%s dx, (n, c, y, x)" % cid)
    for x, dy, dw64, db64 in wgr:
        assert float(dw64.sum()) >= N and float(db64.sum()) == N            # every image lands in a dw element (in several through a reflection)
        dw, db = _wgrad(layer, nhwc(x, cin_pad, dtype, dev), nhwc(dy, cout_pad, dtype, dev), cin_pad, dev)
        _assert_same(dw, dw64, torch.float32, "%s dw, (row, tap, col)" % cid)
        _assert_same(db, db64, torch.float32, "%s db" % cid)


@pytest.mark.gpu
def test_zz_report(hip_device):
    print("\nworst |err| / tol per (case, quantity), bf16 on the device:")
    rows = {k: v for k, v in WORST.items() if k[0] == "gpu"}
    for key in sorted(rows):
        print("  %-13s %-5s %.3g   (with a 2^-9 store term: %.3g)" % (key[1], key[2], rows[key], WORST[("gpu-literal",) + key[1:]]))
    assert rows, "no parity case ran in this process: the table is filled by test_parity"
    assert all(v < 1.0 for v in rows.values()), {k[1:]: v for k, v in rows.items() if not v < 1.0}
