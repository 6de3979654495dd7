"""Op-level parity of the twelve SLAC encoder / decoder conv layers (s2p_amd/slac.py: ENCODER_100, DECODER_100), one layer at a
time, at the map size each layer has in the model and called the way `_StackFn` calls it.  tests/test_slac.py and
tests/test_slac_latent.py reach these layers only through whole stacks, at 4 / 36 images, in the max norm at 4e-2 / 1e-1 (bf16):
one wrong border pixel, one wrong tap of one sub-pixel phase or one wrong last channel chunk of one layer passes there.

Which kernel each case reaches (bf16; fp32 is the generic gather kernel everywhere).  `test_paths_match_production` pins this table
(SLAC_PATHS) on the host, and pins that every production batch -- 1 (actor), 288 (latent step, forward and backward), 2304 (no-grad
encode) -- plans the same path as the test batch that stands for it, so a moved dispatcher threshold names the batch to re-pick:

  layer, map                               N    forward               dgrad
  enc0 conv    3 ->  32 k5 s2     100->50  3    generic               generic (plain dgrad: the first layer of its stack)
  enc1 conv   32 ->  64 k3 s2      50->25  3    generic (Cin % 64)    generic
  enc2 conv   64 -> 128 k3 s2      25->13  3    LDS-DMA               merged phases (four phases of unequal size: 25 = 13 + 12)
  enc3 conv  128 -> 256 k3 s2      13->7   3    LDS-DMA               merged phases (13 = 7 + 6)
  enc4 conv  256 -> 256 k3 s2       7->4   3    split-K               merged phases (7 = 4 + 3)
                                           641  LDS-DMA               --  (forward only: the no-grad encode's form, N > 640)
  enc5 conv  256 -> 256 k4 p0       4->1   3    split-K               split-K
                                           32   plane (generalised)   plane (generalised): several images per workgroup
                                           34   plane (generalised)   plane (generalised): ... 17 workgroup planes, the plain block order
                                           64   plane (generalised)   plane (generalised): ... four images per workgroup (see below)
  dec0 convT 288 -> 256 k4 p0       1->4   3    generic (Cin % 64)    split-K (plain dgrad)
  dec1 convT 256 -> 256 k3 s2       4->7   3    merged phases         split-K
  dec2 convT 256 -> 128 k3 s2       7->13  3    merged phases         LDS-DMA
  dec3 convT 128 ->  64 k3 s2      13->25  3    merged phases         LDS-DMA
  dec4 convT  64 ->  32 k3 s2 op1  25->50  3    generic (Cout <= 32)  generic (gathers 32 channels of dy)
  dec5 convT  32 ->   3 k5 s2 op1  50->100 3    generic               generic

The path query does not tell how many images the generalised plane kernel stacks per workgroup on enc5 (csrc/conv_planeg.hip:
pg_pick_shape -- the largest G of 4, 2 that divides N and leaves 16 workgroup planes).  Read from that code: 32 and 34 give G = 2 (16
planes in the XCD-aware block order, 17 in the plain one); 288 and 2304, the production batches, give G = 4, in both directions.
N = 64 is the smallest batch with G = 4, so it runs beside 32 and 34 (its float64 reference is 1 % of the N = 641 one).

The weight-gradient dispatcher has no query: the wgrad path is UNPINNED.  The wgrad cases below run whatever kernel the library picks
for `deterministic=True` at these shapes; they check its result, not its identity.

Parity (test_parity): forward = bias + LeakyReLU(0.2) in the epilogue; dgrad = EPI_MUL_ACTGRAD with the layer's input as `aux`
(exact zeros and negative values planted at the four corners and in the last real channel), plain for the first layer of a stack;
wgrad = deterministic, `db` fused for the conv layers, `channel_sum(deterministic=True)` for the transposed ones.  Reference: float64
F.conv2d / F.conv_transpose2d + autograd on the CPU (on bf16-rounded operands for bf16); the dgrad reference is
dgrad64 * where(aux > 0, 1, slope), the formula of the epilogue, so no activation kink is involved.  Tolerance: TOL of
tests/test_kernels_gpu.py (1e-5 / 2e-2, max-norm relative).  Padded output channels must be zeros, a repeated call the same bits.

Impulse tests (test_impulse_*): EXACT BY CONSTRUCTION, no tolerance.  Image n carries a single 1.0 at one of nine positions (corners,
edge midpoints, centre) in one of the channels 0 / 63 / 64 / last; weights are bf16-representable, the bias is zero, there is no
activation.  Every output element is then a sum with at most ONE non-zero term, 1.0 * w: the product is exact in fp32, adding zeros
to it is exact in any order (so also across split-K partials and sub-pixel phases), and w survives the bf16 store because it is a
bf16 number.  The output therefore equals the float64 reference cast to the dtype as numbers (torch.equal: -0 == 0), and a tap read
from the wrong place, a border treated wrongly or a channel chunk dropped cannot hide in a max-norm ratio.  The same holds for the
plain dgrad with the impulse in dy; with one impulse in x and one in dy per image, dw and db are small integer counts.  A batch of 3
covers the nine positions in three calls (images 0-2, 3-5, 6-8 of the sequence).

Worst observed error / tolerance on an MI355X: DESIGN.md section 6b.13 (printed by test_zz_report_worst_errors)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from s2p_amd import _lib, ops
from s2p_amd._lib import ACT_LRELU, EPI_MUL_ACTGRAD, chunk_elems
from s2p_amd.slac import DECODER_100, ENCODER_100, SLOPE
from test_kernels_gpu import TOL, nchw, nhwc, pack_bwd, pack_fwd, rel_err

DTYPES = [torch.float32, torch.bfloat16]
STACKS = {"enc": (ENCODER_100, 100), "dec": (DECODER_100, 1)}


def _walk():
    out = {}
    for name, (spec, h) in STACKS.items():
        for i, (kind, cin, cout, k, s, p, op) in enumerate(spec):
            out[(name, i)] = (kind == "convT", cin, cout, k, s, p, op, h)
            h = ops.ConvGeom(cin, cout, k, s, p, transposed=(kind == "convT"), output_padding=op).out_hw(h, h)[0]
    return out


LAYERS = _walk()          # (stack, index) -> (transposed, cin, cout, k, stride, pad, output_padding, input map size)
assert LAYERS[("enc", 5)][7] == 4 and LAYERS[("dec", 5)][7] == 50

# (stack, index, batch, forward only)
CASES = [(st, i, 3, False) for st, i in LAYERS] + [("enc", 5, 32, False), ("enc", 5, 34, False), ("enc", 5, 64, False),
                                                   ("enc", 4, 641, True)]
CASE_IDS = ["%s%d-N%d" % c[:3] for c in CASES]

_G, _D, _P, _S, _PG = _lib.PATH_GENERIC, _lib.PATH_DMA, _lib.PATH_PHASES, _lib.PATH_SPLITK, _lib.PATH_PLANEG
# layer -> {test batch: (forward, dgrad) path the bf16 call must plan; None: that direction is not run at that batch}
SLAC_PATHS = {
    ("enc", 0): {3: (_G, _G)},
    ("enc", 1): {3: (_G, _G)},
    ("enc", 2): {3: (_D, _P)},
    ("enc", 3): {3: (_D, _P)},
    ("enc", 4): {3: (_S, _P), 641: (_D, None)},
    ("enc", 5): {3: (_S, _S), 32: (_PG, _PG), 34: (_PG, _PG), 64: (_PG, _PG)},
    ("dec", 0): {3: (_G, _S)},
    ("dec", 1): {3: (_P, _S)},
    ("dec", 2): {3: (_P, _D)},
    ("dec", 3): {3: (_P, _D)},
    ("dec", 4): {3: (_G, _G)},
    ("dec", 5): {3: (_G, _G)},
}
# production batch -> the test batches that stand for it, per (layer, direction); every pair not listed: the batch of 3
STANDS_FOR = {
    ("enc", 4, "forward"): {1: [3], 288: [3], 2304: [641]},
    ("enc", 5, "forward"): {1: [3], 288: [32, 34, 64], 2304: [32, 34, 64]},
    ("enc", 5, "dgrad"): {288: [32, 34, 64]},
}
PATH_NAMES = {v: k for k, v in vars(_lib).items() if k.startswith("PATH_")}
assert {(st, i, n) for st, i, n, _ in CASES} == {(st, i, n) for (st, i), t in SLAC_PATHS.items() for n in t}

WORST = {}


def _geom(layer):
    tr, cin, cout, k, s, p, op, H = LAYERS[layer]
    return ops.ConvGeom(cin, cout, k, s, p, transposed=tr, output_padding=op)


def _plan(layer, dtype, N, dgrad):
    cin, H = LAYERS[layer][1], LAYERS[layer][7]
    cin_pad = ops.pad_to(cin, chunk_elems(dtype))
    return ops.conv_path(_geom(layer), dtype, (N, H, H, cin_pad), cin_pad, dgrad=dgrad)


@pytest.mark.parametrize("layer", list(LAYERS), ids=["%s%d" % l for l in LAYERS])
def test_paths_match_production(layer):
    """Host only (s2p_conv2d_path launches nothing).  bf16: the path planned at every production batch of the layer equals the path at
    the test batch that stands for it, and the literal SLAC_PATHS; fp32: the generic kernel at all of them.  The production batches:
    1, 288 and 2304 for the encoder's forward, 288 for every backward and for the decoder.  The weight gradient has no such query:
    its path is unpinned."""
    stack = layer[0]
    name = lambda path: PATH_NAMES[path & 0xff]
    for dgrad, direction in enumerate(("forward", "dgrad")):
        for n_test, want in SLAC_PATHS[layer].items():           # the table itself, at every test batch
            if want[dgrad] is not None:
                got = _plan(layer, torch.bfloat16, n_test, bool(dgrad))
                assert got == want[dgrad], ("%s%d %s, test batch %d: plans %s, the table says %s" %
                                            (layer + (direction, n_test, name(got), name(want[dgrad]))))
                assert _plan(layer, torch.float32, n_test, bool(dgrad)) == _G, "%s%d %s, fp32, batch %d" % (layer + (direction, n_test))
        prod = (1, 288, 2304) if stack == "enc" and not dgrad else (288,)
        stands = STANDS_FOR.get(layer + (direction,), {n: [3] for n in prod})
        assert set(stands) == set(prod)
        for n_prod, tests in stands.items():                     # every production batch against the test batches that stand for it
            got_prod = _plan(layer, torch.bfloat16, n_prod, bool(dgrad))
            assert _plan(layer, torch.float32, n_prod, bool(dgrad)) == _G, "%s%d %s, fp32, batch %d" % (layer + (direction, n_prod))
            for n_test in tests:
                want = SLAC_PATHS[layer][n_test][dgrad]
                assert got_prod == want, ("%s%d %s: production batch %d plans %s, test batch %d runs %s -- pick another test batch" %
                                          (layer + (direction, n_prod, name(got_prod), n_test, name(want) if want is not None else "nothing")))


# ---- operands ------------------------------------------------------------------------------------------------------------------
def _corners(H):
    e = H - 1
    return [(0, 0), (0, e), (e, 0), (e, e)]


def _positions(H):
    e, m = H - 1, H // 2
    return _corners(H) + [(0, m), (m, 0), (m, e), (e, m), (m, m)]


def _channels(C):
    return list(dict.fromkeys(c for c in (0, 63, 64, C - 1) if c < C))


def _plant(x, C):
    """Exact zeros and negative values at the four corners (even / odd channels) and in the last real channel (even / odd pixels)."""
    N, _, H, W = x.shape
    for r, c in _corners(H):
        x[:, 0::2, r, c] = 0.0
        x[:, 1::2, r, c] = -(x[:, 1::2, r, c].abs() + 0.5)
    last = x[:, C - 1].reshape(N, H * W)
    last[:, 0::2] = 0.0
    last[:, 1::2] = -(last[:, 1::2].abs() + 0.5)
    x[:, C - 1] = last.reshape(N, H, W)
    return x


def _conv64(layer, x, w, b=None):
    tr, cin, cout, k, s, p, op, H = LAYERS[layer]
    if tr:
        return F.conv_transpose2d(x, w, b, stride=s, padding=p, output_padding=op)
    return F.conv2d(x, w, b, stride=s, padding=p)


def _device_weights(layer, w, dtype, dev):
    tr, cin, cout = LAYERS[layer][:3]
    ce = chunk_elems(dtype)
    cin_pad, cout_pad = ops.pad_to(cin, ce), ops.pad_to(cout, ce)
    w_std = w.permute(1, 0, 2, 3) if tr else w          # [Co,Ci,kh,kw] view of the weight
    return pack_fwd(w_std, cin_pad, dtype, dev), pack_bwd(w_std, cin_pad, cout_pad, dtype, dev), cin_pad, cout_pad


def _wgrad(layer, xd, dyd, cin_pad, dev):
    """dw, db as `_StackFn.backward` produces them: deterministic; db fused for the gather form, a channel sum for the scatter form."""
    tr, cin, cout, k = LAYERS[layer][:4]
    rows, cols = (cin, cout) if tr else (cout, cin)
    dw = torch.zeros((rows, k * k, cols), dtype=torch.float32, device=dev)
    db = torch.zeros(cout, dtype=torch.float32, device=dev)
    if tr:
        ops.conv_wgrad(_geom(layer), xd, dyd, dw, cin_pad, cin, cout, deterministic=True)
        ops.channel_sum(dyd, cout, db, deterministic=True)
    else:
        ops.conv_wgrad(_geom(layer), xd, dyd, dw, cin_pad, cin, cout, db=db, deterministic=True)
    torch.cuda.synchronize()
    return dw.cpu(), db.cpu()


def _dw_layout(layer, wgrad64):
    tr, cin, cout, k = LAYERS[layer][:4]
    rows, cols = (cin, cout) if tr else (cout, cin)
    return wgrad64.permute(0, 2, 3, 1).reshape(rows, k * k, cols)


def _note(case, qty, dtype, err):
    key = ("%s%d" % case[:2], qty, "bf16" if dtype == torch.bfloat16 else "fp32")
    WORST[key] = max(WORST.get(key, 0.0), err / TOL[dtype])
    print("%s%d N %d %s %s: rel err %.3e (tol %.0e)" % (case[:3] + (qty, key[2], err, TOL[dtype])))
    return err


# ---- (b) parity against float64 --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_parity(hip_device, dtype, case):
    stack, idx, N, fwd_only = case
    layer = (stack, idx)
    tr, cin, cout, k, s, p, op, H = LAYERS[layer]
    dev = hip_device
    bf16 = dtype == torch.bfloat16
    rnd = (lambda t: t.bfloat16().float()) if bf16 else (lambda t: t)
    g = torch.Generator().manual_seed(1000 + 10 * CASES.index(case) + int(bf16))
    x = torch.randn(N, cin, H, H, generator=g)
    if idx > 0:               # the layer's input is the `aux` of its dgrad epilogue
        x = _plant(x, cin)
    x = rnd(x)
    w = rnd(torch.randn((cin, cout, k, k) if tr else (cout, cin, k, k), generator=g) / math.sqrt(cin * k * k))
    b = torch.randn(cout, generator=g)
    if idx > 0:
        assert bool((x[:, cin - 1] <= 0).all()) and bool((x[:, cin - 1] < 0).any()) and bool((x[:, cin - 1] == 0).any())
        assert all(bool((x[:, :, r, c] <= 0).all()) and bool((x[:, :, r, c] == 0).any()) for r, c in _corners(H))
    xr, wr = x.double().requires_grad_(not fwd_only), w.double().requires_grad_(not fwd_only)       # float64 reference
    lin = _conv64(layer, xr, wr, b.double())
    y_ref = F.leaky_relu(lin.detach(), SLOPE)
    geom = _geom(layer)
    wf, wb, cin_pad, cout_pad = _device_weights(layer, w, dtype, dev)
    xd = nhwc(x, cin_pad, dtype, dev)
    # forward, as _StackFn.forward calls it
    y = ops.conv_fwd(geom, xd, wf, b.to(dev), cin_pad, act=ACT_LRELU, slope=SLOPE)
    y2 = ops.conv_fwd(geom, xd, wf, b.to(dev), cin_pad, act=ACT_LRELU, slope=SLOPE)
    torch.cuda.synchronize()
    errs = [_note(case, "fwd", dtype, rel_err(nchw(y, cout), y_ref))]
    assert tuple(y.shape) == (N, y_ref.shape[2], y_ref.shape[3], cout_pad)
    assert torch.equal(y, y2), "two identical forward calls differ"
    if cout_pad > cout:      # padded output channels are written as zeros
        assert float(y[..., cout:].float().abs().max()) == 0.0
    if not fwd_only:
        dy = rnd(torch.randn(lin.shape, generator=g))
        lin.backward(dy.double())
        dyd = nhwc(dy, cout_pad, dtype, dev)
        # dgrad, as _StackFn.backward calls it: the LeakyReLU derivative of the layer below folded in, but for the first layer
        if idx > 0:
            call = lambda: ops.conv_dgrad(geom, dyd, wb, tuple(xd.shape), cin_pad, aux=xd, epi=EPI_MUL_ACTGRAD, aux_act=ACT_LRELU, slope=SLOPE)
            dx_ref = xr.grad * torch.where(x.double() > 0, 1.0, SLOPE)
        else:
            call = lambda: ops.conv_dgrad(geom, dyd, wb, tuple(xd.shape), cin_pad)
            dx_ref = xr.grad
        dx, dx2 = call(), call()
        torch.cuda.synchronize()
        errs.append(_note(case, "dgrad", dtype, rel_err(nchw(dx, cin), dx_ref)))
        assert torch.equal(dx[..., :cin], dx2[..., :cin]), "two identical dgrad calls differ"
        (dw, db), (dw2, db2) = _wgrad(layer, xd, dyd, cin_pad, dev), _wgrad(layer, xd, dyd, cin_pad, dev)
        errs.append(_note(case, "dw", dtype, rel_err(dw, _dw_layout(layer, wr.grad))))
        errs.append(_note(case, "db", dtype, rel_err(db, dy.double().sum((0, 2, 3)))))
        assert torch.equal(dw, dw2) and torch.equal(db, db2), "two identical deterministic wgrad calls differ"
    assert max(errs) < TOL[dtype], errs


# ---- (c) exact impulse tests -------------------------------------------------------------------------------------------------------
def _impulse(N, C, H, first):
    """Image n: a single 1.0 at position (first + n) of the nine, in channel (first + n) of the channel list, both cyclic."""
    P, Cs = _positions(H), _channels(C)
    t = torch.zeros(N, C, H, H)
    for n in range(N):
        j = first + n
        r, c = P[j % len(P)]
        t[n, Cs[j % len(Cs)], r, c] = 1.0
    return t


def _rounds(N):
    return list(range(0, 9, N)) if N < 9 else [0]       # a batch of 3 covers the nine positions in three calls


@functools.lru_cache(maxsize=2)
def _impulse_operands(case):
    """bf16-representable weights and the float64 references of one case, shared by its two dtypes: per round (x, y64) for the forward
    and (dy, dx64, x, dw64, db64) for the backward."""
    stack, idx, N, fwd_only = case
    layer = (stack, idx)
    tr, cin, cout, k, s, p, op, H = LAYERS[layer]
    Ho = _geom(layer).out_hw(H, H)[0]
    g = torch.Generator().manual_seed(2000 + CASES.index(case))
    w = (torch.randn((cin, cout, k, k) if tr else (cout, cin, k, k), generator=g) / 4).bfloat16().float()
    fwd, bwd = [], []
    for first in _rounds(N):
        x = _impulse(N, cin, H, first)
        with torch.no_grad():
            fwd.append((x, _conv64(layer, x.double(), w.double())))
        if not fwd_only:
            dy = _impulse(N, cout, Ho, first)
            xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
            _conv64(layer, xr, wr).backward(dy.double())
            bwd.append((dy, xr.grad, x, _dw_layout(layer, wr.grad), dy.double().sum((0, 2, 3))))
    return w, fwd, bwd


def _same(got, ref64, dtype):
    """Equal as numbers to the float64 reference cast to the dtype."""
    return torch.equal(got.float(), ref64.to(dtype).float())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_impulse_forward(hip_device, dtype, case):
    stack, idx, N, _ = case
    layer = (stack, idx)
    cout = LAYERS[layer][2]
    dev = hip_device
    w, fwd, _ = _impulse_operands(case)
    wf, _, cin_pad, cout_pad = _device_weights(layer, w, dtype, dev)
    zero_bias = torch.zeros(cout, device=dev)
    for x, y64 in fwd:
        assert float(y64.abs().max()) > 0
        y = ops.conv_fwd(_geom(layer), nhwc(x, cin_pad, dtype, dev), wf, zero_bias, cin_pad)
        torch.cuda.synchronize()
        bad = (nchw(y, cout) != y64.to(dtype).float()).nonzero()
        assert _same(nchw(y, cout), y64, dtype), "%d elements differ, the first at (n, c, y, x) = %s" % (len(bad), bad[0].tolist())
        if cout_pad > cout:
            assert float(y[..., cout:].float().abs().max()) == 0.0


BWD_CASES = [c for c in CASES if not c[3]]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", BWD_CASES, ids=["%s%d-N%d" % c[:3] for c in BWD_CASES])
def test_impulse_dgrad_wgrad(hip_device, dtype, case):
    """Plain dgrad of an impulse in dy: the weights laid out around it.  Weight gradient of an impulse in x and one in dy per image: dw
    counts the images whose two impulses are one tap apart, db the impulses per channel -- small integers, exact."""
    stack, idx, N, _ = case
    layer = (stack, idx)
    tr, cin, cout, k, s, p, op, H = LAYERS[layer]
    dev = hip_device
    w, _, bwd = _impulse_operands(case)
    _, wb, cin_pad, cout_pad = _device_weights(layer, w, dtype, dev)
    for dy, dx64, x, dw64, db64 in bwd:
        assert float(dx64.abs().max()) > 0 and float(dw64.abs().max()) > 0 and float(db64.sum()) == N
        dyd = nhwc(dy, cout_pad, dtype, dev)
        dx = ops.conv_dgrad(_geom(layer), dyd, wb, (N, H, H, cin_pad), cin_pad)
        torch.cuda.synchronize()
        bad = (nchw(dx, cin) != dx64.to(dtype).float()).nonzero()
        assert _same(nchw(dx, cin), dx64, dtype), "dx: %d elements differ, the first at (n, c, y, x) = %s" % (len(bad), bad[0].tolist())
        dw, db = _wgrad(layer, nhwc(x, cin_pad, dtype, dev), dyd, cin_pad, dev)
        bad = (dw != dw64.float()).nonzero()
        assert torch.equal(dw, dw64.float()), "dw: %d elements differ, the first at (row, tap, col) = %s" % (len(bad), bad[0].tolist())
        assert torch.equal(db, db64.float()), "db"


@pytest.mark.gpu
def test_zz_report_worst_errors(hip_device):
    print("\nworst rel err / TOL per (layer, quantity, dtype):")
    for key in sorted(WORST):
        print("  %-5s %-5s %s  %.3g" % (key + (WORST[key],)))
    assert WORST and max(WORST.values()) < 1.0
