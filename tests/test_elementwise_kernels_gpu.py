"""Edge-case parity of the element-wise, pooling, layout, loss and optimizer kernels of s2p_amd/csrc/misc.hip (and s2p_channel_sum)
against plain CPU references -- never against another kernel of the library.

Criteria (no tolerance here is a measured number):
  * copies, selections and "one fp32 operation, one round-to-nearest-even" kernels: BIT equality with the same fp32 operation and cast done
    by torch on the CPU (`same_bits`; `torch.equal`, which lets -0.0 == +0.0, only where include/s2p_hip.h leaves the sign of a zero open);
  * sums in an order the kernel owns (avg-pool, reflect fold): once on integer-valued data whose partial sums are exact (bit equality), once
    on normal data against float64 with |err| <= (k + 1) 2^-24 sum|terms| (k terms), plus the bf16 rounding 2^-8 |value| for bf16 outputs;
  * loss values and channel sums (fp32 atomics in arbitrary order): float64 reference, |err| <= (t + 8 + g) 2^-24 |scale| sum|terms| with
    t = terms per thread and g = workgroups adding to the word, both computed from the launch rule (the functions below cite it), and the
    integer-valued variant, which must match to the bit;
  * Adam: one step at a time against the float64 formula on the fp32 inputs and fp32-rounded hyper-parameters,
    tol = 4 max|A32 - A64| (A32: the same step in fp32 on the CPU), floor one ulp of the value; posenc: tol = 8 max|fp32 libm - float64|.
    The largest |kernel - A64| / tol of each case is printed.

Every output (and in-place operand) is a view into the middle of a larger allocation whose head and tail hold a fixed bit pattern that
must survive the call; outputs are pre-filled with the same pattern, so an element a kernel skipped is not a plausible value.  Unaligned
pointers go only to the entry points with a per-element path; the others are tested for a refusal before launch.  Sizes come from the
launch constants of misc.hip, read from the source: last one-pass size, first two-pass sizes, a ragged tail, 2.5 x that, and the largest
tensor of the batch-64 84x84 train step.

Not covered: IdxDiv's slow path (totals >= 2^31) and the top of its fast range need ~8 GB of tensors through these kernels; the conv,
norm, linear, spectral and metrics kernels have their own modules."""
import ctypes
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from s2p_amd import _lib, ops  # noqa: E402
from s2p_amd._lib import (ACT_LRELU, ACT_NONE, ACT_RELU, ACT_SWISH, ACT_TANH, check, chunk_elems, dtype_id, lib, ptr,  # noqa: E402
                          stream)

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
U = 2.0 ** -24          # unit roundoff of fp32
UB = 2.0 ** -8          # unit roundoff of bf16
BAND = 256              # guard elements on each side (>= 256 bytes for every dtype used)
PAT = {4: 0x7B7B7B7B, 2: 0x7B7B, 1: 0x7B}        # the sentinel: 1.3e36 as fp32 and as bf16
IVIEW = {4: torch.int32, 2: torch.int16, 1: torch.uint8}

_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "s2p_amd", "csrc", "misc.hip")).read()


def _const(pattern):
    m = re.search(pattern, _SRC, re.S)
    assert m, "launch constant not found in misc.hip: " + pattern
    return int(m.group(1))


WG = _const(r"#define GRID_STRIDE.*?blockIdx\.x \* (\d+) \+ threadIdx")                 # threads per workgroup
CAP = _const(r"grid_for\(long long total, int cap = (\d+)\)")                             # default grid cap
CAP_HINGE = _const(r"int s2p_hinge_loss\(.*?grid_for\(count, (\d+)\)")
CAP_HINGE_NHWC = _const(r"int s2p_hinge_loss_strided\(.*?grid_for\(pixels, (\d+)\)")
CAP_L1 = _const(r'int s2p_l1_loss\(.*?"S2P_L1_BLOCKS", (\d+)\)')
L1_DIV = _const(r"grid_for\(count / (\d+), l1_cap\)")
CAP_L1_MULTI = _const(r'int s2p_l1_loss_multi\(.*?"S2P_L1_BLOCKS", (\d+)\)')
L1_MULTI_PER_WG = _const(r"q\.count / ce \+ (\d+)\) / \d+; if \(nb > cap\)") + 1          # chunks per workgroup of a job
CAP_ADAM = _const(r"int s2p_adam_step_dev_part\(.*?grid_for\(n4, (\d+)\)")


def size_classes(e, cap, production):
    """Sizes (elements) around the grid-stride boundary of a kernel that covers `e` elements per thread iteration."""
    one = WG * e * cap
    s = {1, e + 1, WG * e - 1, one, one + 1, one + e + 3, int(2.5 * (one + e + 3)), production}
    if e > 1:
        s.add(e - 1)
    return sorted(s)


# ---- guard bands ------------------------------------------------------------------------------------------------------------------
class Guarded:
    """A tensor of `shape` in the middle of a larger device allocation filled with the sentinel; `off` elements of misalignment."""

    def __init__(self, shape, dtype, dev, init=None, off=0):
        self.n = int(math.prod(shape))
        esz = torch.empty(0, dtype=dtype).element_size()
        self.iv = IVIEW[esz]
        pat = PAT[esz]
        self.buf = torch.empty(2 * BAND + off + self.n, dtype=dtype, device=dev)
        self.buf.view(self.iv).fill_(pat)
        self.lo = BAND + off
        self.t = self.buf[self.lo:self.lo + self.n].view(shape)
        assert self.t.data_ptr() % 16 == (off * esz) % 16
        if init is not None:
            self.t.copy_(init.reshape(shape).to(dtype))
        self.pat = pat

    def check(self, what=""):
        b = self.buf.view(self.iv)
        assert bool((b[:self.lo] == self.pat).all()) and bool((b[self.lo + self.n:] == self.pat).all()), \
            "guard band overwritten: " + what
        return self.t.cpu()


def sentinel_like(t):
    """CPU tensor of t's shape / dtype holding the sentinel."""
    s = torch.empty_like(t)
    s.view(IVIEW[t.element_size()]).fill_(PAT[t.element_size()])
    return s


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(IVIEW[a.element_size()]), b.view(IVIEW[b.element_size()]))


def first_diff(a, b):
    a, b = a.reshape(-1), b.reshape(-1)
    d = (a.view(IVIEW[a.element_size()]) != b.view(IVIEW[b.element_size()])).nonzero()
    if d.numel() == 0:
        return "equal"
    i = int(d[0])
    return "%d differ, first at %d: got %r want %r" % (d.numel(), i, float(a[i]), float(b[i]))


def rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * scale
    return x.to(dtype)          # bf16 inputs are rounded before the reference sees them


def ints(shape, dtype, seed, lo=-3, hi=4):
    g = torch.Generator().manual_seed(seed)
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return torch.randint(lo, hi, shape, generator=g).float().to(dtype)


def refuses(fn, *args, match=None):
    """The entry point returns non-zero and leaves a message (nothing was launched)."""
    rc = fn(*args)
    msg = lib().s2p_last_error().decode()
    assert rc != 0 and msg, "call was accepted"
    if match:
        assert re.search(match, msg), msg


def out_tol(bound32, ref, dtype):
    """fp32 bound -> bound on the stored value (bf16: one more rounding, relative 2^-8, or half the smallest denormal)."""
    if dtype == F32:
        return bound32
    return bound32 + UB * (ref.abs() + bound32) + 2.0 ** -134


# ---- add / scale_ / cast / act_bwd ------------------------------------------------------------------------------------------------------
PROD_G64 = 64 * 84 * 84 * 64          # the generator's 64-channel 84x84 map at batch 64 (generator.py: residual add of the decoder)
PROD_VGG1 = 64 * 84 * 84 * 64         # VGG relu1_x at batch 64 (loss.py: act_bwd / max-pool of the first stage)


@pytest.mark.parametrize("alias", ["fresh", "out_is_a", "out_is_b", "a_unaligned", "out_unaligned"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_add(hip_device, dtype, alias):
    ce = chunk_elems(dtype)
    sizes = size_classes(ce, CAP, PROD_G64)
    if alias != "fresh":
        sizes = sizes[:-1]              # the production size once per dtype
    for n in sizes:
        a, b = rnd(n, dtype, n % 1000), rnd(n, dtype, n % 1000 + 1)
        want = (a.float() + b.float()).to(dtype)
        A = Guarded((n,), dtype, hip_device, a, off=1 if alias == "a_unaligned" else 0)
        B = Guarded((n,), dtype, hip_device, b)
        O = A if alias == "out_is_a" else B if alias == "out_is_b" else Guarded((n,), dtype, hip_device, off=1 if alias == "out_unaligned" else 0)
        check(lib().s2p_add(dtype_id(dtype), ptr(A.t), ptr(B.t), ptr(O.t), n, stream()), "s2p_add")
        got = O.check("add out n=%d" % n)
        assert same_bits(got, want), "add %s n=%d: %s" % (alias, n, first_diff(got, want))
        if O is not A:
            assert same_bits(A.check(), a)
        if O is not B:
            assert same_bits(B.check(), b)


@pytest.mark.parametrize("scale", [0.0, -1.0, 2.0 ** -10, 1.0 / 3.0])
@pytest.mark.parametrize("dtype", DTYPES)
def test_scale(hip_device, dtype, scale):
    sc = torch.tensor([scale], dtype=F32)
    scd = sc.to(hip_device)
    for n in size_classes(1, CAP, 64 * 84 * 84 * 8):          # autograd_nodes.py: the image gradient at pitch 8
        x = rnd(n, dtype, n % 997)
        want = (x.float() * sc).to(dtype)
        X = Guarded((n,), dtype, hip_device, x)
        check(lib().s2p_scale(dtype_id(dtype), ptr(X.t), n, ptr(scd), stream()), "s2p_scale")
        got = X.check("scale n=%d" % n)
        assert same_bits(got, want), "scale %g n=%d: %s" % (scale, n, first_diff(got, want))


@pytest.mark.parametrize("dst", DTYPES)
@pytest.mark.parametrize("src", DTYPES)
def test_cast(hip_device, src, dst):
    for n in size_classes(1, CAP, 64 * 84 * 84 * 8):
        x = rnd(n, F32, n % 991, scale=3.0)
        x[::5] *= 1e-39 if n > 5 else 1.0                  # denormals of both formats
        x = x.to(src)
        want = x.float().to(dst)
        X = Guarded((n,), src, hip_device, x)
        Y = Guarded((n,), dst, hip_device)
        check(lib().s2p_cast(dtype_id(src), ptr(X.t), dtype_id(dst), ptr(Y.t), n, stream()), "s2p_cast")
        got = Y.check("cast n=%d" % n)
        assert same_bits(got, want), "cast n=%d: %s" % (n, first_diff(got, want))


def _act_inputs(n, dtype, seed):
    dy = rnd(n, dtype, seed)
    y = rnd(n, F32, seed + 1)
    special = torch.tensor([0.0, -0.0, 1.0, -1.0, 1e-40, -1e-40, 2.0 ** -133, -2.0 ** -133, 0.5, -0.5])
    k = min(n, special.numel())
    y[:k] = special[:k]
    if n > 4 * special.numel():
        y[-k:] = special[:k]
    return dy, y.to(dtype)


@pytest.mark.parametrize("act,slope", [(ACT_NONE, 0.0), (ACT_RELU, 0.0), (ACT_LRELU, 0.2), (ACT_LRELU, 1.0), (ACT_TANH, 0.0)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_act_bwd(hip_device, dtype, act, slope):
    sizes = size_classes(1, CAP, PROD_VGG1)
    if not (dtype == BF16 and act == ACT_RELU):
        sizes = sizes[:-1]              # VGG relu1_x backward runs in bf16 with relu: the production size once
    for n in sizes:
        dy, y = _act_inputs(n, dtype, n % 983)
        DY, Y, DX = Guarded((n,), dtype, hip_device, dy), Guarded((n,), dtype, hip_device, y), Guarded((n,), dtype, hip_device)
        check(lib().s2p_act_bwd(dtype_id(dtype), ptr(DY.t), ptr(Y.t), n, act, slope, ptr(DX.t), stream()), "s2p_act_bwd")
        got = DX.check("act_bwd n=%d" % n)
        d32, y32 = dy.float(), y.float()
        if act == ACT_TANH:
            # dy * (1 - y * y): 2 operations after the square -> (k + 1) 2^-24 (|dy| y^2 + |dy (1 - y^2)|), k = 2
            d64, y64 = d32.double(), y32.double()
            ref = d64 * (1.0 - y64 * y64)
            tol = out_tol(3 * U * d64.abs() * (y64 * y64 + (1.0 - y64 * y64).abs()), ref, dtype)
            err = (got.double() - ref).abs()
            assert bool((err <= tol).all()), "act_bwd tanh n=%d: worst err/tol %g" % (n, float((err / tol.clamp_min(1e-300)).max()))
            continue
        one = torch.ones_like(y32)
        grad = {ACT_NONE: one, ACT_RELU: torch.where(y32 > 0, one, 0 * one), ACT_LRELU: torch.where(y32 > 0, one, slope * one)}[act]
        want = (d32 * grad).to(dtype)
        assert same_bits(got, want), "act_bwd act=%d n=%d: %s" % (act, n, first_diff(got, want))


def test_act_bwd_refuses_what_it_cannot_differentiate(hip_device):
    """swish' is not a function of swish(x): s2p_act_bwd, the norm backward, s2p_linear_bwd and the dgrad's aux_act refuse it (and unknown
    ids) instead of passing dy through."""
    dev = hip_device
    n = 64
    dy, y, dx = rnd(n, F32, 1).to(dev), rnd(n, F32, 2).to(dev), Guarded((n,), F32, dev)
    for act in (ACT_SWISH, 7, -1):
        refuses(lib().s2p_act_bwd, 0, ptr(dy), ptr(y), n, act, 0.2, ptr(dx.t), stream(), match="activation")
    assert same_bits(dx.check(), sentinel_like(dx.t.cpu()))          # nothing ran
    x = torch.randn(2, 9, 9, 64, device=dev).bfloat16()
    yv, stats = ops.in_norm_fwd(x, 64, act=ACT_RELU)
    with pytest.raises(RuntimeError, match="activation"):
        ops.in_bwd(x, x, 64, stats, act=ACT_SWISH)
    xl = torch.randn(8, 16, device=dev); dyl = torch.randn(8, 16, device=dev); dw = torch.zeros(16, 16, device=dev)
    for act in (ACT_SWISH, ACT_TANH):                      # the linear backward has relu / lrelu / none only
        with pytest.raises(RuntimeError, match="activation"):
            ops.linear_bwd(xl, dyl, dyl, None, 16, 16, 16, act, 0.2, dw, None, need_dx=False)
    geom = ops.ConvGeom(64, 64, 3, 1, 1)
    wb = torch.randn(64, 9, 64, device=dev).bfloat16()
    with pytest.raises(RuntimeError, match="activation"):
        ops.conv_dgrad(geom, x, wb, tuple(x.shape), 64, aux=x, epi=ops.EPI_MUL_ACTGRAD, aux_act=ACT_SWISH)


# ---- copy_channels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("geom", [(8, 0, 8, 3, 3), (8, 3, 8, 0, 3),      # the two production calls (autograd_nodes.py: prev|fake concat and its slice)
                                  (8, 0, 8, 0, 8), (16, 5, 8, 7, 1), (24, 1, 16, 3, 13), (3, 0, 5, 1, 3)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_copy_channels(hip_device, dtype, geom, accumulate):
    sp, so, dp, d_o, C = geom
    for total in size_classes(1, CAP, 64 * 84 * 84 * C):
        px = max(1, total // C)
        for pixels in sorted({px, px + 1}):
            src, dst0 = rnd((pixels, sp), dtype, pixels % 977), rnd((pixels, dp), dtype, pixels % 977 + 1)
            want = dst0.clone()
            new = src[:, so:so + C].float() + (dst0[:, d_o:d_o + C].float() if accumulate else 0.0)
            want[:, d_o:d_o + C] = new.to(dtype)
            S, D = Guarded((pixels, sp), dtype, hip_device, src), Guarded((pixels, dp), dtype, hip_device, dst0)
            check(lib().s2p_copy_channels(dtype_id(dtype), ptr(S.t), sp, so, ptr(D.t), dp, d_o, C, pixels, accumulate, stream()), "copy_channels")
            got = D.check("copy_channels")
            assert same_bits(got, want), "copy_channels %s acc=%d pixels=%d: %s" % (geom, accumulate, pixels, first_diff(got, want))
            assert same_bits(S.check(), src)


@pytest.mark.parametrize("dtype", DTYPES)
def test_copy_channels_batch_rows(hip_device, dtype):
    """ops.copy_channels(src_rows, src_row0, dst_row0): a batch prefix into the second half of a 2N batch (autograd_nodes.py)."""
    N, H, W = 3, 7, 5
    src, dst0 = rnd((N + 1, H, W, 8), dtype, 5), rnd((2 * N, H, W, 8), dtype, 6)
    for acc in (False, True):
        S, D = Guarded(src.shape, dtype, hip_device, src), Guarded(dst0.shape, dtype, hip_device, dst0)
        ops.copy_channels(S.t, 0, D.t, 3, 3, accumulate=acc, src_rows=N, dst_row0=N, src_row0=1)
        want = dst0.clone()
        want[N:, ..., 3:6] = (src[1:N + 1, ..., 0:3].float() + (dst0[N:, ..., 3:6].float() if acc else 0.0)).to(dtype)
        got = D.check()
        assert same_bits(got, want), first_diff(got, want)


# ---- layout conversions ----------------------------------------------------------------------------------------------------------------
PLANES = [(1, 1), (1, 9), (7, 1), (84, 84), (83, 85)]


@pytest.mark.parametrize("zero_pad", [1, 0])
@pytest.mark.parametrize("C", [1, 3, 6, 8, 17])
@pytest.mark.parametrize("dtype", DTYPES)
def test_nchw_to_nhwc(hip_device, dtype, C, zero_pad):
    ce = chunk_elems(dtype)
    cpad = (C + ce - 1) // ce * ce
    for (H, W) in PLANES:
        for N in ((2, 64) if (H, W) == (84, 84) and C == 3 else (2,)):      # N = 64: the train step's image conversion (one pass: a thread per pixel; two passes below)
            for pitch in (cpad, 2 * cpad, cpad + 3):                      # the last: not a chunk multiple -> per-element branch
                for c_off in sorted({0, min(3, pitch - C), pitch - C}):
                    x = rnd((N, C, H, W), F32, H * W + C)
                    X = x.to(hip_device)
                    Y = Guarded((N, H, W, pitch), dtype, hip_device)
                    check(lib().s2p_nchw_to_nhwc(dtype_id(dtype), ptr(X), N, C, H, W, ptr(Y.t), pitch, c_off, zero_pad, stream()), "nchw_to_nhwc")
                    got = Y.check("nchw_to_nhwc")
                    want = torch.zeros(N, H, W, pitch, dtype=dtype) if zero_pad else sentinel_like(got)
                    want[..., c_off:c_off + C] = x.permute(0, 2, 3, 1).to(dtype)
                    assert same_bits(got, want), "nchw_to_nhwc C=%d %dx%d N=%d pitch=%d c_off=%d zp=%d: %s" % (
                        C, H, W, N, pitch, c_off, zero_pad, first_diff(got, want))


@pytest.mark.parametrize("dtype", DTYPES)
def test_nchw_to_nhwc_second_pass(hip_device, dtype):
    """More pixels than one pass of the capped grid covers (one thread per pixel): 256 * cap + a ragged rest, on a prime-ish plane."""
    ce = 8                              # the image pitch (one bf16 chunk, two fp32 chunks)
    H, W, C = 83, 85, 3
    N = (WG * CAP) // (H * W) + 2
    assert N * H * W > WG * CAP
    x = rnd((N, C, H, W), F32, 11)
    for zero_pad, c_off in ((1, 0), (0, 3)):
        Y = Guarded((N, H, W, ce), dtype, hip_device)
        check(lib().s2p_nchw_to_nhwc(dtype_id(dtype), ptr(x.to(hip_device)), N, C, H, W, ptr(Y.t), ce, c_off, zero_pad, stream()), "nchw_to_nhwc")
        got = Y.check()
        want = torch.zeros(N, H, W, ce, dtype=dtype) if zero_pad else sentinel_like(got)
        want[..., c_off:c_off + C] = x.permute(0, 2, 3, 1).to(dtype)
        assert same_bits(got, want), first_diff(got, want)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("C", [1, 3, 6, 8, 17])
@pytest.mark.parametrize("dtype", DTYPES)
def test_nhwc_to_nchw(hip_device, dtype, C, accumulate):
    ce = chunk_elems(dtype)
    cpad = (C + ce - 1) // ce * ce
    for (H, W) in PLANES:
        for N in ((2, 64) if (H, W) == (84, 84) and C == 3 else (2,)):      # 64 x 3 x 84 x 84 = 1.35 M elements: a second pass (autograd_nodes.py: the fake image back to NCHW)
            for pitch in (cpad, 2 * cpad):
                for c_off in sorted({0, min(3, pitch - C), pitch - C}):
                    x = rnd((N, H, W, pitch), dtype, H + W + C)
                    y0 = rnd((N, C, H, W), F32, 3)
                    Y = Guarded((N, C, H, W), F32, hip_device, y0 if accumulate else None)
                    check(lib().s2p_nhwc_to_nchw(dtype_id(dtype), ptr(x.to(hip_device)), pitch, c_off, N, C, H, W, ptr(Y.t), accumulate, stream()), "nhwc_to_nchw")
                    got = Y.check("nhwc_to_nchw")
                    v = x[..., c_off:c_off + C].float().permute(0, 3, 1, 2)
                    want = (y0 + v) if accumulate else v.contiguous()
                    assert same_bits(got, want), "nhwc_to_nchw C=%d %dx%d N=%d pitch=%d c_off=%d acc=%d: %s" % (
                        C, H, W, N, pitch, c_off, accumulate, first_diff(got, want))


@pytest.mark.parametrize("dtype", DTYPES)
def test_u8_conversions(hip_device, dtype):
    ce = chunk_elems(dtype)
    for pixels in sorted({max(1, s // 3) for s in size_classes(1, CAP, 1)} | {64 * 84 * 84}):      # the last: a batch of 64 frames (augment.py)
        g = torch.Generator().manual_seed(pixels % 971)
        u = torch.randint(0, 256, (pixels, 3), generator=g, dtype=torch.uint8)
        u.view(-1)[:min(256, u.numel())] = torch.arange(min(256, u.numel()), dtype=torch.uint8)
        Y = Guarded((pixels, ce), dtype, hip_device)
        check(lib().s2p_u8_to_nhwc(dtype_id(dtype), ptr(u.to(hip_device)), pixels, 3, ptr(Y.t), ce, stream()), "u8_to_nhwc")
        got = Y.check("u8_to_nhwc")
        want = torch.zeros(pixels, ce, dtype=dtype)
        want[:, :3] = (u.float() / 127.5 - 1.0).to(dtype)
        assert same_bits(got, want), "u8_to_nhwc pixels=%d: %s" % (pixels, first_diff(got, want))
        x = rnd((pixels, ce), dtype, pixels % 971 + 1, scale=0.7)
        B = Guarded((pixels, 3), torch.uint8, hip_device)
        check(lib().s2p_nhwc_to_u8(dtype_id(dtype), ptr(x.to(hip_device)), ce, pixels, 3, ptr(B.t), stream()), "nhwc_to_u8")
        gotb = B.check("nhwc_to_u8")
        wantb = torch.round((x[:, :3].float() + 1.0) * 127.5).clamp(0, 255).to(torch.uint8)      # torch.round: half to even, as rintf
        assert torch.equal(gotb, wantb), "nhwc_to_u8 pixels=%d" % pixels


# ---- avg-pool 3x3 s2 p1 ----------------------------------------------------------------------------------------------------------------
SMALL = [1, 2, 3, 4, 5, 7, 8]
AVG_PLANES = [(h, w) for h in SMALL for w in SMALL] + [(84, 84), (42, 42), (21, 21), (11, 11), (83, 85)]      # + the discriminator's pyramid


def _to_nhwc(x):            # [N,C,H,W] -> [N,H,W,C]
    return x.permute(0, 2, 3, 1).contiguous()


def _to_nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("C,off", [(8, 0), (16, 0), (24, 0), (40, 0), (56, 0), (3, 0), (5, 0), (8, 1)])      # the last three: per-element form
@pytest.mark.parametrize("dtype", DTYPES)
def test_avgpool(hip_device, dtype, C, off):
    dt = dtype_id(dtype)
    for (H, W) in AVG_PLANES:
        N = 2
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        cnt = F.avg_pool2d(torch.ones(1, 1, H, W), 3, 2, 1, divisor_override=1)                 # window sizes (exact)
        for kind in ("int", "normal"):
            x = (ints if kind == "int" else rnd)((N, C, H, W), dtype, H * 9 + W)
            X = Guarded((N, H, W, C), dtype, hip_device, _to_nhwc(x), off=off)
            Y = Guarded((N, Ho, Wo, C), dtype, hip_device, off=off)
            check(lib().s2p_avgpool3x3s2_fwd(dt, ptr(X.t), N, H, W, C, ptr(Y.t), stream()), "avgpool fwd")
            got = _to_nchw(Y.check("avgpool fwd"))
            if kind == "int":           # exact sums, one correctly rounded division, one cast
                want = (F.avg_pool2d(x.float(), 3, 2, 1, divisor_override=1) / cnt).to(dtype)
                assert same_bits(got, want), "avgpool fwd int %dx%d C=%d: %s" % (H, W, C, first_diff(got, want))
            else:
                x64 = x.double()
                ref = F.avg_pool2d(x64, 3, 2, 1, count_include_pad=False)
                tol = out_tol((cnt.double() + 1) * U * F.avg_pool2d(x64.abs(), 3, 2, 1, count_include_pad=False), ref, dtype)
                assert bool(((got.double() - ref).abs() <= tol).all()), "avgpool fwd %dx%d C=%d" % (H, W, C)
            # backward, with and without accumulation into a pre-filled dx.  Integer variant: dy = 36 i, so that dy / (cy cx) is an
            # integer for every window size (1, 2, 3, 4, 6, 9) and every sum is exact; dx += is one fp32 add and one rounding
            dy = (ints((N, C, Ho, Wo), dtype, H + W * 9, -3, 4) * 36).to(dtype) if kind == "int" else rnd((N, C, Ho, Wo), dtype, H + W * 9)
            dx0 = (ints if kind == "int" else rnd)((N, C, H, W), dtype, H + W)
            for acc in (0, 1):
                DY = Guarded((N, Ho, Wo, C), dtype, hip_device, _to_nhwc(dy), off=off)
                DX = Guarded((N, H, W, C), dtype, hip_device, _to_nhwc(dx0) if acc else None, off=off)
                check(lib().s2p_avgpool3x3s2_bwd(dt, ptr(DY.t), N, H, W, C, ptr(DX.t), acc, stream()), "avgpool bwd")
                got = _to_nchw(DX.check("avgpool bwd"))
                xr = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
                F.avg_pool2d(xr, 3, 2, 1, count_include_pad=False).backward(dy.double())
                ref = xr.grad + (dx0.double() if acc else 0.0)
                if kind == "int":
                    want = ref.float().to(dtype)
                    assert same_bits(got, want), "avgpool bwd int %dx%d C=%d acc=%d: %s" % (H, W, C, acc, first_diff(got, want))
                else:                   # <= 4 windows per pixel (+ the stored value): k = 5 terms, each quotient one rounding
                    xa = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
                    F.avg_pool2d(xa, 3, 2, 1, count_include_pad=False).backward(dy.double().abs())
                    tol = out_tol(6 * U * (xa.grad + (dx0.double().abs() if acc else 0.0)), ref, dtype)
                    assert bool(((got.double() - ref).abs() <= tol).all()), "avgpool bwd %dx%d C=%d acc=%d" % (H, W, C, acc)


@pytest.mark.parametrize("dtype", DTYPES)
def test_avgpool_second_pass(hip_device, dtype):
    """> 256 * cap chunks: 64 x 84 x 84 x 8 input (discriminator.py: the image pyramid at batch 64) has 451 584 / 903 168 chunks for the
    backward -- below one pass -- so the pass boundary is crossed with C = 24 (3 chunks per pixel) at N = 64 instead."""
    N, C, H, W = 64, 24, 84, 84
    ce = chunk_elems(dtype)
    assert N * H * W * (C // ce) > WG * CAP
    x = ints((N, C, H, W), dtype, 1)
    cnt = F.avg_pool2d(torch.ones(1, 1, H, W), 3, 2, 1, divisor_override=1)
    X, Y = Guarded((N, H, W, C), dtype, hip_device, _to_nhwc(x)), Guarded((N, 42, 42, C), dtype, hip_device)
    check(lib().s2p_avgpool3x3s2_fwd(dtype_id(dtype), ptr(X.t), N, H, W, C, ptr(Y.t), stream()), "avgpool fwd")
    got, want = _to_nchw(Y.check()), (F.avg_pool2d(x.float(), 3, 2, 1, divisor_override=1) / cnt).to(dtype)
    assert same_bits(got, want), first_diff(got, want)
    dy = (ints((N, C, 42, 42), dtype, 2) * 36).to(dtype)
    dx0 = ints((N, C, H, W), dtype, 3)
    DY, DX = Guarded((N, 42, 42, C), dtype, hip_device, _to_nhwc(dy)), Guarded((N, H, W, C), dtype, hip_device, _to_nhwc(dx0))
    check(lib().s2p_avgpool3x3s2_bwd(dtype_id(dtype), ptr(DY.t), N, H, W, C, ptr(DX.t), 1, stream()), "avgpool bwd")
    xr = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    F.avg_pool2d(xr, 3, 2, 1, count_include_pad=False).backward(dy.double())
    got, want = _to_nchw(DX.check()), (xr.grad + dx0.double()).float().to(dtype)
    assert same_bits(got, want), first_diff(got, want)


# ---- max-pool 2x2 with the ReLU mask ---------------------------------------------------------------------------------------------------
def _maxpool_check(dev, dtype, x, dy, what):
    """x: [N,C,H,W] 'ReLU output' (may hold -0.0 and negative values), dy: [N,C,H/2,W/2]."""
    N, C, H, W = x.shape
    dt = dtype_id(dtype)
    X, DYt = Guarded((N, H, W, C), dtype, dev, _to_nhwc(x)), Guarded((N, H // 2, W // 2, C), dtype, dev, _to_nhwc(dy))
    Y, DX = Guarded((N, H // 2, W // 2, C), dtype, dev), Guarded((N, H, W, C), dtype, dev)
    xr = x.float().clone().requires_grad_(True)
    if H // 2 and W // 2:
        F.max_pool2d(F.relu(xr), 2, 2).backward(dy.float())
    else:
        xr.grad = torch.zeros_like(xr)      # no window at all: every pixel is "uncovered"
    if H // 2 and W // 2:
        check(lib().s2p_maxpool2x2_fwd(dt, ptr(X.t), N, H, W, C, ptr(Y.t), stream()), "maxpool fwd")
        # the forward is the plain maximum of the stored values (no clamp): same as relu's for a relu output; sign of a zero open
        got, want = _to_nchw(Y.check(what)), F.max_pool2d(x.float(), 2, 2).to(dtype)
        assert torch.equal(got, want), "maxpool fwd %s: %s" % (what, first_diff(got, want))
    check(lib().s2p_maxpool2x2_bwd(dt, ptr(DYt.t), ptr(X.t), N, H, W, C, ptr(DX.t), stream()), "maxpool bwd")
    got, want = _to_nchw(DX.check(what)), xr.grad.to(dtype)
    assert torch.equal(got, want), "maxpool bwd %s: %s" % (what, first_diff(got, want))      # (header: "else 0", sign open)
    assert not bool(torch.isnan(got.float()).any())


def _coarse(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = F.relu(torch.round(2 * torch.randn(shape, generator=g)) / 2)
    z = (x == 0) & (torch.rand(shape, generator=g) < 0.4)
    x[z] = -0.0                       # what the library's own ReLU, max(v, v * 0), leaves for a negative input
    return x.to(dtype)


@pytest.mark.parametrize("C", [8, 24, 40, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_maxpool_ties_and_zeros(hip_device, dtype, C):
    for (N, H, W) in [(4, 11, 9), (2, 1, 6), (2, 6, 1), (1, 2, 2), (3, 83, 85), (2, 84, 84)]:
        x = _coarse((N, C, H, W), dtype, H * W + C)
        dy = rnd((N, C, H // 2, W // 2), dtype, 7)
        dy.view(-1)[::3] = dy.view(-1)[::3].abs() + 0.5           # non-zero where it is routed
        _maxpool_check(hip_device, dtype, x, dy, "coarse %dx%dx%dx%d" % (N, C, H, W))
        if (H, W) == (11, 9) and C == 8:          # the draw really holds what it is for
            w = F.unfold(x.float(), 2, stride=2).view(N, C, 4, -1)
            m = w.max(2, keepdim=True).values
            assert int(((w == m).sum(2) > 1).__and__(m[:, :, 0] > 0).sum()) > 20 and int((m <= 0).sum()) > 20


@pytest.mark.parametrize("dtype", DTYPES)
def test_maxpool_hand_built_windows(hip_device, dtype):
    """Every pattern of >= 2 equal maxima among the 4 positions (11 of them), with the others smaller / zero / -0.0 / negative; maxima at
    the largest finite value and at the smallest positive denormal of the dtype."""
    fi = torch.finfo(dtype)
    tiny = 2.0 ** -133 if dtype == BF16 else 2.0 ** -149
    wins = []
    for mask in range(16):
        if bin(mask).count("1") < 2:
            continue
        for mx in (1.5, fi.max, tiny, 2.0 ** -126):
            for other in (0.0, -0.0, -1.0, mx / 2 if mx > tiny else 0.0):
                wins.append([mx if mask >> k & 1 else other for k in range(4)])
    for other in (0.0, -0.0, -2.0):                  # no positive maximum: nothing passes
        wins.append([other] * 4)
        wins.append([-0.0, 0.0, other, -1.0])
    for k in range(4):                               # single maxima at each position
        wins.append([3.0 if j == k else 1.0 for j in range(4)])
    nw = len(wins)
    C = 8
    Wn = 2 * nw + 1                                   # odd width: the last column receives zeros
    x = torch.zeros(1, C, 3, Wn)
    wt = torch.tensor(wins, dtype=torch.float64)
    for c in range(C):                                # channel c: the window list rotated, so that every chunk lane sees every pattern
        r = torch.roll(wt, c, 0)
        x[0, c, 0, 0:2 * nw:2], x[0, c, 0, 1:2 * nw:2] = r[:, 0].float(), r[:, 1].float()
        x[0, c, 1, 0:2 * nw:2], x[0, c, 1, 1:2 * nw:2] = r[:, 2].float(), r[:, 3].float()
    x[0, :, 2, :] = 5.0                               # uncovered last row holds large values: still zero gradient
    x[0, :, :, -1] = 5.0
    x = x.to(dtype)
    assert float(x.float().max()) == fi.max and float(x.float()[x.float() > 0].min()) == tiny
    dy = (torch.arange(C * nw).float().view(1, C, 1, nw) % 13 + 1).to(dtype)
    _maxpool_check(hip_device, dtype, x, dy, "hand-built windows")


def test_maxpool_production_size(hip_device):
    """VGG relu1_2 -> pool1 at batch 64 (loss.py): 64 x 84 x 84 x 64 bf16, 3.6 M chunks = 3-4 passes of the capped grid."""
    N, C, H, W = 64, 64, 84, 84
    x = _coarse((N, C, H, W), BF16, 1)
    dy = rnd((N, C, H // 2, W // 2), BF16, 2)
    assert N * H * W * C // 8 > 3 * WG * CAP
    _maxpool_check(hip_device, BF16, x, dy, "production")


def test_maxpool_second_pass_fp32(hip_device):
    N, C, H, W = 24, 64, 83, 85            # 2.7 M fp32 chunks, odd plane
    x = _coarse((N, C, H, W), F32, 3)
    dy = rnd((N, C, H // 2, W // 2), F32, 4)
    assert N * H * W * C // 4 > 2 * WG * CAP
    _maxpool_check(hip_device, F32, x, dy, "fp32 second pass")


# ---- nearest resize --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_resize_nearest(hip_device, dtype, C):
    S = [1, 5, 11, 21, 37, 42, 84, 85]
    pairs = [((h, h), (ho, ho)) for h in S for ho in S] + [((5, 84), (42, 11)), ((21, 37), (84, 1)), ((85, 11), (21, 85))]
    pairs += [((84, 84), (s, s)) for s in (21, 42, 84)]       # generator.py: the conditioning image at each norm's resolution
    for (H, W), (Ho, Wo) in pairs:
        N = 2
        x = rnd((N, C, H, W), dtype, H * 100 + Ho)
        X, Y = Guarded((N, H, W, C), dtype, hip_device, _to_nhwc(x)), Guarded((N, Ho, Wo, C), dtype, hip_device)
        check(lib().s2p_resize_nearest(dtype_id(dtype), ptr(X.t), N, H, W, C, ptr(Y.t), Ho, Wo, stream()), "resize")
        got, want = _to_nchw(Y.check("resize")), F.interpolate(x.float(), size=(Ho, Wo), mode="nearest").to(dtype)
        assert same_bits(got, want), "resize %dx%d -> %dx%d C=%d: %s" % (H, W, Ho, Wo, C, first_diff(got, want))


@pytest.mark.parametrize("dtype", DTYPES)
def test_resize_nearest_second_pass(hip_device, dtype):
    N, C, H, W, Ho, Wo = 64, 8, 21, 21, 84, 84          # 3.6 M output elements: 3-4 passes (the batch-64 conditioning image, pitch 8)
    assert N * Ho * Wo * C > 3 * WG * CAP
    x = rnd((N, C, H, W), dtype, 5)
    X, Y = Guarded((N, H, W, C), dtype, hip_device, _to_nhwc(x)), Guarded((N, Ho, Wo, C), dtype, hip_device)
    check(lib().s2p_resize_nearest(dtype_id(dtype), ptr(X.t), N, H, W, C, ptr(Y.t), Ho, Wo, stream()), "resize")
    got, want = _to_nchw(Y.check()), F.interpolate(x.float(), size=(Ho, Wo), mode="nearest").to(dtype)
    assert same_bits(got, want), first_diff(got, want)


# ---- reflect-pad adjoint ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [1, 2, 3])
@pytest.mark.parametrize("C", [8, 24, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_reflect_pad_bwd(hip_device, dtype, C, pad):
    planes = [(pad + 1, pad + 1), (pad + 1, 9), (pad + 2, pad + 3), (2 * pad + 1, 2 * pad), (11, 9), (83, 85)]
    if C == 64:
        planes.append((84, 84))         # the output conv's input gradient (generator.py)
    for (H, W) in planes:
        N = 40 if (H, W) == (84, 84) and dtype == BF16 else 2        # 40 x 84 x 84 x 8 chunks = 2.26 M: a second and third pass
        for kind in ("int", "normal"):
            dxp = (ints if kind == "int" else rnd)((N, C, H + 2 * pad, W + 2 * pad), dtype, H * 7 + W + pad)
            P, D = Guarded((N, H + 2 * pad, W + 2 * pad, C), dtype, hip_device, _to_nhwc(dxp)), Guarded((N, H, W, C), dtype, hip_device)
            check(lib().s2p_reflect_pad_bwd(dtype_id(dtype), ptr(P.t), N, H, W, C, pad, ptr(D.t), stream()), "reflect_pad_bwd")
            got = _to_nchw(D.check("reflect fold"))
            xr = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
            F.pad(xr, (pad,) * 4, mode="reflect").backward(dxp.double())
            if kind == "int":
                want = xr.grad.float().to(dtype)
                assert same_bits(got, want), "reflect fold int %dx%d pad=%d C=%d: %s" % (H, W, pad, C, first_diff(got, want))
            else:
                xa = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
                F.pad(xa, (pad,) * 4, mode="reflect").backward(dxp.double().abs())
                tol = out_tol(10 * U * xa.grad, xr.grad, dtype)          # k = 9 terms at most
                assert bool(((got.double() - xr.grad).abs() <= tol).all()), "reflect fold %dx%d pad=%d C=%d" % (H, W, pad, C)


# ---- losses ---------------------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def l1_launch(count, ce, vec):
    """(t, g) of s2p_l1_loss: `dim3 g(grid_for(count / 4, l1_cap))`, 256 threads; l1_loss_kernel walks count / CE chunks grid-stride
    (CE terms each) when every pointer is 16-byte aligned, then the rest (everything, if not) element by element."""
    g = min(max(_cdiv(count // L1_DIV, WG), 1), CAP_L1)
    nch = count // ce if vec else 0
    t = ce * _cdiv(nch, g * WG) + _cdiv(count - nch * ce, g * WG)
    return t, g


def hinge_launch(count, cap):
    """(t, g) of s2p_hinge_loss / _strided: `dim3 g(grid_for(count, 256))`, one element (pixel) per thread iteration."""
    g = min(max(_cdiv(count, WG), 1), cap)
    return _cdiv(count, g * WG), g


def l1_multi_launch(count, ce):
    """(t, g) of one job of s2p_l1_loss_multi: `nb = (q.count / ce + 4095) / 4096`, capped at 512, at least 1; each thread takes
    the chunks congruent to it modulo nb * 256."""
    nb = min(max(_cdiv(count // ce, L1_MULTI_PER_WG), 1), CAP_L1_MULTI)
    return ce * _cdiv(count // ce, nb * WG), nb


def _l1_pair(n, dtype, seed, kind):
    if kind == "int":           # a == b but on <= 2^18 places, |a - b| <= 2 there: every partial sum < 2^24, exact
        a = ints(n, dtype, seed)
        b = a.clone()
        g = torch.Generator().manual_seed(seed + 1)
        idx = torch.unique(torch.randint(0, n, (min(n, 2 ** 18),), generator=g))
        b[idx] = (a[idx].float() + torch.randint(-2, 3, (idx.numel(),), generator=g).float()).to(dtype)
    else:
        a, b = rnd(n, dtype, seed), rnd(n, dtype, seed + 1)
        b[::7] = a[::7]                 # exact zeros of a - b: the gradient there is 0, not +-scale
    return a, b


L1_PROD = 64 * 84 * 84 * 8              # the generated image at pitch 8 against the real one (autograd_nodes.py: the L1 term)


@pytest.mark.parametrize("align", ["aligned", "a_unaligned", "grad_unaligned"])
@pytest.mark.parametrize("gradmode", ["nograd", "grad", "accumulate"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_l1_loss(hip_device, dtype, gradmode, align):
    if align == "grad_unaligned" and gradmode == "nograd":
        gradmode = "grad"               # (a duplicate of the cell next to it rather than a skipped one)
    ce = chunk_elems(dtype)
    scale = 0.25
    for n in size_classes(L1_DIV, CAP_L1, L1_PROD):
        for kind in ("int", "normal"):
            a, b = _l1_pair(n, dtype, n % 967, kind)
            g0 = (ints if kind == "int" else rnd)(n, dtype, n % 967 + 2)
            A = Guarded((n,), dtype, hip_device, a, off=1 if align == "a_unaligned" else 0)
            B = Guarded((n,), dtype, hip_device, b)
            G = Guarded((n,), dtype, hip_device, g0 if gradmode == "accumulate" else None, off=1 if align == "grad_unaligned" else 0) \
                if gradmode != "nograd" else None
            l0 = 3.0 if kind == "int" else 0.0          # "+=" onto a non-zero word where everything is exact
            L = Guarded((1,), F32, hip_device, torch.tensor([l0]))
            check(lib().s2p_l1_loss(dtype_id(dtype), ptr(A.t), ptr(B.t), n, scale, ptr(L.t), ptr(G.t) if G else None,
                                    int(gradmode == "accumulate"), stream()), "s2p_l1_loss")
            d = a.float() - b.float()
            what = "l1 %s %s %s n=%d %s" % (dtype, gradmode, align, n, kind)
            if G is not None:
                sg = torch.where(d > 0, scale, 0.0) - torch.where(d < 0, scale, 0.0)
                want = ((sg + g0.float()) if gradmode == "accumulate" else sg).to(dtype)
                got = G.check(what)
                assert same_bits(got, want), what + ": " + first_diff(got, want)
            got = float(L.check(what)[0]) - l0
            ref = scale * float(d.double().abs().sum())
            if kind == "int":
                assert got == ref, what + ": %r != %r" % (got, ref)
            else:
                t, g = l1_launch(n, ce, align == "aligned")
                bound = (t + 8 + g) * U * ref
                assert abs(got - ref) <= bound, what + ": err %g bound %g" % (abs(got - ref), bound)


@pytest.mark.parametrize("dtype", DTYPES)
def test_l1_loss_multi(hip_device, dtype):
    ce = chunk_elems(dtype)
    dev = hip_device
    relu1_1 = 64 * 84 * 84 * 64                 # VGG relu1_1 at batch 64 (loss.py): the 512-workgroup cap, several rounds per thread
    sizes = [ce, 2 * ce, L1_MULTI_PER_WG * ce, L1_MULTI_PER_WG * ce + ce, 37 * L1_MULTI_PER_WG * ce - 3 * ce]
    assert l1_multi_launch(sizes[0], ce)[1] == 1 and l1_multi_launch(sizes[-1], ce)[1] == 37
    assert l1_multi_launch(relu1_1, ce)[1] == CAP_L1_MULTI
    for kind in ("int", "normal"):
        for njobs, nogr in ((1, ()), (2, (0,)), (16, (7,)), (16, (15,)), (17, (0, 16))):
            loss = Guarded((4,), F32, dev, torch.zeros(4))
            jobs, refs = [], []
            for j in range(njobs):
                n = relu1_1 if (j == 1 and nogr in ((0,), (7,))) else sizes[(j + njobs) % len(sizes)]      # the large map once per table shape
                a, b = _l1_pair(n, dtype, 31 * j + njobs, kind)
                G = None if j in nogr else Guarded((n,), dtype, dev)
                scale, word = (0.5, 0.25, 2.0)[j % 3], j % 3                  # jobs j, j + 3, ... share a loss word
                jobs.append((a.to(dev), b.to(dev), scale, loss.t[word:word + 1], G.t if G else None))
                refs.append((a, b, scale, word, G, n))
            if njobs <= 16:
                arr = (_lib.L1Job * njobs)(*[_lib.L1Job(ptr(a), ptr(b), ptr(g), a.numel(), s, ptr(lo)) for a, b, s, lo, g in jobs])
                check(lib().s2p_l1_loss_multi(dtype_id(dtype), arr, njobs, stream()), "s2p_l1_loss_multi")
            else:
                ops.l1_loss_multi(jobs)           # splits into launches of <= 16 jobs
            got_loss = loss.check("l1_multi loss words")
            want, bound = [0.0] * 4, [0.0] * 4
            gtot = [sum(l1_multi_launch(r[5], ce)[1] for r in refs if r[3] == w) for w in range(3)]
            for (a, b, scale, word, G, n) in refs:
                d = a.float() - b.float()
                s = scale * float(d.double().abs().sum())
                want[word] += s
                bound[word] += (l1_multi_launch(n, ce)[0] + 8 + gtot[word]) * U * s
                if G is not None:
                    g_want = (torch.where(d > 0, scale, 0.0) - torch.where(d < 0, scale, 0.0)).to(dtype)
                    got = G.check("l1_multi grad")
                    assert same_bits(got, g_want), "l1_multi %s njobs=%d n=%d: %s" % (kind, njobs, n, first_diff(got, g_want))
            for w in range(4):
                if kind == "int":
                    assert float(got_loss[w]) == want[w], "l1_multi int njobs=%d word %d: %r != %r" % (njobs, w, float(got_loss[w]), want[w])
                else:
                    assert abs(float(got_loss[w]) - want[w]) <= bound[w], "l1_multi njobs=%d word %d: err %g bound %g" % (
                        njobs, w, abs(float(got_loss[w]) - want[w]), bound[w])


def _hinge_ref(x32, mode, scale, dtype):
    sgn = 1.0 if mode == 0 else -1.0
    t = 1.0 + sgn * x32                                   # the kernel's fp32 operation
    on = t > 0
    if mode == 2:
        term, gr = -x32, torch.full_like(x32, -scale)
    else:
        term, gr = torch.where(on, t, torch.zeros_like(t)), torch.where(on, sgn * scale, 0.0) + 0 * x32
    return term.double(), gr.to(dtype)


def _hinge_inputs(n, dtype, seed, kind):
    x = (ints if kind == "int" else rnd)(n, dtype, seed)
    if kind != "int":
        one = torch.tensor([1.0], dtype=dtype)
        hi, lo = one.view(IVIEW[one.element_size()]) + 1, one.view(IVIEW[one.element_size()]) - 1      # one ulp either side of 1
        sp = torch.cat([one, -one, hi.view(dtype), -hi.view(dtype), lo.view(dtype), -lo.view(dtype)])
        k = min(n, 6)
        x[:k] = sp[:k]
        if n > 600:
            x[-6:] = sp
    return x


HINGE_PROD = [64 * 13 * 13, 64 * 7 * 7]          # the PatchGAN logit maps of the two scales at batch 64 (discriminator.py)


@pytest.mark.parametrize("want_grad", [True, False])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_hinge_loss(hip_device, dtype, mode, want_grad):
    scale = 0.5
    for n in size_classes(1, CAP_HINGE, HINGE_PROD[0]) + HINGE_PROD[1:]:
        for kind in ("int", "normal"):
            x = _hinge_inputs(n, dtype, n % 953 + mode, kind)
            X = Guarded((n,), dtype, hip_device, x)
            G = Guarded((n,), dtype, hip_device) if want_grad else None
            L = Guarded((1,), F32, hip_device, torch.zeros(1))
            check(lib().s2p_hinge_loss(dtype_id(dtype), ptr(X.t), n, mode, scale, ptr(L.t), ptr(G.t) if G else None, stream()), "hinge")
            term, gr = _hinge_ref(x.float(), mode, scale, dtype)
            what = "hinge %s mode=%d n=%d %s" % (dtype, mode, n, kind)
            if G is not None:
                got = G.check(what)
                assert same_bits(got, gr), what + ": " + first_diff(got, gr)
            got, ref = float(L.check(what)[0]), scale * float(term.sum())
            if kind == "int":
                assert got == ref, what + ": %r != %r" % (got, ref)
            else:
                t, g = hinge_launch(n, CAP_HINGE)
                bound = (t + 8 + g) * U * scale * float(term.abs().sum())
                assert abs(got - ref) <= bound, what + ": err %g bound %g" % (abs(got - ref), bound)


@pytest.mark.parametrize("pitch_chunks", [1, 2])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_hinge_loss_nhwc(hip_device, dtype, mode, pitch_chunks):
    pitch = pitch_chunks * chunk_elems(dtype)
    scale = 0.5
    for n in size_classes(1, CAP_HINGE_NHWC, HINGE_PROD[0]) + HINGE_PROD[1:]:
        for kind in ("int", "normal"):
            x = _hinge_inputs(n, dtype, n % 947 + mode, kind)
            xm = torch.full((n, pitch), 7.0, dtype=dtype)              # junk in the padding channels of the input
            xm[:, 0] = x
            X, G = Guarded((n, pitch), dtype, hip_device, xm), Guarded((n, pitch), dtype, hip_device)
            L = Guarded((1,), F32, hip_device, torch.zeros(1))
            check(lib().s2p_hinge_loss_strided(dtype_id(dtype), ptr(X.t), n, pitch, mode, scale, ptr(L.t), ptr(G.t), stream()), "hinge nhwc")
            term, gr = _hinge_ref(x.float(), mode, scale, dtype)
            want = torch.zeros(n, pitch, dtype=dtype)                   # the sentinel-filled padding channels come back zero
            want[:, 0] = gr
            what = "hinge nhwc %s mode=%d pitch=%d n=%d %s" % (dtype, mode, pitch, n, kind)
            got = G.check(what)
            assert same_bits(got, want), what + ": " + first_diff(got, want)
            got, ref = float(L.check(what)[0]), scale * float(term.sum())
            if kind == "int":
                assert got == ref, what
            else:
                t, g = hinge_launch(n, CAP_HINGE_NHWC)
                assert abs(got - ref) <= (t + 8 + g) * U * scale * float(term.abs().sum()), what
    # through the wrapper, without a gradient
    xw = torch.full((2, 5, 5, pitch), 7.0, dtype=dtype)
    xw[..., 0] = ints((2, 5, 5), dtype, 3)
    L = torch.zeros(1, device=hip_device)
    assert ops.hinge_loss_nhwc(xw.to(hip_device), mode, scale, L, want_grad=False) is None
    assert float(L) == scale * float(_hinge_ref(xw[..., 0].float().reshape(-1), mode, scale, dtype)[0].sum())


@pytest.mark.parametrize("dtype", DTYPES)
def test_hinge_loss_x_off(hip_device, dtype):
    """ops.hinge_loss(x_off=...): the terms of a sub-range (the fake half of a 2N batch); the rest of the gradient buffer is untouched."""
    n, off, cnt = 700, 301, 333
    x = ints(n, dtype, 1)
    X, G = Guarded((n,), dtype, hip_device, x), Guarded((n,), dtype, hip_device)
    L = Guarded((1,), F32, hip_device, torch.zeros(1))
    ops.hinge_loss(X.t, cnt, 0, 0.5, L.t, G.t, x_off=off)
    term, gr = _hinge_ref(x[off:off + cnt].float(), 0, 0.5, dtype)
    want = sentinel_like(x)
    want[off:off + cnt] = gr
    assert same_bits(G.check(), want) and float(L.check()[0]) == 0.5 * float(term.sum())


# ---- channel sum (bias gradient) -------------------------------------------------------------------------------------------------------
def channel_sum_launch(pixels, C):
    """(t, g) of s2p_channel_sum, restating channel_sum_geom (norm.hip): nb pixel blocks of `rows` pixels each; a workgroup folds its
    rows in an order of its own, so t = rows (any order of summing k terms is within (k - 1) 2^-24 sum|terms|), g = nb."""
    slabs = _cdiv(C, 64)
    nb = _cdiv(1536, slabs)
    if nb * 128 > pixels:
        nb = pixels // 128
    nb = max(1, min(nb, 256))
    rows = _cdiv(pixels, nb)
    return rows, _cdiv(pixels, rows)


@pytest.mark.parametrize("C", [1, 3, 64, 200])
@pytest.mark.parametrize("dtype", DTYPES)
def test_channel_sum(hip_device, dtype, C):
    ce = chunk_elems(dtype)
    for pixels in (1, 2, 127, 128, 129, 1000, 13 * 13 * 64, 84 * 84 * 3 + 1) + ((64 * 84 * 84,) if C in (3, 64) else ()):
        for pitch in sorted({_cdiv(C, ce) * ce, _cdiv(C, ce) * ce + ce}):
            for kind in ("int", "normal"):
                if kind == "int":       # sparse: every partial sum stays below 2^24
                    dy = ints((pixels, pitch), dtype, pixels % 941, -1, 2)
                else:
                    dy = rnd((pixels, pitch), dtype, pixels % 941)
                dy[:, C:] = 9.0                                             # junk in the padding channels
                db0 = ints(C, F32, 3)
                DB = Guarded((C,), F32, hip_device, db0)
                check(lib().s2p_channel_sum(dtype_id(dtype), ptr(dy.to(hip_device)), pixels, C, pitch, ptr(DB.t), stream()), "channel_sum")
                what = "channel_sum %s C=%d pixels=%d pitch=%d %s" % (dtype, C, pixels, pitch, kind)
                got = DB.check(what).double()
                s = dy[:, :C].double().sum(0)
                if kind == "int":
                    assert torch.equal(got, db0.double() + s), what
                else:
                    t, g = channel_sum_launch(pixels, C)
                    sa = dy[:, :C].double().abs().sum(0)
                    bound = (t + 8 + g) * U * sa + g * U * db0.double().abs()
                    assert bool(((got - db0.double() - s).abs() <= bound).all()), what


# ---- Adam ----------------------------------------------------------------------------------------------------------------------------------
def _adam_ref(p, g, m, v, lr, b1, b2, eps, t, gs, dt):
    """One step of torch.optim.Adam's formula in dtype `dt` on fp32 inputs and fp32-rounded hyper-parameters."""
    f = lambda z: torch.tensor(z, dtype=F32).to(dt)
    lr, b1, b2, eps, gs = f(lr), f(b1), f(b2), f(eps), f(gs)
    p, g, m, v = p.to(dt), g.to(dt) * gs, m.to(dt), v.to(dt)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    p = p - (lr / bc1) * m / (v.sqrt() / bc2.sqrt() + eps)
    return p, m, v


def _ulp32(x):
    x = x.abs().float().clamp_min(2.0 ** -126)
    return torch.ldexp(torch.ones_like(x), torch.frexp(x).exponent - 24).double()


def _adam_compare(got, prev, g, hyper, t, what, worst):
    lr, b1, b2, eps, gs = hyper
    a64 = _adam_ref(*prev, lr, b1, b2, eps, t, gs, torch.float64)
    a32 = _adam_ref(*prev, lr, b1, b2, eps, t, gs, F32)
    for name, k, r64, r32 in zip("pmv", got, a64, a32):
        tol = torch.maximum(4 * (r32.double() - r64).abs().max(), _ulp32(r64))
        ratio = float(((k.double() - r64).abs() / tol).max())
        worst[name] = max(worst.get(name, 0.0), ratio)
        assert math.isfinite(ratio) and ratio <= 1.0, "%s step %d %s: |kernel - A64| / tol = %g" % (what, t, name, ratio)


ADAM_N = [1, 3, 4, 5, 1003, 4 * WG * CAP_ADAM, 4 * WG * CAP_ADAM + 1, 4 * WG * CAP_ADAM + 7]


@pytest.mark.parametrize("form", ["host", "dev", "dev_part"])
@pytest.mark.parametrize("betas", [(0.0, 0.9), (0.5, 0.999), (0.9, 0.999)])
def test_adam_one_step_at_a_time(hip_device, betas, form):
    dev = hip_device
    lr, eps, gs = 2e-4, 1e-8, 0.5
    hyper = (lr, betas[0], betas[1], eps, gs)
    for n in ADAM_N:
        big = n > 100000
        if big and betas != (0.5, 0.999):
            continue                    # the two-pass sizes with the trainer's own betas (the kernel does not branch on them)
        worst = {}
        p0 = rnd(n, F32, n % 937)
        g = rnd(n, F32, n % 937 + 1)
        g[::5] = 0.0                    # exact zeros: m, v stay 0 there and the parameter must not move
        P, M, V = Guarded((n,), F32, dev, p0), Guarded((n,), F32, dev, torch.zeros(n)), Guarded((n,), F32, dev, torch.zeros(n))
        Gd = Guarded((n,), F32, dev, g)
        sd = Guarded((1,), torch.int32, dev, torch.zeros(1, dtype=torch.int32))
        prev = (p0, g, torch.zeros(n), torch.zeros(n))
        steps = [1, 2, 3] if big else [1, 2, 3, 4, 5, 1000, 100000]
        cuts = [c for c in (4, 500, n // 8 * 4) if 0 < c < n]
        for i, t in enumerate(steps):
            if t >= 1000:
                sd.t.fill_(t - 1)       # jump of the device step counter
            if form == "host":
                ops.adam_step(P.t, Gd.t, M.t, V.t, lr, betas[0], betas[1], eps, t, gs)
            elif form == "dev" or not cuts:
                ops.adam_step_dev(P.t, Gd.t, M.t, V.t, lr, betas[0], betas[1], eps, sd.t, gs)
            else:                       # tail first with the tick, head second without (Pix2PixTrainer, EARLY_ADAM)
                c = cuts[i % len(cuts)]
                ops.adam_step_dev_part(P.t[c:], Gd.t[c:], M.t[c:], V.t[c:], lr, betas[0], betas[1], eps, sd.t, gs, tick=True)
                ops.adam_step_dev_part(P.t[:c], Gd.t[:c], M.t[:c], V.t[:c], lr, betas[0], betas[1], eps, sd.t, gs, tick=False)
            what = "adam %s betas=%s n=%d" % (form, betas, n)
            got = (P.check(what), M.check(what), V.check(what))
            assert same_bits(Gd.check(what), g)
            if form != "host":
                assert int(sd.check(what)[0]) == t
            _adam_compare(got, prev, g, hyper, t, what, worst)
            z = g == 0
            assert same_bits(got[0][z], p0[z]) and not bool(got[1][z].any()) and not bool(got[2][z].any())
            prev = (got[0], g, got[1], got[2])          # the kernel's own state feeds the next reference step: nothing accumulates
        print("adam %-8s betas=%s n=%d: max |kernel - A64| / tol  p %.3f  m %.3f  v %.3f" % (
            form, betas, n, worst["p"], worst["m"], worst["v"]))


def test_adam_refuses_unaligned_ranges(hip_device):
    """All three forms move 16-byte groups: a range that does not start at a multiple of 4 floats is refused before the launch (the
    head / tail split of FlatParams is checked on the CPU: tests/test_host_logic.py::test_flat_adam_ranges_are_16_byte_aligned)."""
    dev = hip_device
    n = 64
    bufs = [Guarded((n,), F32, dev, rnd(n, F32, i)) for i in range(4)]
    before = [b.t.cpu().clone() for b in bufs]
    sd = torch.zeros(1, dtype=torch.int32, device=dev)
    for bad in range(4):
        ps = [ptr(b.t) + (4 if i == bad else 0) for i, b in enumerate(bufs)]
        refuses(lib().s2p_adam_step_dev_part, *ps, n - 1, 1e-3, 0.5, 0.999, 1e-8, ptr(sd), 1.0, 1, stream(), match="aligned")
        refuses(lib().s2p_adam_step_dev, *ps, n - 1, 1e-3, 0.5, 0.999, 1e-8, ptr(sd), 1.0, stream(), match="aligned")
        refuses(lib().s2p_adam_step, *ps, n - 1, 1e-3, 0.5, 0.999, 1e-8, 1, 1.0, stream(), match="aligned")
    torch.cuda.synchronize()
    assert int(sd.item()) == 0                                       # no tick either
    for b, w in zip(bufs, before):
        assert same_bits(b.check(), w)
    with pytest.raises(RuntimeError, match="aligned"):
        ops.adam_step_dev_part(bufs[0].t[1:], bufs[1].t[1:], bufs[2].t[1:], bufs[3].t[1:], 1e-3, 0.5, 0.999, 1e-8, sd)
    # n == 0: a successful no-op without a tick
    assert lib().s2p_adam_step_dev(None, None, None, None, 0, 1e-3, 0.5, 0.999, 1e-8, None, 1.0, stream()) == 0
    assert int(sd.item()) == 0


# ---- positional encoding ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,L", [(1, 1), (17, 10), (24, 10), (17, 1), (1, 10)])
def test_posenc(hip_device, S, L):
    width = S * (1 + 2 * L)
    for N in (1, 5, 4096):
        for pitch in (width, (width + 3) // 4 * 4 + 4):
            s = rnd((N, S), F32, N + S)
            s[0, 0] = 8.0
            s.view(-1)[-1] = -8.0                          # 2^9 * 8: a large argument
            O = Guarded((N, pitch), F32, hip_device)
            check(lib().s2p_posenc_fwd(ptr(s.to(hip_device)), N, S, L, ptr(O.t), pitch, stream()), "posenc")
            got = O.check("posenc")
            assert same_bits(got[:, :S], s) and not bool(got[:, width:].any()), "posenc identity / padding columns"
            args = torch.cat([s * float(2 ** k) for k in range(L)], 1)                # exact in fp32
            for b, fn in ((0, torch.sin), (1, torch.cos)):
                cols = torch.cat([got[:, S + (2 * k + b) * S:S + (2 * k + b + 1) * S] for k in range(L)], 1)
                r64 = fn(args.double())
                tol = torch.maximum(8 * (fn(args).double() - r64).abs().max(), _ulp32(r64))
                ratio = float(((cols.double() - r64).abs() / tol).max())
                print("posenc S=%d L=%d N=%d %s: max |kernel - f64| / tol %.3f" % (S, L, N, fn.__name__, ratio))
                assert ratio <= 1.0, "posenc %s S=%d L=%d N=%d: ratio %g" % (fn.__name__, S, L, N, ratio)


# ---- refusals before launch, and empty calls ---------------------------------------------------------------------------------------------
def test_refusals_and_empty_calls(hip_device):
    dev = hip_device
    L = lib()
    st = stream()
    x = Guarded((2, 4, 4, 8), BF16, dev, rnd((2, 4, 4, 8), BF16, 1))
    y = Guarded((2, 4, 4, 8), BF16, dev)
    loss = Guarded((1,), F32, dev, torch.zeros(1))
    px, py, pl = ptr(x.t), ptr(y.t), ptr(loss.t)
    # unaligned pointers where the kernel moves whole chunks unconditionally
    refuses(L.s2p_maxpool2x2_fwd, 1, px + 2, 2, 4, 4, 8, py, st, match="aligned")
    refuses(L.s2p_maxpool2x2_fwd, 1, px, 2, 4, 4, 8, py + 2, st, match="aligned")
    refuses(L.s2p_maxpool2x2_bwd, 1, py + 2, px, 2, 4, 4, 8, py, st, match="aligned")
    refuses(L.s2p_maxpool2x2_bwd, 1, py, px, 2, 4, 4, 8, py + 2, st, match="aligned")
    refuses(L.s2p_reflect_pad_bwd, 1, px + 2, 2, 2, 2, 8, 1, py, st, match="aligned")
    refuses(L.s2p_reflect_pad_bwd, 1, px, 2, 2, 2, 8, 1, py + 2, st, match="aligned")
    refuses(L.s2p_hinge_loss_strided, 1, px, 32, 8, 0, 1.0, pl, py + 2, st, match="aligned")
    refuses(L.s2p_nchw_to_nhwc, 1, px, 1, 3, 2, 2, py + 2, 8, 0, 1, st, match="aligned")
    job = (_lib.L1Job * 1)(_lib.L1Job(px + 2, py, None, 64, 1.0, pl))
    refuses(L.s2p_l1_loss_multi, 1, job, 1, st, match="aligned")
    # chunk multiples, pitches, offsets
    refuses(L.s2p_maxpool2x2_fwd, 1, px, 2, 4, 4, 6, py, st, match="multiple")
    refuses(L.s2p_reflect_pad_bwd, 1, px, 2, 2, 2, 6, 1, py, st, match="multiple")
    refuses(L.s2p_reflect_pad_bwd, 1, px, 2, 2, 2, 8, 2, py, st, match="pad")            # pad >= H: not a reflection
    refuses(L.s2p_hinge_loss_strided, 1, px, 32, 6, 0, 1.0, pl, py, st, match="pitch")
    refuses(L.s2p_nchw_to_nhwc, 1, px, 1, 6, 2, 2, py, 8, 3, 1, st, match="pitch")
    refuses(L.s2p_nhwc_to_nchw, 1, px, 8, 6, 1, 3, 2, 2, py, 0, st, match="pitch")
    refuses(L.s2p_copy_channels, 1, px, 8, 6, py, 8, 0, 3, 4, 0, st, match="pitch")
    refuses(L.s2p_copy_channels, 1, px, 8, 0, py, 8, 6, 3, 4, 0, st, match="pitch")
    refuses(L.s2p_hinge_loss, 1, px, 16, 3, 1.0, pl, py, st)                             # mode
    # null pointers, negative sizes, unknown dtypes
    for fn, args in [
        (L.s2p_add, (1, None, px, py, 8, st)), (L.s2p_add, (1, px, px, None, 8, st)), (L.s2p_add, (1, px, px, py, -1, st)),
        (L.s2p_add, (5, px, px, py, 8, st)),
        (L.s2p_scale, (1, px, 8, None, st)), (L.s2p_scale, (1, None, 8, pl, st)), (L.s2p_scale, (1, px, -8, pl, st)),
        (L.s2p_cast, (1, None, 0, py, 8, st)), (L.s2p_cast, (1, px, 2, py, 8, st)), (L.s2p_cast, (1, px, 0, py, -8, st)),
        (L.s2p_act_bwd, (1, None, px, 8, 1, 0.0, py, st)), (L.s2p_act_bwd, (1, px, None, 8, 1, 0.0, py, st)),
        (L.s2p_act_bwd, (1, px, px, -1, 1, 0.0, py, st)),
        (L.s2p_copy_channels, (1, None, 8, 0, py, 8, 0, 3, 4, 0, st)), (L.s2p_copy_channels, (1, px, 8, 0, py, 8, 0, 3, -4, 0, st)),
        (L.s2p_maxpool2x2_fwd, (1, None, 2, 4, 4, 8, py, st)), (L.s2p_maxpool2x2_fwd, (1, px, -2, 4, 4, 8, py, st)),
        (L.s2p_maxpool2x2_bwd, (1, py, None, 2, 4, 4, 8, py, st)), (L.s2p_maxpool2x2_bwd, (1, None, px, 2, 4, 4, 8, py, st)),
        (L.s2p_avgpool3x3s2_fwd, (1, None, 2, 4, 4, 8, py, st)), (L.s2p_avgpool3x3s2_bwd, (1, px, 2, 4, 4, 8, None, 0, st)),
        (L.s2p_avgpool3x3s2_fwd, (1, px, 2, -4, 4, 8, py, st)),
        (L.s2p_resize_nearest, (1, None, 2, 4, 4, 8, py, 4, 4, st)), (L.s2p_resize_nearest, (1, px, 2, 0, 4, 8, py, 4, 4, st)),
        (L.s2p_reflect_pad_bwd, (1, None, 2, 2, 2, 8, 1, py, st)), (L.s2p_reflect_pad_bwd, (1, px, 2, 2, 2, 8, -1, py, st)),
        (L.s2p_nchw_to_nhwc, (1, None, 1, 3, 2, 2, py, 8, 0, 1, st)), (L.s2p_nhwc_to_nchw, (1, px, 8, 0, 1, 3, 2, 2, None, 0, st)),
        (L.s2p_l1_loss, (1, None, px, 8, 1.0, pl, None, 0, st)), (L.s2p_l1_loss, (1, px, px, 8, 1.0, None, None, 0, st)),
        (L.s2p_l1_loss, (1, px, px, -8, 1.0, pl, None, 0, st)),
        (L.s2p_hinge_loss, (1, None, 8, 0, 1.0, pl, None, st)), (L.s2p_hinge_loss, (1, px, -8, 0, 1.0, pl, None, st)),
        (L.s2p_hinge_loss_strided, (1, px, 8, 8, 0, 1.0, None, None, st)), (L.s2p_hinge_loss_strided, (1, px, -8, 8, 0, 1.0, pl, None, st)),
        (L.s2p_posenc_fwd, (None, 2, 3, 1, py, 9, st)), (L.s2p_posenc_fwd, (px, -2, 3, 1, py, 9, st)),
        (L.s2p_posenc_fwd, (px, 2, 3, 1, py, 8, st)),
        (L.s2p_u8_to_nhwc, (1, px, 4, 3, None, 8, st)), (L.s2p_nhwc_to_u8, (1, px, 8, 4, 9, py, st)),
        (L.s2p_adam_step_dev, (None, px, px, px, 8, 1e-3, 0.5, 0.9, 1e-8, pl, 1.0, st)),
        (L.s2p_adam_step_dev, (px, px, px, px, -8, 1e-3, 0.5, 0.9, 1e-8, pl, 1.0, st)),
        (L.s2p_adam_step, (px, px, px, px, 8, 1e-3, 0.5, 0.9, 1e-8, 0, 1.0, st)),
    ]:
        refuses(fn, *args)
    # a size of zero: success, nothing launched, pointers not looked at
    for fn, args in [
        (L.s2p_add, (1, None, None, None, 0, st)), (L.s2p_scale, (1, None, 0, None, st)), (L.s2p_cast, (1, None, 0, None, 0, st)),
        (L.s2p_act_bwd, (1, None, None, 0, 1, 0.0, None, st)), (L.s2p_copy_channels, (1, None, 8, 0, None, 8, 0, 3, 0, 0, st)),
        (L.s2p_copy_channels, (1, None, 8, 0, None, 8, 0, 0, 5, 0, st)),
        (L.s2p_maxpool2x2_fwd, (1, None, 0, 4, 4, 8, None, st)), (L.s2p_maxpool2x2_fwd, (1, None, 2, 1, 4, 8, None, st)),
        (L.s2p_maxpool2x2_bwd, (1, None, None, 0, 4, 4, 8, None, st)),
        (L.s2p_avgpool3x3s2_fwd, (1, None, 0, 4, 4, 8, None, st)), (L.s2p_avgpool3x3s2_bwd, (1, None, 2, 0, 4, 8, None, 1, st)),
        (L.s2p_resize_nearest, (1, None, 2, 4, 4, 8, None, 0, 4, st)), (L.s2p_reflect_pad_bwd, (1, None, 0, 4, 4, 8, 1, None, st)),
        (L.s2p_nchw_to_nhwc, (1, None, 0, 3, 2, 2, None, 8, 0, 1, st)), (L.s2p_nhwc_to_nchw, (1, None, 8, 0, 0, 3, 2, 2, None, 0, st)),
        (L.s2p_l1_loss, (1, None, None, 0, 1.0, None, None, 0, st)), (L.s2p_hinge_loss, (1, None, 0, 0, 1.0, None, None, st)),
        (L.s2p_hinge_loss_strided, (1, None, 0, 8, 0, 1.0, None, None, st)), (L.s2p_posenc_fwd, (None, 0, 3, 1, None, 9, st)),
        (L.s2p_u8_to_nhwc, (1, None, 0, 3, None, 8, st)), (L.s2p_nhwc_to_u8, (1, None, 8, 0, 3, None, st)),
        (L.s2p_adam_step, (None, None, None, None, 0, 1e-3, 0.5, 0.9, 1e-8, 1, 1.0, st)),
        (L.s2p_adam_step_dev_part, (None, None, None, None, 0, 1e-3, 0.5, 0.9, 1e-8, None, 1.0, 1, st)),
    ]:
        assert fn(*args) == 0, (fn.__name__, args)
    # a window-less max-pool backward (H = 1) still zero-fills dx
    dx = Guarded((2, 1, 4, 8), BF16, dev)
    check(L.s2p_maxpool2x2_bwd(1, None, px, 2, 1, 4, 8, ptr(dx.t), st), "maxpool bwd, H = 1")
    assert not bool(dx.check().float().any())
    torch.cuda.synchronize()
    assert same_bits(y.check(), sentinel_like(y.t.cpu())) and float(loss.check()[0]) == 0.0        # none of the refused calls ran
