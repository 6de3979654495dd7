"""Raw (non-autograd) wrappers over the C ABI.  Tensors are explicit NHWC: shape [N, H, W, pitch] (contiguous),
where `pitch` >= channel count and is a multiple of the 16-byte chunk (4 fp32 / 8 bf16 elements).

Each wrapper cites the torch op of the SPADE-lineage model it replaces (the reference checkout itself ships no
generator code: SURVEY.md section 0; lineage README.md:72-75).
"""
import ctypes

import torch

from . import _lib
from ._lib import (ACT_LRELU, ACT_NONE, ACT_RELU, ACT_TANH, EPI_ADD, EPI_MUL_ACTGRAD, EPI_STORE, ConvDesc,
                   check, chunk_elems, dtype_id, lib, ptr, stream)

IN_EPS = 1e-5

# When True, every "side stream" helper of the networks returns the CURRENT stream: the step runs as one serial chain of
# launches.  bench.py sets it for its instrumented roofline step only, so that a kernel's HIP-event duration is that of the
# kernel alone (in the product configuration independent chains overlap on several streams and would inflate each
# other's per-launch times).
SERIALIZE = False


# Optional in-situ profiler used by bench.py's roofline leg: when PROFILE is a list, every MFMA conv launch is
# bracketed by two events on the launch stream and logged with its algorithmic FLOPs (2*MACs, un-padded channels).
PROFILE = None


class _Prof:
    def __init__(self, kind, geom, N, H, W, dtype):
        self.on = PROFILE is not None
        if self.on:
            Ho, Wo = geom.out_hw(H, W)
            pix = N * H * W if geom.transposed else N * Ho * Wo
            self.rec = dict(kind=kind, flops=2.0 * pix * geom.cin * geom.cout * geom.k * geom.k * geom.groups,
                            shape=(N, H, W, geom.cin, geom.cout, geom.k, geom.stride, geom.groups, int(geom.transposed)),
                            dtype=str(dtype), net=getattr(geom, "net", ""))
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def done(self):
        if self.on:
            self.e1.record()
            self.rec["events"] = (self.e0, self.e1)
            PROFILE.append(self.rec)


class _ProfNorm:
    """Same hook for the IN / MAT kernels: algorithmic HBM bytes instead of FLOPs."""

    def __init__(self, kind, x, C, nbytes, modulated):
        self.on = PROFILE is not None
        if self.on:
            N, H, W, _ = x.shape
            self.rec = dict(kind=kind, flops=0.0, bytes=float(nbytes), shape=(N, H, W, C, int(modulated)), dtype=str(x.dtype))
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def done(self):
        if self.on:
            self.e1.record()
            self.rec["events"] = (self.e0, self.e1)
            PROFILE.append(self.rec)


def pad_to(c, ce):
    return (c + ce - 1) // ce * ce


_MAT_FUSED = {}           # (geometry, problem) -> s2p_conv2d_mat_is_fused, asked once (conv_fwd_mat)
SKIP_UNUSED_Y = True      # conv_fwd_mat(want_y=False) really skips the conv output (tools/ab_step.py flips it for same-box A/Bs)


class ConvGeom:
    """Static geometry of one conv layer (F.conv2d / F.conv_transpose2d arguments)."""

    def __init__(self, cin, cout, k, stride=1, pad=0, transposed=False, reflect=False, groups=1,
                 output_padding=0, x_gstride=0, y_gstride=0, net=""):
        self.net = net              # which network the layer belongs to ("G" / "D" / "VGG": bench.py's per-network aggregates)
        self.cin, self.cout, self.k = cin, cout, k
        self.stride, self.pad = stride, pad
        self.transposed, self.reflect, self.groups = transposed, reflect, groups
        self.output_padding = output_padding
        self.x_gstride, self.y_gstride = x_gstride, y_gstride

    def out_hw(self, H, W):
        k, s, p = self.k, self.stride, self.pad
        if self.transposed:
            return ((H - 1) * s - 2 * p + k + self.output_padding, (W - 1) * s - 2 * p + k + self.output_padding)
        return ((H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1)

    def desc(self, dtype, N, H, W, cin_pad, x_pitch, y_pitch):
        Ho, Wo = self.out_hw(H, W)
        return ConvDesc(dtype_id(dtype), N, H, W, cin_pad, x_pitch, Ho, Wo, self.cout, y_pitch,
                        self.k, self.k, self.stride, self.pad, int(self.transposed), int(self.reflect),
                        self.groups, self.x_gstride, self.y_gstride, self.cin if self.groups == 1 else 0)


def conv_fwd(geom, x, w_fwd, bias, cin_pad, y_pitch=None, act=ACT_NONE, slope=0.2, aux=None, epi=EPI_STORE,
             out=None):
    """y = act(conv(x, w) + b) [+ aux]   (F.conv2d / F.conv_transpose2d + bias + activation)."""
    N, H, W, xp = x.shape
    ce = chunk_elems(x.dtype)
    Ho, Wo = geom.out_hw(H, W)
    if y_pitch is None:
        y_pitch = pad_to(geom.cout * geom.groups if geom.groups > 1 else geom.cout, ce)
    y = out if out is not None else torch.empty((N, Ho, Wo, y_pitch), dtype=x.dtype, device=x.device)
    d = geom.desc(x.dtype, N, H, W, cin_pad, xp, y_pitch)
    need = lib().s2p_conv2d_fwd_workspace(ctypes.byref(d), epi)        # > 0: small-map launch that splits K over the idle CUs
    ws = torch.empty(need, dtype=torch.uint8, device=x.device) if need else None
    pr = _Prof("fwd", geom, N, H, W, x.dtype)
    check(lib().s2p_conv2d_fwd_ws(ctypes.byref(d), ptr(x), ptr(w_fwd), ptr(bias), ptr(aux), ptr(y), act, slope, epi,
                                  ptr(ws), need, stream()), "s2p_conv2d_fwd")
    pr.done()
    return y


def conv_path(geom, dtype, x_shape, cin_pad, dgrad=False, workspace=True):
    """The dispatcher's path (_lib.PATH_*; _lib.halo_path(kind) for the halo-resident kernel, _lib.thin_path(kind) for the thin-Cout
    forward) of conv_fwd / conv_dgrad on an input of `x_shape` = (N, H, W, x_pitch): a dry run on the host, nothing is launched.
    workspace=False: as called without a scratch."""
    N, H, W, xp = x_shape
    ce = chunk_elems(dtype)
    d = geom.desc(dtype, N, H, W, cin_pad, xp, pad_to(geom.cout * geom.groups if geom.groups > 1 else geom.cout, ce))
    return int(lib().s2p_conv2d_path(ctypes.byref(d), int(dgrad), int(workspace)))


def conv_fwd_mat(geom, x, w_fwd, bias, cin_pad, gb, gb_off, gb_st, st_off, act=ACT_LRELU, slope=0.2, aux=None, epi=EPI_STORE,
                 want_y=True):
    """conv (+ bias, + residual aux) followed by InstanceNorm + MAT modulation + activation of its output, one launch where
    the plane-resident kernel applies (s2p_conv2d_fwd_mat; conv_fwd + in_norm_fwd otherwise).
    Returns (y, y_mat, stats): the conv output (kept for the backward), the modulated activation, the norm statistics.
    want_y=False (a forward without a backward): where the launch is fused the conv output is not written at all (y is None)."""
    N, H, W, xp = x.shape
    Ho, Wo = geom.out_hw(H, W)
    C = geom.cout
    y_pitch = pad_to(C, chunk_elems(x.dtype))
    y_mat = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
    stats = torch.empty(lib().s2p_in_stats_floats(N, Ho * Wo, C), dtype=torch.float32, device=x.device)
    d = geom.desc(x.dtype, N, H, W, cin_pad, xp, y_pitch)
    y = None
    if not SKIP_UNUSED_Y:
        want_y = True
    if not want_y:
        # (the answer is a property of the geometry: asked once -- the query walks the launcher's planning path on the host, which an
        # eager forward cannot afford six times per pass)
        # (a module-level table: layers compare their geometry objects attribute by attribute -- ConvLayer.wgrad_many -- so nothing
        # may be cached ON them)
        key = (geom.cin, geom.cout, geom.k, geom.stride, geom.pad, geom.transposed, geom.reflect, geom.groups, geom.output_padding,
               x.dtype, N, H, W, cin_pad, xp, gb is not None)
        if key not in _MAT_FUSED:
            _MAT_FUSED[key] = bool(lib().s2p_conv2d_mat_is_fused(ctypes.byref(d), 0, 1 if gb is not None else 0))
        want_y = not _MAT_FUSED[key]
    if want_y:
        y = torch.empty((N, Ho, Wo, y_pitch), dtype=x.dtype, device=x.device)
    need = lib().s2p_conv2d_fwd_workspace(ctypes.byref(d), epi)
    ws = torch.empty(need, dtype=torch.uint8, device=x.device) if need else None
    gbp, gb_pitch, stp, st_pitch = _gb_args(gb, gb_off, gb_st, st_off)
    pr = _Prof("fwd", geom, N, H, W, x.dtype)
    if pr.on:       # the fused launch also moves the norm's bytes: gamma, beta read + the modulated tensor written
        pr.rec["norm_bytes"] = float(N * Ho * Wo * C * x.element_size() * 3)
        pr.rec["variant"] = "mat_fwd"
    check(lib().s2p_conv2d_fwd_mat(ctypes.byref(d), ptr(x), ptr(w_fwd), ptr(bias), ptr(aux), ptr(y), epi, gbp, gb_pitch, stp,
                                   st_pitch, act, slope, IN_EPS, ptr(y_mat), C, ptr(stats), ptr(ws), need, stream()),
          "s2p_conv2d_fwd_mat")
    pr.done()
    return y, y_mat, stats


def conv_dgrad(geom, dy, w_bwd, x_shape, cin_pad, aux=None, epi=EPI_STORE, aux_act=ACT_NONE, slope=0.2, aux2=None):
    """dx of the conv (cudnn_convolution_backward_input equivalent).  For reflect-padded convs the padded-grid
    gradient is folded back (adjoint of F.pad(mode='reflect'))."""
    N, H, W, xp = x_shape
    d = geom.desc(dy.dtype, N, H, W, cin_pad, xp, dy.shape[3])
    if geom.reflect:
        p = geom.pad
        dxp = torch.empty((N, H + 2 * p, W + 2 * p, xp), dtype=dy.dtype, device=dy.device)
        need = lib().s2p_conv2d_dgrad_workspace(ctypes.byref(d))
        ws = torch.empty(need, dtype=torch.uint8, device=dy.device) if need else None
        pr = _Prof("dgrad", geom, N, H, W, dy.dtype)
        check(lib().s2p_conv2d_dgrad_ws(ctypes.byref(d), ptr(dy), ptr(w_bwd), None, None, ptr(dxp), EPI_STORE, ACT_NONE, 0.0,
                                        ptr(ws), need, stream()), "s2p_conv2d_dgrad")
        pr.done()
        dx = torch.empty((N, H, W, xp), dtype=dy.dtype, device=dy.device)
        check(lib().s2p_reflect_pad_bwd(dtype_id(dy.dtype), ptr(dxp), N, H, W, xp, p, ptr(dx), stream()),
              "s2p_reflect_pad_bwd")
        if aux2 is not None:
            dx = add(dx, aux2, out=dx)
        if epi == EPI_MUL_ACTGRAD:
            dx = act_bwd(dx, aux, aux_act, slope)
        elif epi == EPI_ADD:
            dx = add(dx, aux, out=dx)
        return dx
    dx = torch.empty((N, H, W, xp), dtype=dy.dtype, device=dy.device)
    if xp != cin_pad * geom.groups:
        dx.zero_()
    need = lib().s2p_conv2d_dgrad_workspace(ctypes.byref(d))
    ws = torch.empty(need, dtype=torch.uint8, device=dy.device) if need else None
    pr = _Prof("dgrad", geom, N, H, W, dy.dtype)
    check(lib().s2p_conv2d_dgrad_ws(ctypes.byref(d), ptr(dy), ptr(w_bwd), ptr(aux), ptr(aux2), ptr(dx), epi, aux_act, slope,
                                    ptr(ws), need, stream()), "s2p_conv2d_dgrad")
    pr.done()
    return dx


def conv_dgrad_mat(geom, dy, w_bwd, xn, cin_pad, stats, gb, gb_off, gb_st, st_off, act, slope, dgb, dgb_off, dgb_st, dst_off,
                   res=None, aux=None):
    """dgrad of a conv whose input was a MAT / InstanceNorm's output, fused with that norm's backward (s2p_conv2d_dgrad_mat):
    returns dL/d(xn) (+ res); writes d(gamma|beta) as in_bwd does.  xn: the norm's input [N,H,W,C].  aux: a second gradient
    arriving at the norm's output (layout of the dgrad result), added before the norm backward."""
    N, H, W, xp = xn.shape
    C = geom.cin
    if cin_pad != C or xp != C:
        # (a norm's channel count is a multiple of the 16-byte chunk -- the norm kernels require it -- so its tensor is dense; widths such
        # as --ndf 12 give 24 / 48 / 96 normed channels and take this path unchanged: tests/test_model_gpu.py::test_small_width_discriminator)
        raise ValueError("conv_dgrad_mat: the norm's tensor must be dense in channels (C %d, cin_pad %d, pitch %d)" % (C, cin_pad, xp))
    d = geom.desc(dy.dtype, N, H, W, cin_pad, C, dy.shape[3])
    dxn = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    fused = bool(lib().s2p_conv2d_mat_is_fused(ctypes.byref(d), 1, int(gb is not None))) and (aux is None or geom.k != 3)
    # scratch of the two-launch form only when that form runs
    d_mid = None if fused else torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    sums = None if fused else torch.empty(lib().s2p_in_bwd_sums_floats(N, H * W, C), dtype=torch.float32, device=dy.device)
    need = lib().s2p_conv2d_dgrad_workspace(ctypes.byref(d))
    ws = torch.empty(need, dtype=torch.uint8, device=dy.device) if need else None
    gbp, gb_pitch, stp, st_pitch = _gb_args(gb, gb_off, gb_st, st_off)
    dgbp = dgb.data_ptr() + dgb_off * dgb.element_size() if dgb is not None else None
    dstp = dgb_st.data_ptr() + dst_off * 4 if dgb_st is not None else None
    _ = ptr(dgb), ptr(dgb_st)
    if res is not None:
        assert res.shape == dxn.shape and res.dtype == dxn.dtype and res.is_contiguous()
    if aux is not None:
        assert aux.shape == dxn.shape and aux.dtype == dxn.dtype and aux.is_contiguous()
    pr = _Prof("dgrad", geom, N, H, W, dy.dtype)
    if pr.on:       # + the norm backward's bytes: xn, gamma, beta read (+ res, aux), dxn, d(gamma), d(beta) written; dy is the conv's own
        nt = (2 + (res is not None) + (aux is not None)) if gb is None else (6 + (res is not None) + (aux is not None))
        pr.rec["norm_bytes"] = float(N * H * W * C * dy.element_size() * nt)
        pr.rec["variant"] = "mat_bwd"
    check(lib().s2p_conv2d_dgrad_mat(ctypes.byref(d), ptr(dy), ptr(w_bwd), ptr(d_mid), ptr(aux), ptr(xn), xp, ptr(stats), gbp, gb_pitch,
                                     stp, st_pitch, act, slope, IN_EPS, ptr(sums), ptr(dxn), C, dgbp,
                                     dgb.shape[3] if dgb is not None else 0, dstp,
                                     dgb_st.shape[1] if dgb_st is not None else 0, ptr(res), C if res is not None else 0,
                                     ptr(ws), need, stream()), "s2p_conv2d_dgrad_mat")
    pr.done()
    return dxn


def conv_wgrad(geom, x, dy, dw, cin_pad, cin_real, cout_real, dw_gstride=0, splitk=0, db=None, deterministic=False):
    """dw += wgrad (cudnn_convolution_backward_weight equivalent); dw is an fp32 view in channels-last layout.
    The K-split partial sums go through a scratch buffer and are added in a fixed order (s2p_conv2d_wgrad_ws): no atomics
    for bf16; `deterministic` asks for the larger scratch with which fp32 tensors take the same route."""
    N, H, W, xp = x.shape
    d = geom.desc(x.dtype, N, H, W, cin_pad, xp, dy.shape[3])
    if deterministic:
        need = lib().s2p_conv2d_wgrad_det_workspace(ctypes.byref(d), cin_real, cout_real, splitk)
    else:
        need = lib().s2p_conv2d_wgrad_workspace(ctypes.byref(d), cin_real, cout_real)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    pr = _Prof("wgrad", geom, N, H, W, x.dtype)
    check(lib().s2p_conv2d_wgrad_ws(ctypes.byref(d), ptr(x), ptr(dy), ptr(dw), ptr(db), cin_real, cout_real, dw_gstride, splitk,
                                    ptr(ws), need, stream()), "s2p_conv2d_wgrad_ws")
    pr.done()


def conv_wgrad_batched(geom, jobs, cin_pad, cin_real, cout_real):
    """dw_j += wgrad(x_j, dy_j), db_j += sum dy_j for several convs of the SAME geometry in one launch
    (s2p_conv2d_wgrad_batched).  jobs: list of (x, x_ch_off, dy, dy_ch_off, dw, db): x / dy NHWC tensors (all the
    same shape) read from channel offset *_ch_off (a grouped conv is one job per group), dw fp32 view, db fp32 view or
    None.  `geom` must describe ONE group (groups == 1)."""
    x0, _, dy0 = jobs[0][0], jobs[0][1], jobs[0][2]
    N, H, W, xp = x0.shape
    d = geom.desc(x0.dtype, N, H, W, cin_pad, xp, dy0.shape[3])
    arr = (_lib.WgradJob * len(jobs))()
    esz = x0.element_size()
    for i, (x, xo, dy, dyo, dw, db) in enumerate(jobs):
        assert x.shape == x0.shape and dy.shape == dy0.shape
        arr[i] = _lib.WgradJob(ptr(x) + xo * esz, ptr(dy) + dyo * esz, ptr(dw), ptr(db))
    need = lib().s2p_conv2d_wgrad_batched_workspace(ctypes.byref(d), len(jobs), cin_real, cout_real)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x0.device)
    pr = _Prof("wgrad", geom, N, H, W, x0.dtype)
    if pr.on:
        pr.rec["flops"] *= len(jobs)
        pr.rec["shape"] = pr.rec["shape"][:7] + (len(jobs),) + pr.rec["shape"][8:]
    check(lib().s2p_conv2d_wgrad_batched(ctypes.byref(d), arr, len(jobs), cin_real, cout_real, ptr(ws), need, stream()),
          "s2p_conv2d_wgrad_batched")
    pr.done()


def channel_sum(dy, C, db, deterministic=False):
    """db += dy.sum over pixels (bias gradient); `deterministic`: partial sums in a scratch + fixed-order reduce, no atomics."""
    pixels = dy.shape[0] * dy.shape[1] * dy.shape[2]
    if deterministic:
        need = lib().s2p_channel_sum_workspace(pixels, C)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dy.device)
        check(lib().s2p_channel_sum_ws(dtype_id(dy.dtype), ptr(dy), pixels, C, dy.shape[3], ptr(db), ptr(ws), need, stream()),
              "s2p_channel_sum_ws")
        return
    check(lib().s2p_channel_sum(dtype_id(dy.dtype), ptr(dy), pixels, C, dy.shape[3], ptr(db), stream()),
          "s2p_channel_sum")


def in_stats(x, C):
    """Per-(n,c) InstanceNorm statistics: an opaque buffer of partial moments (include/s2p_hip.h) consumed by
    in_apply_fwd / in_bwd with the same x shape."""
    N, H, W, xp = x.shape
    stats = torch.empty(lib().s2p_in_stats_floats(N, H * W, C), dtype=torch.float32, device=x.device)
    pr = _ProfNorm("norm_stats", x, C, N * H * W * C * x.element_size(), False)
    check(lib().s2p_in_stats(dtype_id(x.dtype), ptr(x), N, H * W, C, xp, IN_EPS, ptr(stats), stream()), "s2p_in_stats")
    pr.done()
    return stats


def _gb_args(gb, gb_off, gb_st, st_off):
    gbp = gb.data_ptr() + gb_off * gb.element_size() if gb is not None else None
    gb_pitch = gb.shape[3] if gb is not None else 0
    stp = gb_st.data_ptr() + st_off * 4 if gb_st is not None else None
    st_pitch = gb_st.shape[1] if gb_st is not None else 0
    return gbp, gb_pitch, stp, st_pitch


def in_apply_fwd(x, C, stats, gb=None, gb_off=0, gb_st=None, st_off=0, act=ACT_NONE, slope=0.2):
    """F.instance_norm(x) * (1 + gamma) + beta, then activation; gamma/beta = image map + per-sample state affine."""
    N, H, W, xp = x.shape
    y = torch.empty((N, H, W, C), dtype=x.dtype, device=x.device)
    gbp, gb_pitch, stp, st_pitch = _gb_args(gb, gb_off, gb_st, st_off)
    pr = _ProfNorm("norm_fwd", x, C, N * H * W * C * x.element_size() * (4 if gb is not None else 2), gb is not None)
    check(lib().s2p_in_apply_fwd(dtype_id(x.dtype), ptr(x), N, H * W, C, xp, ptr(stats), gbp, gb_pitch, stp, st_pitch,
                                 act, slope, IN_EPS, ptr(y), C, stream()), "s2p_in_apply_fwd")
    pr.done()
    return y


def in_norm_fwd(x, C, gb=None, gb_off=0, gb_st=None, st_off=0, act=ACT_NONE, slope=0.2):
    """in_stats + in_apply_fwd as ONE call (one fused launch for small planes): returns (y, stats)."""
    N, H, W, xp = x.shape
    stats = torch.empty(lib().s2p_in_stats_floats(N, H * W, C), dtype=torch.float32, device=x.device)
    y = torch.empty((N, H, W, C), dtype=x.dtype, device=x.device)
    gbp, gb_pitch, stp, st_pitch = _gb_args(gb, gb_off, gb_st, st_off)
    esz = x.element_size()
    pr = _ProfNorm("norm_fwd", x, C, N * H * W * C * esz * ((4 if gb is not None else 2) + 1), gb is not None)
    check(lib().s2p_in_norm_fwd(dtype_id(x.dtype), ptr(x), N, H * W, C, xp, gbp, gb_pitch, stp, st_pitch, act, slope, IN_EPS,
                                ptr(y), C, ptr(stats), stream()), "s2p_in_norm_fwd")
    pr.done()
    return y, stats


def in_bwd(da, x, C, stats, gb=None, gb_off=0, gb_st=None, st_off=0, act=ACT_NONE, slope=0.2, dgb=None, dgb_off=0,
           dgb_st=None, dst_off=0, res=None):
    """Backward of in_apply_fwd.  Returns dx; writes d(gamma_img|beta_img) into dgb at channel offset dgb_off and
    d(gamma_st|beta_st) into the fp32 [N, pitch] tensor dgb_st at column offset dst_off (layout of gb_st).
    res: optional [N,H,W,C] tensor added to dx in the same launch (the skip-connection gradient of a residual block)."""
    N, H, W, xp = x.shape
    sums = torch.empty(lib().s2p_in_bwd_sums_floats(N, H * W, C), dtype=torch.float32, device=x.device)
    gbp, gb_pitch, stp, st_pitch = _gb_args(gb, gb_off, gb_st, st_off)
    dt = dtype_id(x.dtype)
    el = N * H * W * C * x.element_size()
    # reduce reads x, da (+gamma, beta); apply reads the same and writes dx (+dgamma, dbeta)
    pr = _ProfNorm("norm_bwd", x, C, el * ((4 + 4 + 3) if gb is not None else (2 + 2 + 1)), gb is not None)
    dx = torch.empty((N, H, W, C), dtype=x.dtype, device=x.device)
    dgbp = dgb.data_ptr() + dgb_off * dgb.element_size() if dgb is not None else None
    dstp = dgb_st.data_ptr() + dst_off * 4 if dgb_st is not None else None
    _ = ptr(dgb), ptr(dgb_st)
    # one fused launch for small planes, the reduce + apply pair otherwise (s2p_in_norm_bwd decides)
    if res is not None:
        assert res.shape == dx.shape and res.dtype == dx.dtype and res.is_contiguous()
    check(lib().s2p_in_norm_bwd_res(dt, ptr(da), da.shape[3], ptr(x), N, H * W, C, xp, ptr(stats), gbp, gb_pitch, stp,
                                    st_pitch, act, slope, IN_EPS, ptr(sums), ptr(dx), C, dgbp,
                                    dgb.shape[3] if dgb is not None else 0, dstp,
                                    dgb_st.shape[1] if dgb_st is not None else 0, ptr(res), C if res is not None else 0,
                                    stream()), "s2p_in_norm_bwd")
    pr.done()
    return dx


def linear_fwd(x, w_fwd, bias, K, N, act=ACT_NONE, slope=0.2, n_store=None):
    """y = act(x @ w.T + b) for the small fp32 layers of the state path.  x: fp32 [M, x_pitch]; w_fwd: packed
    [1][N][1][Kpad] fp32 (ParamStore pack); returns fp32 [M, n_store] (columns >= N zero)."""
    M, xp = x.shape
    n_store = pad_to(N, 4) if n_store is None else n_store
    y = torch.empty((M, n_store), dtype=torch.float32, device=x.device)
    check(lib().s2p_linear_fwd(ptr(x), M, K, xp, ptr(w_fwd), w_fwd.shape[-1], ptr(bias), N, act, slope, ptr(y), n_store,
                               n_store, stream()), "s2p_linear_fwd")
    return y


def linear_bwd(x, dy, y, w_bwd, K, k_real, N, act, slope, dw, db, need_dx=True):
    """Backward of linear_fwd: dw += dpre.T @ x, db += dpre.sum(0), returns dx = dpre @ w (or None); dpre = dy * act'(y)."""
    M, xp = x.shape
    dx = torch.empty((M, xp), dtype=torch.float32, device=x.device) if need_dx else None
    need = lib().s2p_linear_bwd_workspace(M, K, N) if need_dx else 0
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    check(lib().s2p_linear_bwd(ptr(x), xp, ptr(dy), dy.shape[1], ptr(y), y.shape[1] if y is not None else 0, M, K, k_real, N,
                               ptr(w_bwd), w_bwd.shape[-1] if w_bwd is not None else 0, act, slope, ptr(dw), k_real, ptr(db),
                               ptr(dx), xp, ptr(ws), need, stream()), "s2p_linear_bwd")
    return dx


def posenc(state, L, pitch):
    N, S = state.shape
    out = torch.empty((N, pitch), dtype=torch.float32, device=state.device)
    check(lib().s2p_posenc_fwd(ptr(state), N, S, L, ptr(out), pitch, stream()), "s2p_posenc_fwd")
    return out


def avgpool_fwd(x):
    N, H, W, C = x.shape
    y = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), dtype=x.dtype, device=x.device)
    check(lib().s2p_avgpool3x3s2_fwd(dtype_id(x.dtype), ptr(x), N, H, W, C, ptr(y), stream()), "s2p_avgpool3x3s2_fwd")
    return y


def avgpool_bwd(dy, x_shape, dx=None, accumulate=False):
    N, H, W, C = x_shape
    if dx is None:
        dx = torch.empty(x_shape, dtype=dy.dtype, device=dy.device)
    check(lib().s2p_avgpool3x3s2_bwd(dtype_id(dy.dtype), ptr(dy), N, H, W, C, ptr(dx), int(accumulate), stream()),
          "s2p_avgpool3x3s2_bwd")
    return dx


def maxpool_fwd(x):
    N, H, W, C = x.shape
    y = torch.empty((N, H // 2, W // 2, C), dtype=x.dtype, device=x.device)
    check(lib().s2p_maxpool2x2_fwd(dtype_id(x.dtype), ptr(x), N, H, W, C, ptr(y), stream()), "s2p_maxpool2x2_fwd")
    return y


def maxpool_bwd(dy, x):
    N, H, W, C = x.shape
    dx = torch.empty_like(x)
    check(lib().s2p_maxpool2x2_bwd(dtype_id(x.dtype), ptr(dy), ptr(x), N, H, W, C, ptr(dx), stream()),
          "s2p_maxpool2x2_bwd")
    return dx


def resize_nearest(x, Ho, Wo):
    N, H, W, C = x.shape
    y = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
    check(lib().s2p_resize_nearest(dtype_id(x.dtype), ptr(x), N, H, W, C, ptr(y), Ho, Wo, stream()), "s2p_resize_nearest")
    return y


def nchw_to_nhwc(x, dtype, pitch, out=None, c_off=0, zero_pad=True):
    """fp32 NCHW image -> NHWC compute-dtype tensor with zero-padded channel pitch."""
    N, C, H, W = x.shape
    x = x.contiguous()
    y = out if out is not None else torch.empty((N, H, W, pitch), dtype=dtype, device=x.device)
    check(lib().s2p_nchw_to_nhwc(dtype_id(dtype), ptr(x), N, C, H, W, ptr(y), pitch, c_off, int(zero_pad), stream()),
          "s2p_nchw_to_nhwc")
    return y


def nhwc_to_nchw(x, C, c_off=0, out=None, accumulate=False):
    N, H, W, xp = x.shape
    y = out if out is not None else torch.empty((N, C, H, W), dtype=torch.float32, device=x.device)
    if not y.is_contiguous() or tuple(y.shape) != (N, C, H, W) or y.dtype != torch.float32:
        raise ValueError("nhwc_to_nchw: `out` must be a contiguous fp32 [N,C,H,W] tensor, got shape %s strides %s %s" % (
            tuple(y.shape), y.stride(), y.dtype))
    check(lib().s2p_nhwc_to_nchw(dtype_id(x.dtype), ptr(x), xp, c_off, N, C, H, W, ptr(y), int(accumulate), stream()),
          "s2p_nhwc_to_nchw")
    return y


def cast(x, dtype):
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    check(lib().s2p_cast(dtype_id(x.dtype), ptr(x), dtype_id(dtype), ptr(y), x.numel(), stream()), "s2p_cast")
    return y


def act_bwd(dy, y, act, slope=0.2):
    dx = torch.empty_like(dy)
    check(lib().s2p_act_bwd(dtype_id(dy.dtype), ptr(dy), ptr(y), dy.numel(), act, slope, ptr(dx), stream()), "s2p_act_bwd")
    return dx


def scale_(x, scale_dev):
    """x *= scale (fp32 device scalar)."""
    check(lib().s2p_scale(dtype_id(x.dtype), ptr(x), x.numel(), ptr(scale_dev), stream()), "s2p_scale")
    return x


def l1_loss(a, b, scale, loss_out, grad_a=None, accumulate=False):
    """loss_out += scale * sum|a-b|; grad_a (+)= scale*sign(a-b).  a, b contiguous, same numel."""
    check(lib().s2p_l1_loss(dtype_id(a.dtype), ptr(a), ptr(b), a.numel(), scale, ptr(loss_out), ptr(grad_a),
                            int(accumulate), stream()), "s2p_l1_loss")


def l1_loss_multi(jobs):
    """Several L1 terms in one launch.  jobs: list of (a, b, scale, loss_out, grad_a|None) with a, b contiguous NHWC
    activations of one dtype; loss_out += scale * sum|a-b|, grad_a = scale * sign(a-b).  Lists longer than the kernel's job
    table go out in several launches."""
    cap = 16
    for i0 in range(0, len(jobs), cap):
        part = jobs[i0:i0 + cap]
        arr = (_lib.L1Job * len(part))()
        for i, (a, b, scale, loss_out, g) in enumerate(part):
            assert a.dtype == part[0][0].dtype and a.numel() == b.numel()
            arr[i] = _lib.L1Job(ptr(a), ptr(b), ptr(g), a.numel(), scale, ptr(loss_out))
        check(lib().s2p_l1_loss_multi(dtype_id(part[0][0].dtype), arr, len(part), stream()), "s2p_l1_loss_multi")


def hinge_loss(x, count, mode, scale, loss_out, grad_x=None, x_off=0):
    esz = x.element_size()
    xp = x.data_ptr() + x_off * esz
    gp = grad_x.data_ptr() + x_off * esz if grad_x is not None else None
    _ = ptr(x)
    check(lib().s2p_hinge_loss(dtype_id(x.dtype), xp, count, mode, scale, ptr(loss_out), gp, stream()), "s2p_hinge_loss")


def hinge_loss_nhwc(x, mode, scale, loss_out, want_grad=True):
    """Hinge term on an NHWC logit map [B,h,w,pitch] (channel 0 = logit): loss_out += ..., returns the gradient in the
    same layout (padding channels zero) or None."""
    B, h, w, pitch = x.shape
    g = torch.empty_like(x) if want_grad else None
    check(lib().s2p_hinge_loss_strided(dtype_id(x.dtype), ptr(x), B * h * w, pitch, mode, scale, ptr(loss_out), ptr(g), stream()),
          "s2p_hinge_loss_strided")
    return g


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0):
    check(lib().s2p_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, step, grad_scale,
                              stream()), "s2p_adam_step")


def add(a, b, out=None):
    out = out if out is not None else torch.empty_like(a)
    check(lib().s2p_add(dtype_id(a.dtype), ptr(a), ptr(b), ptr(out), a.numel(), stream()), "s2p_add")
    return out


def copy_channels(src, src_off, dst, dst_off, C, accumulate=False, src_rows=None, dst_row0=0, src_row0=0):
    """dst[dst_row0 + p, ..., dst_off:dst_off+C] (+)= src[src_row0 + p, ..., src_off:src_off+C] over `src_rows` images."""
    n_img = src.shape[0] if src_rows is None else src_rows
    ppi = src.shape[1] * src.shape[2]
    sp, dp = src.shape[3], dst.shape[3]
    sptr = src.data_ptr() + src_row0 * ppi * sp * src.element_size()
    dptr = dst.data_ptr() + dst_row0 * ppi * dp * dst.element_size()
    _ = ptr(src), ptr(dst)
    check(lib().s2p_copy_channels(dtype_id(src.dtype), sptr, sp, src_off, dptr, dp, dst_off, C, n_img * ppi,
                                  int(accumulate), stream()), "s2p_copy_channels")
    return dst


def adam_step_dev(p, g, m, v, lr, beta1, beta2, eps, step_dev, grad_scale=1.0):
    """Graph-capturable Adam: `step_dev` is an int32 device tensor incremented on the device."""
    check(lib().s2p_adam_step_dev(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, ptr(step_dev),
                                  grad_scale, stream()), "s2p_adam_step_dev")


def adam_step_dev_part(p, g, m, v, lr, beta1, beta2, eps, step_dev, grad_scale=1.0, tick=True):
    """One optimizer step applied to a RANGE (views of the flat buffers); the first part ticks the device step counter."""
    check(lib().s2p_adam_step_dev_part(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, ptr(step_dev),
                                       grad_scale, int(tick), stream()), "s2p_adam_step_dev_part")


def u8_to_nhwc(x_u8, dtype, pitch):
    """uint8 NHWC frames [N,H,W,C] on the device -> compute-dtype NHWC in [-1,1], zero-padded to `pitch` channels."""
    N, H, W, C = x_u8.shape
    y = torch.empty((N, H, W, pitch), dtype=dtype, device=x_u8.device)
    check(lib().s2p_u8_to_nhwc(dtype_id(dtype), ptr(x_u8), N * H * W, C, ptr(y), pitch, stream()), "s2p_u8_to_nhwc")
    return y


def nhwc_to_u8(x, C, out=None):
    """compute-dtype NHWC in [-1,1] -> uint8 NHWC [N,H,W,C] (the on-disk layout of image_observations*)."""
    N, H, W, xp = x.shape
    y = out if out is not None else torch.empty((N, H, W, C), dtype=torch.uint8, device=x.device)
    check(lib().s2p_nhwc_to_u8(dtype_id(x.dtype), ptr(x), xp, N * H * W, C, ptr(y), stream()), "s2p_nhwc_to_u8")
    return y


def window_gather_u8(pool, table, win, dtype, pitch=None, want_x=True, want_u8=True):
    """Frames of the windows `win` (int64 [B], ids into `table` int32 [n_windows,T]) out of the uint8 frame pool
    [n_slots,H,W,C] (csrc/replay.hip): returns (x, u8) with x [B*T,H,W,pitch] = u8 / 255 in `dtype` (pad channels zero) and
    u8 [B,T,H,W,C]; a form not wanted is None.  The caller has range-checked `win`."""
    n_slots, H, W, C = pool.shape
    T, B = table.shape[1], win.numel()
    if pool.dtype != torch.uint8 or table.dtype != torch.int32 or win.dtype != torch.int64:
        raise TypeError("pool is uint8, table int32 and win int64")
    if not (pool.is_contiguous() and table.is_contiguous() and win.is_contiguous()):
        raise ValueError("pool, table and win must be contiguous")
    pitch = chunk_elems(dtype) if pitch is None else pitch
    x = torch.empty((B * T, H, W, pitch), dtype=dtype, device=pool.device) if want_x else None
    u8 = torch.empty((B, T, H, W, C), dtype=torch.uint8, device=pool.device) if want_u8 else None
    check(lib().s2p_window_gather_u8(dtype_id(dtype), ptr(pool), n_slots, H * W, C, ptr(table), T, ptr(win), B, ptr(x), pitch,
                                     ptr(u8), stream()), "s2p_window_gather_u8")
    return x, u8


def decoded_to_frames(y, C, quantize, x=None, u8_out=None):
    """The decoder's NHWC output y [N,H,W,y_pitch] -> the frames an environment would hand out (csrc/replay.hip, SPEC.md N3o), in one
    launch: x [N,H,W,x_pitch] in y's dtype = the encoder's input (byte / 255 with `quantize`, else the value clamped to [0,1]; pad
    channels zero) and u8_out uint8 [N,H,W,C] = clamp(round(v * 255), 0, 255).  Both are caller-owned and contiguous; one may be
    None.  -> (x, u8_out)."""
    N, H, W, yp = y.shape
    if not y.is_contiguous():
        raise ValueError("y must be contiguous")
    if x is not None and (x.dtype != y.dtype or x.dim() != 4 or tuple(x.shape[:3]) != (N, H, W) or not x.is_contiguous()):
        raise ValueError("x is contiguous [N,H,W,x_pitch] in y's dtype")
    if u8_out is not None and (u8_out.dtype != torch.uint8 or tuple(u8_out.shape) != (N, H, W, C) or not u8_out.is_contiguous()):
        raise ValueError("u8_out is contiguous uint8 [N,H,W,C]")
    check(lib().s2p_decoded_to_frames(dtype_id(y.dtype), ptr(y), yp, N * H * W, C, int(bool(quantize)), ptr(x),
                                      x.shape[3] if x is not None else 0, ptr(u8_out), stream()), "s2p_decoded_to_frames")
    return x, u8_out


def feature_action_push(src, dst, S, F, A, feat, action):
    """dst row n = src row n shifted left by one feature and one action, with feat[n] and action[n] last (csrc/actor.hip,
    `SlacObservation.append`): src / dst fp32 [N,pitch] with pitch a multiple of 4 at least S F + (S - 1) A (pad columns written as
    zeros), feat / action 2-D fp32 views.  src and dst may not overlap: the caller ping-pongs two buffers.  No reset code is set."""
    (sp, ss), (dp, ds), (fp, fs), (ap, as_) = _view2(src), _view2(dst), _view2(feat), _view2(action)
    N = src.shape[0]
    if ss != ds or dst.shape[0] != N or src.shape[1] != ss or dst.shape[1] != ds or feat.shape[0] != N or action.shape[0] != N:
        raise ValueError("src and dst are dense [N,pitch]; feat and action have N rows")
    check(lib().s2p_feature_action_push(sp, dp, ss, N, S, F, A, fp, fs, ap, as_, None, None, stream()), "s2p_feature_action_push")
    return dst


def feature_window_gather(feat, table, win, action_, reward_, done_):
    """Cached encoder features of the windows `win` (int64 [B], ids into `table` int32 [n_windows,T]) out of the feature table `feat`
    fp32 [n_slots,F] (row pitch = its stride), with the windows' actions [n_windows,T-1,A], rewards and terminals [n_windows,T-1,1], in
    one launch (csrc/replay.hip): returns (feature_ [B,T,F], fa, next_fa [B,P] = `create_feature_actions`, action_seq [B,T-1,A],
    action_last [B,A], reward [B,1], terminal [B,1]).  fa / next_fa are `[:, :P]` views of buffers whose row pitch is P rounded up to 4 floats
    (pad columns zero).  The caller has range-checked `win`."""
    if feat.dtype != torch.float32 or table.dtype != torch.int32 or win.dtype != torch.int64 or feat.dim() != 2 or feat.stride(1) != 1:
        raise TypeError("feat is fp32 [n_slots,F] with unit column stride, table int32 and win int64")
    if any(t.dtype != torch.float32 or not t.is_contiguous() for t in (action_, reward_, done_)) or not (table.is_contiguous() and win.is_contiguous()):
        raise ValueError("action_, reward_, done_ are contiguous fp32; table and win are contiguous")
    (n_slots, F), T, B = feat.shape, table.shape[1], win.numel()
    A = 1
    for d in action_.shape[2:]:
        A *= d
    if action_.dim() < 2 or action_.shape[:2] != (table.shape[0], T - 1) or reward_.numel() != table.shape[0] * (T - 1) or done_.numel() != reward_.numel():
        raise ValueError("action_ [n_windows,T-1,A], reward_ and done_ [n_windows,T-1,1] are needed")
    P = (T - 1) * F + (T - 2) * A
    fa_pitch = pad_to(P, 4)
    dev, f = feat.device, torch.float32
    feature_ = torch.empty((B, T, F), dtype=f, device=dev)
    fa, next_fa = torch.empty((B, fa_pitch), dtype=f, device=dev), torch.empty((B, fa_pitch), dtype=f, device=dev)
    action_seq, action_last = torch.empty((B, T - 1) + tuple(action_.shape[2:]), dtype=f, device=dev), torch.empty((B,) + tuple(action_.shape[2:]), dtype=f, device=dev)
    reward, terminal = torch.empty((B, 1), dtype=f, device=dev), torch.empty((B, 1), dtype=f, device=dev)
    check(lib().s2p_feature_window_gather(ptr(feat), n_slots, feat.stride(0), F, ptr(table), T, ptr(win), B, ptr(action_), ptr(reward_),
                                          ptr(done_), A, ptr(feature_), ptr(fa), ptr(next_fa), fa_pitch, ptr(action_seq), ptr(action_last),
                                          A, ptr(reward), ptr(terminal), stream()), "s2p_feature_window_gather")
    return feature_, fa[:, :P], next_fa[:, :P], action_seq, action_last, reward, terminal


def frame_pair_gather(pool, states, idx, size, prev, image=None, state=None):
    """The (frame t, frame t+1, state t+1) triples of the frame numbers `idx` (device int64 [B]) out of the dataset's uint8 frames
    `pool` [n_frames,H,W,C] and fp32 `states` [n_frames,S] in one launch (csrc/replay.hip): prev / image fp32 NCHW [B,C,h,w] =
    u8 / 127.5 - 1 nearest-resized to `size` = (h, w), state [B,S]; image and state may be None.  The outputs are caller-owned and
    contiguous.  The caller has range-checked `idx` (a row out of range comes out as zeros)."""
    n_frames, H, W, C = pool.shape
    (h, w), B = size, idx.numel()
    if pool.dtype != torch.uint8 or states.dtype != torch.float32 or idx.dtype != torch.int64:
        raise TypeError("pool is uint8, states fp32 and idx int64")
    if states.dim() != 2 or states.shape[0] != n_frames:
        raise ValueError("states is [n_frames,S]")
    S = states.shape[1]
    for t, shape in ((prev, (B, C, h, w)), (image, (B, C, h, w)), (state, (B, S))):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError("prev / image are contiguous fp32 [B,C,h,w] and state is contiguous fp32 [B,S]")
    if not (pool.is_contiguous() and states.is_contiguous() and idx.is_contiguous()):
        raise ValueError("pool, states and idx must be contiguous")
    check(lib().s2p_frame_pair_gather(ptr(pool), n_frames, H, W, C, ptr(states), S, ptr(idx), B, h, w, ptr(prev), ptr(image), ptr(state),
                                      stream()), "s2p_frame_pair_gather")


def transition_pack(obs, action, obs_mean, obs_std, out):
    """out[r] = [(obs[r] - obs_mean) / obs_std | action[r] | 0 ...] for every row of a dataset in one launch (csrc/transition.hip):
    the two operations separately rounded in fp32, i.e. numpy's `(obs - mean) / std` bit for bit.  obs [N,obs_dim], action [N,A] and
    are 2-D fp32 views with unit stride in their last dimension (the row pitch is the view's stride); out [N,pitch >= obs_dim + A]
    is dense (every column of it is written) at any alignment; obs_mean / obs_std are contiguous fp32 [obs_dim]."""
    (po, so), (pa, sa), (px, sx) = _view2(obs), _view2(action), _view2(out)
    N, obs_dim, A = obs.shape[0], obs.shape[1], action.shape[1]
    if sx != out.shape[1]:
        raise ValueError("out must be dense: its row pitch is its width")
    if action.shape[0] != N or out.shape[0] != N or obs_mean.shape != (obs_dim,) or obs_std.shape != (obs_dim,):
        raise ValueError("obs [N,obs_dim], action [N,A], out [N,pitch], obs_mean / obs_std [obs_dim] are needed")
    if obs_mean.dtype != torch.float32 or obs_std.dtype != torch.float32 or not (obs_mean.is_contiguous() and obs_std.is_contiguous()):
        raise ValueError("obs_mean and obs_std must be contiguous fp32")
    check(lib().s2p_transition_pack(po, so, pa, sa, ptr(obs_mean), ptr(obs_std), N, obs_dim, A, px, out.shape[1], stream()),
          "s2p_transition_pack")
    return out


# ---- SLAC latent model (csrc/gauss.hip).  Arguments are 2-D fp32 VIEWS (unit stride in the last dimension): the row pitch is the
# view's stride, so a slice of a [B,S+1,288] sequence buffer is read or written in place -- no cat / chunk / stack copy.
def _view2(t):
    if t is None:
        return None, 0
    if t.dim() != 2 or t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError("a 2-D fp32 view with unit stride in its last dimension is needed")
    return ptr(t), (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))


def linear_fwd_into(x, w, bias, N, y, act=ACT_NONE, slope=0.2, add=None):
    """y[:, :] = act(x @ w[:N].T + add + bias); x [M,K] view (K a multiple of 4), w [>=N, w_row], y [M, n_store >= N] view
    (columns >= N written as zeros).  With `add` ([M, >= N] view) the launch is s2p_linear_add_fwd, else s2p_linear_fwd."""
    (xp, xs), (yp, ys) = _view2(x), _view2(y)
    M, K = x.shape
    if add is None:
        check(lib().s2p_linear_fwd(xp, M, K, xs, ptr(w), w.shape[-1], ptr(bias), N, act, slope, yp, ys, y.shape[1], stream()),
              "s2p_linear_fwd")
    else:
        ap, as_ = _view2(add)
        check(lib().s2p_linear_add_fwd(xp, M, K, xs, ptr(w), w.shape[-1], ptr(bias), N, ap, as_, act, slope, yp, ys, y.shape[1],
                                       stream()), "s2p_linear_add_fwd")
    return y


def linear_add_bwd(dy, y, N, act, slope=0.2, x=None, k_real=0, dw=None, db=None, w_bwd=None, dx=None, accumulate=False, dadd=None):
    """Backward of linear_fwd_into given dy ([M, >= N] view) and the layer output y (None with ACT_NONE); dpre = dy * act'(y).
    dw [N, k_real] += dpre.T @ x, db += dpre.sum(0) (needs x);  dx (view [M, K]) = or += dpre @ w (needs w_bwd [K, >= N]);
    dadd (view) = dpre.  Every output is optional."""
    (dyp, dys), (yp, ys), (xp, xs), (dxp, dxs), (dap, das) = _view2(dy), _view2(y), _view2(x), _view2(dx), _view2(dadd)
    M = dy.shape[0]
    K = x.shape[1] if x is not None else dx.shape[1] if dx is not None else 4
    check(lib().s2p_linear_add_bwd(xp, xs, dyp, dys, yp, ys, M, K, k_real, N, ptr(w_bwd), w_bwd.shape[-1] if w_bwd is not None else 0,
                                   act, slope, ptr(dw), dw.shape[-1] if dw is not None else 0, ptr(db), dxp, dxs, int(accumulate),
                                   dap, das, stream()), "s2p_linear_add_bwd")
    return dx


def gauss_head_fwd(raw, D, eps=None, mean=None, std=None, z=None, z2=None):
    """raw [M, >= 2D] = [mean | raw_std] -> mean, std = softplus + 1e-5, z = z2 = mean + eps * std, each into its own view."""
    views = [_view2(t) for t in (raw, eps, mean, std, z, z2)]
    (rp, rs), (ep, es), (mp, ms), (sp, ss), (zp, zs), (z2p, z2s) = views
    check(lib().s2p_gauss_head_fwd(rp, rs, raw.shape[0], D, ep, es, mp, ms, sp, ss, zp, zs, z2p, z2s, stream()), "s2p_gauss_head_fwd")


def chain_mlp(pk, group=0, k1=None):
    """The s2p_chain_mlp of a Gaussian.packed() dict; `group`: which first-layer column group is the chain's; `k1`: the chain reads
    only the first k1 columns of that group, in place (z1_prior in the prior chain: its action columns are hoisted)."""
    w1, _, k = pk["g1"][group]
    return _lib.ChainMlp(ptr(w1), ptr(pk["b1"]), ptr(pk["w2"]), ptr(pk["b2"]), ptr(pk["w3"]), ptr(pk["b3"]), k if k1 is None else k1,
                         w1.shape[1])


def chain_mlp_bf16(pk):
    """The s2p_chain_mlp_bf16 of a Gaussian.packed_bf16() dict."""
    w1 = pk["w1"]
    for w in (w1, pk["w2"], pk["w3"]):
        if w.dtype != torch.bfloat16 or not w.is_contiguous():
            raise ValueError("the weight operands of a bf16 chain are contiguous torch.bfloat16 packs")
    return _lib.ChainMlpBf16(ptr(w1), ptr(pk["b1"]), ptr(pk["w2"]), ptr(pk["b2"]), ptr(pk["w3"]), ptr(pk["b3"]), w1.shape[1], w1.shape[1])


def _chain_views(B, T, *ts):
    for t in ts:
        if t.dtype != torch.float32 or t.shape[:2] != (B, T) or t.stride(2) != 1 or (B > 1 and T > 0 and t.stride(0) != T * t.stride(1)):
            raise ValueError("[B, T, C] fp32 views whose rows (b, t) are evenly pitched are needed")


def _chain_operands(src, eps, mlps, n_mlps, mean, std, z, terms=(), steps=0, more=(), mlp_type=_lib.ChainMlp):
    """What the chain wrappers share.  Checks eps, mean, std, z and `more` as [B, T, C] views (_chain_views) and the hoisted
    `terms` as contiguous fp32 [steps*B, 256] (None passes: the entry point says when a term may be absent).  -> the (pointer, pitch)
    of the 2-D view `src`, the array of `n_mlps` ChainMlp, and the argument tail of all three entry points, mean .. stream."""
    B, T = eps.shape[:2]
    _chain_views(B, T, eps, mean, std, z, *more)
    for r in terms:
        if r is not None and (not r.is_contiguous() or r.dtype != torch.float32 or r.shape != (steps * B, 256)):
            raise ValueError("the hoisted terms are contiguous fp32 [%d*B, 256]" % steps)
    tail = (ptr(mean), mean.stride(1), ptr(std), std.stride(1), ptr(z), z.stride(1), B, T, stream())
    return _view2(src), (mlp_type * n_mlps)(*mlps), tail


def prior_chain_fwd(z2_0, rc, rb, eps, mlps, mean, std, z):
    """The whole open-loop prior rollout in one launch (s2p_prior_chain_fwd).  z2_0: a [B, 256] view (a column slice of z(0) is read
    in place); rc, rb [H*B, 256] contiguous, time-major; eps, mean, std, z: [B, H, C] views as for posterior_chain_fwd; mlps: the
    chain_mlp() structs of z1_prior (k1 = 256) and z2_prior."""
    (zp, zs), arr, tail = _chain_operands(z2_0, eps, mlps, 2, mean, std, z, terms=(rc, rb), steps=eps.shape[1])
    check(lib().s2p_prior_chain_fwd(zp, zs, ptr(rc), ptr(rb), ptr(eps), eps.stride(1), arr, *tail), "s2p_prior_chain_fwd")


def prior_chain_fwd_bf16(z2_0, rc, rb, eps, mlps, mean, std, z):
    """prior_chain_fwd in bf16 compute (s2p_prior_chain_fwd_bf16; SPEC.md N3m): the same fp32 tensors, mlps: the chain_mlp_bf16()
    structs of z1_prior (its z2-column pack) and z2_prior."""
    (zp, zs), arr, tail = _chain_operands(z2_0, eps, mlps, 2, mean, std, z, terms=(rc, rb), steps=eps.shape[1], mlp_type=_lib.ChainMlpBf16)
    check(lib().s2p_prior_chain_fwd_bf16(zp, zs, ptr(rc), ptr(rb), ptr(eps), eps.stride(1), arr, *tail), "s2p_prior_chain_fwd_bf16")


def _policy_built(policy):
    """ValueError for a policy outside the shapes s2p_imagine_chain_fwd and s2p_imagine_chain_fwd_bf16 are built for."""
    hs = policy.hidden_sizes
    if policy.obs_dim != 288 or len(hs) != 2 or hs[0] != hs[1] or hs[0] % 128 or not 128 <= hs[0] <= 1024 or not 1 <= policy.action_dim <= 8:
        raise ValueError("the fused imagination chain is built for obs_dim 288, two hidden layers of one width W (a multiple of 128, "
                         "128 <= W <= 1024) and 1 <= action_dim <= 8; got obs_dim %d, hidden_sizes %s, action_dim %d"
                         % (policy.obs_dim, hs, policy.action_dim))


def policy_mlp(policy):
    """The s2p_policy_mlp of a two-hidden-layer TanhGaussianPolicy: its packed layers in place (the last layer's first A rows are
    `last_fc`).  ValueError for a shape outside what s2p_imagine_chain_fwd is built for."""
    _policy_built(policy)
    pk, hs = policy.packed, policy.hidden_sizes
    w, b = [pk.w(policy.flat, li) for li in range(3)], [pk.b(policy.flat, li) for li in range(3)]
    return _lib.PolicyMlp(ptr(w[0]), ptr(b[0]), ptr(w[1]), ptr(b[1]), ptr(w[2]), ptr(b[2]), w[0].shape[1], hs[0])


def policy_mlp_bf16(policy):
    """The s2p_policy_mlp_bf16 of a two-hidden-layer TanhGaussianPolicy: the weights of its `packed_bf16()`, the fp32 biases in place.
    ValueError for a shape outside what s2p_imagine_chain_fwd_bf16 is built for (those of policy_mlp)."""
    _policy_built(policy)
    pk = policy.packed_bf16()
    w, b = pk["w"], pk["b"]
    for t in w:
        if t.dtype != torch.bfloat16 or not t.is_contiguous():
            raise ValueError("the weight operands of a bf16 chain are contiguous torch.bfloat16 packs")
    return _lib.PolicyMlpBf16(ptr(w[0]), ptr(b[0]), ptr(w[1]), ptr(b[1]), ptr(w[2]), ptr(b[2]), w[0].shape[1], policy.hidden_sizes[0])


def imagine_chain_fwd(z0, eps, mlps, wc, wb, A, policy, act, mean, std, z):
    """The whole closed-loop rollout in one launch (s2p_imagine_chain_fwd).  z0: a [B, 288] view; eps, act, mean, std, z: [B, H, C]
    views as for posterior_chain_fwd; mlps: the chain_mlp() structs of z1_prior (k1 = 256) and z2_prior; wc, wb: their action
    columns [256][pad4(A)]; policy: a policy_mlp() struct."""
    (zp, zs), arr, tail = _chain_operands(z0, eps, mlps, 2, mean, std, z, more=(act,))
    check(lib().s2p_imagine_chain_fwd(zp, zs, ptr(eps), eps.stride(1), arr, ptr(wc), wc.shape[1], ptr(wb), wb.shape[1], A,
                                      ctypes.byref(policy), ptr(act), act.stride(1), *tail), "s2p_imagine_chain_fwd")


def imagine_chain_fwd_bf16(z0, eps, mlps, wc, wb, A, policy, act, mean, std, z):
    """imagine_chain_fwd in bf16 compute (s2p_imagine_chain_fwd_bf16; SPEC.md N3n): the same fp32 tensors (wc, wb included), mlps: the
    chain_mlp_bf16() structs of z1_prior (its z2-column pack) and z2_prior; policy: a policy_mlp_bf16() struct."""
    (zp, zs), arr, tail = _chain_operands(z0, eps, mlps, 2, mean, std, z, more=(act,), mlp_type=_lib.ChainMlpBf16)
    check(lib().s2p_imagine_chain_fwd_bf16(zp, zs, ptr(eps), eps.stride(1), arr, ptr(wc), wc.shape[1], ptr(wb), wb.shape[1], A,
                                           ctypes.byref(policy), ptr(act), act.stride(1), *tail), "s2p_imagine_chain_fwd_bf16")


def posterior_chain_fwd(feat0, ra, rb, eps, mlps, mean, std, z):
    """The whole no-grad posterior chain in one launch (s2p_posterior_chain_fwd).  feat0: the [B, 256] view feat[:, 0]; ra, rb
    [(T-1)*B, 256] contiguous (None when T == 1); eps, mean, std, z: [B, T, C] views with unit stride in C and stride(0) =
    T * stride(1) (a slice of a wider [B, T, W] buffer is written in place); mlps: four chain_mlp() structs."""
    (fp, fs), arr, tail = _chain_operands(feat0, eps, mlps, 4, mean, std, z, terms=(ra, rb), steps=eps.shape[1] - 1)
    check(lib().s2p_posterior_chain_fwd(fp, fs, ptr(ra), ptr(rb), ptr(eps), eps.stride(1), arr, *tail), "s2p_posterior_chain_fwd")


def posterior_chain_fwd_bf16(feat0, ra, rb, eps, mlps, mean, std, z):
    """posterior_chain_fwd in bf16 compute (s2p_posterior_chain_fwd_bf16; SPEC.md N3m): the same fp32 tensors, mlps: four
    chain_mlp_bf16() structs."""
    (fp, fs), arr, tail = _chain_operands(feat0, eps, mlps, 4, mean, std, z, terms=(ra, rb), steps=eps.shape[1] - 1,
                                          mlp_type=_lib.ChainMlpBf16)
    check(lib().s2p_posterior_chain_fwd_bf16(fp, fs, ptr(ra), ptr(rb), ptr(eps), eps.stride(1), arr, *tail), "s2p_posterior_chain_fwd_bf16")


def _dense(ts):
    for t in ts:
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("the chain state and its gradients are contiguous fp32 buffers")
    return [ptr(t) for t in ts]


def chain_state(a0, b0, sv=None):
    """The s2p_chain_state of what _PosteriorFn keeps: a0, b0 = (h1, h2, raw) of the two t = 0 heads, sv = (h1a, h2a, rawa, h1b,
    h2b, rawb, xz), time-major (None when T == 1: the chain has no step)."""
    return _lib.ChainState(*(_dense(tuple(a0) + tuple(b0)) + (_dense(sv) if sv is not None else [None] * 7)))


def posterior_chain_fwd_save(feat0, ra, rb, eps, mlps, mean, std, z, state):
    """posterior_chain_fwd that also fills `state` (a chain_state()) with everything the backward reads: one launch
    (s2p_posterior_chain_fwd_save), bitwise the per-layer path."""
    (fp, fs), arr, tail = _chain_operands(feat0, eps, mlps, 4, mean, std, z, terms=(ra, rb), steps=eps.shape[1] - 1)
    check(lib().s2p_posterior_chain_fwd_save(fp, fs, ptr(ra), ptr(rb), ptr(eps), eps.stride(1), arr, *tail[:6], ctypes.byref(state),
                                             *tail[6:]), "s2p_posterior_chain_fwd_save")


def chain_mlp_bwd(pk):
    """The s2p_chain_mlp_bwd of a Gaussian.packed() dict: the transposes of the chain columns of the first layer, of w2 and of w3."""
    _, w1t, k = pk["g1"][0]
    return _lib.ChainMlpBwd(ptr(w1t), ptr(pk["w2t"]), ptr(pk["w3t"]), k, w1t.shape[1])


def posterior_chain_bwd(eps, dmean, dstd, dz, mlps, state, grads):
    """The steps t = T-1 .. 1 of the posterior chain's backward in one launch (s2p_posterior_chain_bwd).  eps, dz [B, T, 288],
    dmean, dstd [B, T, 32] views as for posterior_chain_fwd; mlps: the chain_mlp_bwd() of z1_posterior and z2_prior; state: a
    chain_state(); grads = (drawa, dh2a, dh1a, drawb, dh2b, dh1b, dxz), contiguous and time-major: all of them are written."""
    B, T = eps.shape[:2]
    _chain_views(B, T, eps, dmean, dstd, dz)
    check(lib().s2p_posterior_chain_bwd(ptr(eps), eps.stride(1), ptr(dmean), dmean.stride(1), ptr(dstd), dstd.stride(1), ptr(dz),
                                        dz.stride(1), (_lib.ChainMlpBwd * 2)(*mlps), ctypes.byref(state),
                                        ctypes.byref(_lib.ChainGrads(*_dense(grads))), B, T, stream()), "s2p_posterior_chain_bwd")


def posterior_chain_fwd_save_bf16(feat0, ra, rb, eps, mlps, mean, std, z, state):
    """posterior_chain_fwd_save in bf16 compute (s2p_posterior_chain_fwd_save_bf16; SPEC.md N3p): mean, std, z bitwise those of
    posterior_chain_fwd_bf16, `state` filled with the unrounded fp32 values; mlps: four chain_mlp_bf16() structs."""
    (fp, fs), arr, tail = _chain_operands(feat0, eps, mlps, 4, mean, std, z, terms=(ra, rb), steps=eps.shape[1] - 1,
                                          mlp_type=_lib.ChainMlpBf16)
    check(lib().s2p_posterior_chain_fwd_save_bf16(fp, fs, ptr(ra), ptr(rb), ptr(eps), eps.stride(1), arr, *tail[:6], ctypes.byref(state),
                                                  *tail[6:]), "s2p_posterior_chain_fwd_save_bf16")


def chain_mlp_bwd_bf16(pk):
    """The s2p_chain_mlp_bwd_bf16 of a Gaussian.packed_bf16_grad() dict: the transposes of its three bf16 packs."""
    w1t = pk["w1t"]
    for w in (w1t, pk["w2t"], pk["w3t"]):
        if w.dtype != torch.bfloat16 or not w.is_contiguous():
            raise ValueError("the weight operands of a bf16 chain are contiguous torch.bfloat16 packs")
    return _lib.ChainMlpBwdBf16(ptr(w1t), ptr(pk["w2t"]), ptr(pk["w3t"]), w1t.shape[0], w1t.shape[1])


def posterior_chain_bwd_bf16(eps, dmean, dstd, dz, mlps, state, grads):
    """posterior_chain_bwd in bf16 compute (s2p_posterior_chain_bwd_bf16; SPEC.md N3p): the same fp32 tensors, mlps: the
    chain_mlp_bwd_bf16() of z1_posterior and z2_prior."""
    B, T = eps.shape[:2]
    _chain_views(B, T, eps, dmean, dstd, dz)
    check(lib().s2p_posterior_chain_bwd_bf16(ptr(eps), eps.stride(1), ptr(dmean), dmean.stride(1), ptr(dstd), dstd.stride(1), ptr(dz),
                                             dz.stride(1), (_lib.ChainMlpBwdBf16 * 2)(*mlps), ctypes.byref(state),
                                             ctypes.byref(_lib.ChainGrads(*_dense(grads))), B, T, stream()),
          "s2p_posterior_chain_bwd_bf16")


def chain_pack_bf16(jobs):
    """bf16 packs of fp32 matrices in ONE launch (s2p_chain_pack_bf16).  jobs: (src, dst, dst_t) with src a 2-D fp32 view with unit
    stride in its last dimension (a column slice of a wider matrix is read in place), dst [rows, >= cols] and dst_t [cols, >= rows]
    torch.bfloat16 views of the same kind, either None: dst = src rounded to nearest even, dst_t its transpose.  Columns past the
    shape of src are not written."""
    arr = (_lib.Bf16PackJob * len(jobs))()
    for job, (src, dst, dst_t) in zip(arr, jobs):
        rows, cols = src.shape
        for t, shape in ((dst, (rows, cols)), (dst_t, (cols, rows))):
            if t is not None and (t.dim() != 2 or t.dtype != torch.bfloat16 or tuple(t.shape) != shape or (shape[1] > 1 and t.stride(1) != 1)):
                raise ValueError("a pack is a 2-D torch.bfloat16 view of the shape of src (dst) or of its transpose (dst_t)")
        pitch = lambda t: 0 if t is None else t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])
        job.src, job.src_pitch = _view2(src)
        job.dst, job.dst_t, job.rows, job.cols, job.dst_pitch, job.dst_t_pitch = ptr(dst), ptr(dst_t), rows, cols, pitch(dst), pitch(dst_t)
    check(lib().s2p_chain_pack_bf16(arr, len(jobs), stream()), "s2p_chain_pack_bf16")


def gauss_head_bwd(raw, D, draw, eps=None, dmean=None, dstd=None, dz=None, dz2=None):
    """draw[:, :2D] = [dmean + dz + dz2 | (dstd + (dz + dz2) * eps) * sigmoid(raw_std)]."""
    views = [_view2(t) for t in (raw, eps, dmean, dstd, dz, dz2, draw)]
    (rp, rs), (ep, es), (mp, ms), (sp, ss), (zp, zs), (z2p, z2s), (dp, ds) = views
    check(lib().s2p_gauss_head_bwd(rp, rs, raw.shape[0], D, ep, es, mp, ms, sp, ss, zp, zs, z2p, z2s, dp, ds, stream()),
          "s2p_gauss_head_bwd")


def gauss_kl(mu_p, std_p, mu_q, std_q, B, T, scale, loss, const_first=True, want_grad=True):
    """loss[0] += scale * sum KL(p || q); p [B*T, D] rows (b, t), q [B*(T-1), D] rows (b, t-1) (t = 0: N(0, I)) or [B*T, D].
    Returns (dmu_p, dstd_p, dmu_q, dstd_q), already scaled, or None."""
    D = mu_p.shape[1]
    g = [torch.empty_like(t) for t in (mu_p, std_p, mu_q, std_q)] if want_grad else [None] * 4
    check(lib().s2p_gauss_kl(ptr(mu_p), ptr(std_p), mu_p.stride(0), ptr(mu_q), ptr(std_q), mu_q.stride(0) if mu_q is not None else 0, B, T,
                             D, int(const_first), scale, ptr(loss), ptr(g[0]), ptr(g[1]), D, ptr(g[2]), ptr(g[3]), D, stream()),
          "s2p_gauss_kl")
    return g if want_grad else None


def gauss_ll(mu, std, target, done, scale, loss, want_grad=True):
    """loss[0] += scale * sum (1 - done) * nll(target | mu, std); mu, std [n, 1] views, target / done contiguous [n]."""
    n = mu.shape[0]
    dmu = torch.empty(n, dtype=torch.float32, device=mu.device) if want_grad else None
    dstd = torch.empty(n, dtype=torch.float32, device=mu.device) if want_grad else None
    check(lib().s2p_gauss_ll(ptr(mu), mu.stride(0), ptr(std), std.stride(0), ptr(target), ptr(done), n, scale, ptr(loss), ptr(dmu),
                             ptr(dstd), stream()), "s2p_gauss_ll")
    return dmu, dstd


def gauss_ll_image(mu, target, C, sigma, scale, loss, want_grad=True):
    """mu: NHWC [N,H,W,pitch] (compute dtype); target: fp32 NCHW [N,C,H,W] or uint8 NHWC [N,H,W,C] (read as u8 / 255).
    loss[0] += scale * sum nll; returns dmu (layout and dtype of mu, padded channels zero) or None."""
    N, H, W, pitch = mu.shape
    u8 = target.dtype == torch.uint8
    if not u8 and target.dtype != torch.float32:
        raise TypeError("the image target is fp32 NCHW or uint8 NHWC")
    if target.numel() != N * C * H * W or not target.is_contiguous() or not mu.is_contiguous():
        raise ValueError("image likelihood: target / mu shape or layout")
    dmu = torch.empty_like(mu) if want_grad else None
    check(lib().s2p_gauss_ll_image(dtype_id(mu.dtype), ptr(mu), pitch, ptr(target), int(u8), N, C, H * W, sigma, scale, ptr(loss),
                                   ptr(dmu), stream()), "s2p_gauss_ll_image")
    return dmu
