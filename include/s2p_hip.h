/* libs2p_hip.so -- C ABI of the MI355X (gfx950) S2P hot path.
 *
 * Drop-in boundary.  The reference checkout ships NO native code
 * and NO generator source, so "the reference interface each entry
 * replaces" is the PyTorch op the SPADE-lineage generator/discriminator would call from
 * Python (README.md:72-75 names the lineage; README.md:33,59 name the CLI that reaches
 * them).  Each entry point below cites that torch op; INTEGRATION.md shows the ctypes
 * stub a maintainer adds.
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer is DEVICE memory owned by the caller
 *     (the library never allocates, frees or retains device memory);
 *   - every launch goes to the `stream` argument (a hipStream_t passed as void*), no
 *     implicit synchronisation, safe under hipGraph capture;
 *   - return 0 on success, negative on error; s2p_last_error() gives the message
 *     (thread-local); no C++ exception crosses the ABI;
 *   - activations are NHWC ("channels-last") in `dtype` (S2P_F32 or S2P_BF16); weights
 *     are "packed" [group][Cout][tap][Cin_pad] in the same dtype (s2p_pack_weights);
 *     master weights / gradients / optimizer state are fp32.
 */
#ifndef S2P_HIP_H
#define S2P_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: only the entry points declared here are exported */
#pragma GCC visibility push(default)

#define S2P_VERSION 125

enum { S2P_F32 = 0, S2P_BF16 = 1 };
enum { S2P_ACT_NONE = 0, S2P_ACT_RELU = 1, S2P_ACT_LRELU = 2, S2P_ACT_TANH = 3, S2P_ACT_SWISH = 4 };
/* epilogue modes of the conv family */
enum { S2P_EPI_STORE = 0,       /* y = act(conv + bias)                                   */
       S2P_EPI_ADD = 1,         /* y = act(conv + bias) + aux          (residual add)     */
       S2P_EPI_MUL_ACTGRAD = 2  /* y = conv * act'(aux)  (fused backward of the producer's
                                   ReLU / LeakyReLU; aux = that producer's OUTPUT)        */ };

/* One 2-D convolution problem, forward orientation.  torch equivalents:
 *   transposed == 0 : F.conv2d(x, w, b, stride, padding)            (pad mode zeros/reflect)
 *   transposed == 1 : F.conv_transpose2d(x, w, None, stride, padding, output_padding)
 * x : [N, H, W, x_pitch>=groups*Cin]   y : [N, Ho, Wo, y_pitch>=groups*Cout]
 * Cin must be a multiple of 16/sizeof(dtype) elements (pad thin inputs with zeros). */
typedef struct {
  int32_t dtype;
  int32_t N, H, W, Cin, x_pitch;
  int32_t Ho, Wo, Cout, y_pitch;
  int32_t KH, KW, stride, pad;
  int32_t transposed;
  int32_t reflect;
  int32_t groups;       /* >=1: batched independent convs; group g reads channels
                           [g*x_gstride, +Cin) and writes [g*y_gstride, +Cout).  A stride
                           >= the pitch makes that side group-major: [groups][N][H][W][pitch]
                           (whole tensors `stride` elements apart), e.g. the 12 gamma|beta
                           planes of the generator, one 1-KB-row tensor per norm            */
  int32_t x_gstride, y_gstride;
  int32_t cin_real;     /* un-padded input channels (0: unknown = Cin).  Lets the thin-input kernels skip zero
                           padding channels: a 7x7 conv with <= 4 real input channels (the generator's stem)
                           contracts 4 channels per tap instead of 8                                        */
} s2p_conv_desc;

int s2p_version(void);
const char* s2p_last_error(void);

/* ---- conv family (replaces torch.nn.functional.conv2d / conv_transpose2d and their
 *      autograd backward: cudnn_convolution_backward_input / _weight) ---------------- */
/* w_fwd : packed [groups][Cout][KH*KW][Cin]      (for transposed==1 too)               */
/* act == S2P_ACT_LRELU: slope must be <= 1 in every FORWARD entry point of this header (conv, fused conv + norm,
 * InstanceNorm forward / apply): the kernels evaluate  max(v, v * slope)  -- one multiply and one maximum; a larger slope is
 * rejected with an error (s2p_last_error).  The reference uses 0.2 everywhere (LeakyReLU(0.2): SPEC.md).                    */
int s2p_conv2d_fwd(const s2p_conv_desc* d, const void* x, const void* w_fwd, const float* bias,
                   const void* aux, void* y, int act, float slope, int epi, void* stream);
/* dx = d(loss)/dx.  w_bwd : packed [groups][Cin][KH*KW][Cout_pad] (the transpose of w_fwd).
 * dy has pitch y_pitch and channel count Cout (must itself satisfy the chunk multiple).
 * epi / aux as above (aux has the layout of dx); with S2P_EPI_MUL_ACTGRAD the result is
 * multiplied by aux_act'(aux) (aux = OUTPUT of the activation that produced x); an optional
 * aux2 (layout of dx) is added first: dx = (dgrad + aux2) * aux_act'(aux)  -- the gradient
 * arriving at x from a second consumer (e.g. a feature-matching / perceptual loss tap).
 * Reflect-padded convs: dx is produced on the PADDED grid [N,H+2p,W+2p,x_pitch]; fold it
 * with s2p_reflect_pad_bwd.                                                             */
int s2p_conv2d_dgrad(const s2p_conv_desc* d, const void* dy, const void* w_bwd,
                     const void* aux, const void* aux2, void* dx, int epi, int aux_act, float slope,
                     void* stream);
/* s2p_conv2d_fwd / s2p_conv2d_dgrad with a caller-owned device scratch of at least s2p_conv2d_{fwd,dgrad}_workspace(...)
 * bytes (0 for most shapes).  bf16 launches that cannot fill the chip (<= 160 workgroups: small maps with a long K, e.g.
 * the PatchGAN 256->512 layers on 7x7 / 12x12 maps) then split K over the idle CUs: every slice stores an fp32 partial
 * tile to the scratch and a second kernel applies bias / activation / epilogue to their fixed-order sum (no atomics;
 * bitwise reproducible).  A NULL / short workspace runs the unsplit kernels: same result up to fp32 summation order.   */
size_t s2p_conv2d_fwd_workspace(const s2p_conv_desc* d, int epi);
int s2p_conv2d_fwd_ws(const s2p_conv_desc* d, const void* x, const void* w_fwd, const float* bias,
                      const void* aux, void* y, int act, float slope, int epi, void* workspace,
                      size_t workspace_bytes, void* stream);
size_t s2p_conv2d_dgrad_workspace(const s2p_conv_desc* d);
int s2p_conv2d_dgrad_ws(const s2p_conv_desc* d, const void* dy, const void* w_bwd,
                        const void* aux, const void* aux2, void* dx, int epi, int aux_act, float slope,
                        void* workspace, size_t workspace_bytes, void* stream);
/* conv -> InstanceNorm -> MAT / SPADE modulation -> activation (replaces F.conv2d followed by F.instance_norm and the
 * `normalized * (1 + gamma) + beta` + LeakyReLU of the SPADE-lineage ResBlk: s2p_conv2d_fwd_ws + s2p_in_norm_fwd):
 *   y      = conv(x, w) + bias  [+ aux with epi == S2P_EPI_ADD]                 (kept: the backward needs it)
 *   y_mat  = act(IN(y) * (1 + g_img + g_st) + b_img + b_st),  stats = the statistics of y (s2p_in_stats format)
 * For bf16 3x3 stride-1 pad-1 convs on planes of 321..448 pixels (<= 21 x 21) with Cin, Cout multiples of 64 this is ONE
 * launch: the workgroup that owns an (image, 64-channel) plane of y normalises it in its epilogue (csrc/conv_plane.hip);
 * so is it, without gamma / beta maps (plain InstanceNorm: gb_img == NULL), for the PatchGAN 4x4 stride-1 layers on planes
 * of up to 192 pixels (csrc/conv_planeg.hip).  Other shapes run the two calls above back to back
 * (s2p_conv2d_mat_is_fused tells which).  groups must be 1; act: none / relu / lrelu.
 * y may be NULL where the launch is fused (s2p_conv2d_mat_is_fused): the conv output itself is then not written -- a forward
 * pass that keeps nothing for a backward only needs y_mat.  Where the launch is not fused a call with y == NULL is refused
 * (non-zero, s2p_last_error) before anything is launched.                                                                */
int s2p_conv2d_fwd_mat(const s2p_conv_desc* d, const void* x, const void* w_fwd, const float* bias, const void* aux,
                       void* y, int epi, const void* gb_img, int gb_pitch, const float* gb_st, int gb_st_pitch,
                       int act, float slope, float eps, void* y_mat, int y_mat_pitch, float* stats, void* workspace,
                       size_t workspace_bytes, void* stream);
/* The backward counterpart: dgrad of a conv whose INPUT was the output of a MAT norm, followed by that norm's backward
 * (s2p_conv2d_dgrad_ws + s2p_in_norm_bwd_res).  d describes the conv (forward orientation); dy = dL/d(conv output);
 * xn / stats / gb_img / gb_st / act: the norm's input, statistics and modulation as in s2p_in_norm_bwd; outputs
 * dxn = dL/d(xn) (+ res), dgb_img, dgb_st as there.  aux (may be NULL; layout of d_mid) is a second gradient arriving at
 * the norm's OUTPUT (a feature-matching tap on the activation): it is added to the dgrad result before the norm backward.
 * Under the conditions of s2p_conv2d_fwd_mat (on the dgrad: Cout is the contraction, Cin the produced channels) this is ONE
 * launch and dL/d(norm output) never reaches HBM (d_mid and sums may then be NULL: s2p_conv2d_mat_is_fused); otherwise it
 * is written to d_mid ([N,H,W,x_pitch]) and the norm backward runs as its own launch(es) (needs `sums`:
 * s2p_in_bwd_sums_floats(N, H*W, Cin) floats).  A call without d_mid or sums that is not one launch FOR ITS ARGUMENTS (with
 * aux the 3x3 family is two launches, which s2p_conv2d_mat_is_fused -- it has no aux argument -- cannot tell) is refused
 * (non-zero, s2p_last_error) before anything is launched.                                                               */
int s2p_conv2d_dgrad_mat(const s2p_conv_desc* d, const void* dy, const void* w_bwd, void* d_mid, const void* aux, const void* xn,
                         int xn_pitch, const float* stats, const void* gb_img, int gb_pitch, const float* gb_st,
                         int gb_st_pitch, int act, float slope, float eps, float* sums, void* dxn, int dxn_pitch,
                         void* dgb_img, int dgb_pitch, float* dgb_st, int dgb_st_pitch, const void* res, int res_pitch,
                         void* workspace, size_t workspace_bytes, void* stream);
/* 1 when s2p_conv2d_fwd_mat (dgrad == 0) / s2p_conv2d_dgrad_mat (dgrad == 1) run this problem as ONE fused launch (no d_mid / sums
 * scratch needed), 0 when they fall back to two calls.  has_gb: gamma / beta image maps are passed.                    */
int s2p_conv2d_mat_is_fused(const s2p_conv_desc* d, int dgrad, int has_gb);
/* Which kernel family s2p_conv2d_fwd_ws (dgrad == 0) / s2p_conv2d_dgrad_ws (dgrad == 1) run this problem on, with
 * epi == S2P_EPI_STORE and no fused norm: the S2P_CONV_PATH_* id of the plan's first launch; for S2P_CONV_PATH_HALO the
 * kernel variant (S2P_HALO_*) rides in bits 8 and up, for S2P_CONV_PATH_THIN the kernel behind it
 * (S2P_THIN_*).  has_workspace: the caller passes a scratch of the size the workspace query asks for (0: none).  A dry
 * run of the dispatcher -- nothing is dereferenced or launched; -1 for a descriptor the conv entry points refuse.  The
 * query plans with S2P_ACT_NONE: a call with S2P_ACT_SWISH keeps the row-streaming kernel out (it then runs the tiled or
 * the lanes-per-pixel kernel), which the query does not tell.  For tests and tools: which path a shape takes is not part
 * of the contract. */
enum { S2P_CONV_PATH_THIN = 0, S2P_CONV_PATH_THIN4 = 1, S2P_CONV_PATH_THIN_CIN = 2, S2P_CONV_PATH_THIN_ROWS = 3,
       S2P_CONV_PATH_PLANE = 4, S2P_CONV_PATH_PLANEG = 5, S2P_CONV_PATH_HALO = 6, S2P_CONV_PATH_SPLITK = 7,
       S2P_CONV_PATH_DMA = 8, S2P_CONV_PATH_PHASES = 9, S2P_CONV_PATH_GENERIC = 10 };
enum { S2P_HALO_S9_176_PIPE = 0, S2P_HALO_S9_176 = 1, S2P_HALO_S9_320 = 2, S2P_HALO_R_176 = 3, S2P_HALO_R_320 = 4 };
enum { S2P_THIN_LANES = 0, S2P_THIN_TILED, S2P_THIN_ROWS, S2P_THIN_HEAD, S2P_THIN_HEAD_MFMA };
int s2p_conv2d_path(const s2p_conv_desc* d, int dgrad, int has_workspace);
/* dw (fp32) [groups][Cout][KH*KW][Cin_real] for transposed==0,
 *           [groups][Cin][KH*KW][Cout_real] for transposed==1  (= channels-last physical
 * layout of the torch parameter).  dw is ACCUMULATED into (caller zeroes it);
 * dw_gstride = elements between groups.  cin_real/cout_real: un-padded channel counts.
 * db (may be NULL; transposed==0 only): fp32 [groups][Cout] bias gradient, ACCUMULATED into,
 * fused into the same pass over dy.                                                     */
int s2p_conv2d_wgrad(const s2p_conv_desc* d, const void* x, const void* dy, float* dw, float* db,
                     int cin_real, int cout_real, int64_t dw_gstride, int splitk, void* stream);
/* The same with a caller-owned device scratch of at least s2p_conv2d_wgrad_workspace(...) bytes: the K-split units of the
 * bf16 kernels (and the workgroups of the thin tiled kernel, and the pixel blocks of a separate bias-gradient pass) then
 * store partial tiles / sums there and a second kernel adds them to dw / db in a fixed order -- no atomics, bitwise
 * reproducible (s2p_conv2d_wgrad itself, and a NULL / short workspace, accumulate with fp32 atomics).                    */
size_t s2p_conv2d_wgrad_workspace(const s2p_conv_desc* d, int cin_real, int cout_real);
int s2p_conv2d_wgrad_ws(const s2p_conv_desc* d, const void* x, const void* dy, float* dw, float* db,
                        int cin_real, int cout_real, int64_t dw_gstride, int splitk, void* workspace,
                        size_t workspace_bytes, void* stream);
/* Scratch size with which s2p_conv2d_wgrad_ws is free of atomics for fp32 tensors as well (groups == 1; `splitk` as passed to the
 * launch): every K split stores a partial image of dw (and partial channel sums for db), added in split order.  For bf16 it
 * equals s2p_conv2d_wgrad_workspace.  A call with the smaller scratch of s2p_conv2d_wgrad_workspace runs fp32 as before.  */
size_t s2p_conv2d_wgrad_det_workspace(const s2p_conv_desc* d, int cin_real, int cout_real, int splitk);
/* Batched weight gradient: n_jobs (<= 16) convolutions of the SAME geometry `d` (groups must be 1; a grouped conv is
 * passed as one job per group with offset pointers and the tensors' pitches in d->x_pitch / d->y_pitch) in ONE launch.
 * `jobs` is a HOST array (copied into the kernel arguments: safe under hipGraph capture).  dw / db are ACCUMULATED into,
 * as in s2p_conv2d_wgrad.  For bf16 3x3 stride-1 pad-1 convs with Cin, Cout multiples of 64 this runs the slab kernel
 * (csrc/wgrad_slab.hip): no atomics -- K-split partial tiles go to `workspace` and are summed in a fixed order, so the
 * result is bitwise reproducible; other geometries run one s2p_conv2d_wgrad_ws launch per job on the same workspace.
 * workspace: caller-owned device scratch of at least s2p_conv2d_wgrad_batched_workspace(...) bytes (may be 0).       */
typedef struct { const void* x; const void* dy; float* dw; float* db; } s2p_wgrad_job;
size_t s2p_conv2d_wgrad_batched_workspace(const s2p_conv_desc* d, int n_jobs, int cin_real, int cout_real);
int s2p_conv2d_wgrad_batched(const s2p_conv_desc* d, const s2p_wgrad_job* jobs, int n_jobs, int cin_real,
                             int cout_real, void* workspace, size_t workspace_bytes, void* stream);
/* adjoint of F.pad(mode='reflect'): dx[N,H,W,C] = fold(dxp[N,H+2p,W+2p,C]).  C is the NHWC pitch (a multiple of the
 * 16-byte chunk), dxp and dx 16-byte aligned, pad < H and pad < W (as F.pad requires).   */
int s2p_reflect_pad_bwd(int dtype, const void* dxp, int N, int H, int W, int C, int pad, void* dx,
                        void* stream);
/* db[c] += sum over pixels of dy[p][c]  (bias gradient; fp32 accumulate into db)        */
int s2p_channel_sum(int dtype, const void* dy, int64_t pixels, int C, int pitch, float* db,
                    void* stream);
/* the same without atomics: per-block partial sums in a caller-owned scratch of s2p_channel_sum_workspace(pixels, C) bytes and
 * a fixed-order reduce (bitwise reproducible); a NULL / short scratch runs s2p_channel_sum                               */
size_t s2p_channel_sum_workspace(int64_t pixels, int C);
int s2p_channel_sum_ws(int dtype, const void* dy, int64_t pixels, int C, int pitch, float* db, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- instance norm + MAT/SPADE modulation (replaces F.instance_norm + the elementwise
 *      `normalized * (1 + gamma) + beta` + activation of the SPADE-lineage norm) -------- */
/* Per-(n,c) statistics of x over the HW pixels of each image.  `stats` is an OPAQUE fp32 buffer of
 * s2p_in_stats_floats(N,HW,C) elements, written (not accumulated: no zero-init needed) by s2p_in_stats and read by
 * the three consumers below with the SAME (N,HW,C): per-split partial moments {mean_b, M2_b} about a pivot, merged
 * by the consumers in a fixed order (no atomics: bitwise reproducible; no cancellation for |mean| >> std).
 * The buffer is self-describing (it starts with its split geometry): a consumer may be called on a batch PREFIX
 * (N' <= N images of the same x) with the same buffer.  Consumers use mean and rstd = 1/sqrt(biased var + eps).
 * Pitches may exceed C: every entry point of this section reads and writes channels [0, C) of a pixel only -- the pad
 * columns at and beyond C of y, dx and dgb_img (beyond 2C there: gamma | beta) and everything outside [0, 2C) of a
 * dgb_st row keep what they held.
 * Every entry point of this section refuses (returns -1 and sets s2p_last_error, before any launch) N <= 0, HW <= 0
 * and a NULL required pointer: x, stats, the output (y / dx), da for the backward, `sums` where the two kernels run. */
int64_t s2p_in_stats_floats(int N, int HW, int C);
int s2p_in_stats(int dtype, const void* x, int N, int HW, int C, int pitch, float eps,
                 float* stats, void* stream);
/* y = act(xhat*(1+g_img+g_st) + (b_img+b_st)).  gb_img: [N,HW,gb_pitch] with gamma at
 * channel offset 0 and beta at offset C (NULL -> 0); gb_st: fp32 [N][gb_st_pitch], gamma at
 * [0,C) beta at [C,2C) (NULL -> 0).                                                     */
int s2p_in_apply_fwd(int dtype, const void* x, int N, int HW, int C, int pitch,
                     const float* stats, const void* gb_img, int gb_pitch,
                     const float* gb_st, int gb_st_pitch, int act, float slope, float eps,
                     void* y, int y_pitch, void* stream);
/* s2p_in_stats + s2p_in_apply_fwd in one call: for planes of at most 512 (bf16) / 256 (fp32) pixels ONE fused launch
 * reads x once, computes exact two-pass statistics and applies the modulation; larger planes run the two kernels.
 * `stats` (s2p_in_stats_floats(N,HW,C) floats) is written in the same format either way, for the backward.        */
int s2p_in_norm_fwd(int dtype, const void* x, int N, int HW, int C, int pitch, const void* gb_img, int gb_pitch,
                    const float* gb_st, int gb_st_pitch, int act, float slope, float eps, void* y, int y_pitch,
                    float* stats, void* stream);
/* backward, given da = dL/dy (post-activation).  `sums` is an OPAQUE fp32 buffer of
 * s2p_in_bwd_sums_floats(N,HW,C) elements (per-split partial backward sums; written by
 * s2p_in_bwd_reduce, read by s2p_in_bwd_apply; no zero-init needed).
 * s2p_in_bwd_apply writes dx, d(gamma_img | beta_img) into dgb_img (layout of gb_img; may be NULL)
 * and d(gamma_st | beta_st) into dgb_st (fp32 [N][dgb_st_pitch], layout of gb_st; may be NULL). */
int64_t s2p_in_bwd_sums_floats(int N, int HW, int C);
int s2p_in_bwd_reduce(int dtype, const void* da, int da_pitch, const void* x, int N, int HW, int C,
                      int pitch, const float* stats, const void* gb_img, int gb_pitch,
                      const float* gb_st, int gb_st_pitch, int act, float slope, float eps,
                      float* sums, void* stream);
/* (the backward entry points take act none / relu / lrelu / tanh: the derivative is formed from the activation's
 * output, which swish does not allow -- S2P_ACT_SWISH and unknown ids are refused)       */
int s2p_in_bwd_apply(int dtype, const void* da, int da_pitch, const void* x, int N, int HW, int C,
                     int pitch, const float* stats, const void* gb_img, int gb_pitch,
                     const float* gb_st, int gb_st_pitch, int act, float slope, float eps,
                     const float* sums, void* dx, int dx_pitch, void* dgb_img, int dgb_pitch,
                     float* dgb_st, int dgb_st_pitch, void* stream);

/* ---- state path: positional encoding (nerf-pytorch embedder)  ------------------------ */
/* out[n][0:S]=s, then for k<L: sin(2^k s), cos(2^k s); columns >= S*(1+2L) up to out_pitch
 * are zero-filled.  fp32 in / fp32 out.                                                 */
int s2p_posenc_fwd(const float* state, int N, int S, int L, float* out, int out_pitch, void* stream);

/* s2p_in_bwd_reduce + s2p_in_bwd_apply in one call (one fused launch for planes of at most 512 (bf16) / 256 (fp32) pixels with
 * relu / lrelu / no activation; otherwise the two kernels, which need `sums`).                                             */
int s2p_in_norm_bwd(int dtype, const void* da, int da_pitch, const void* x, int N, int HW, int C, int pitch,
                    const float* stats, const void* gb_img, int gb_pitch, const float* gb_st, int gb_st_pitch,
                    int act, float slope, float eps, float* sums, void* dx, int dx_pitch, void* dgb_img,
                    int dgb_pitch, float* dgb_st, int dgb_st_pitch, void* stream);
/* The same with dx += res folded into the store (res: a tensor of dx's layout and dtype, e.g. the skip-connection gradient of
 * a residual block; fp32 add, one rounding; the two-kernel path adds it in a third pass).                                   */
int s2p_in_norm_bwd_res(int dtype, const void* da, int da_pitch, const void* x, int N, int HW, int C, int pitch,
                        const float* stats, const void* gb_img, int gb_pitch, const float* gb_st, int gb_st_pitch,
                        int act, float slope, float eps, float* sums, void* dx, int dx_pitch, void* dgb_img,
                        int dgb_pitch, float* dgb_st, int dgb_st_pitch, const void* res, int res_pitch, void* stream);
/* Which launch form s2p_in_norm_fwd (backward == 0) / s2p_in_norm_bwd[_res] (backward != 0) take for this problem: PAIR = the two
 * kernels (s2p_in_stats + s2p_in_apply_fwd / s2p_in_bwd_reduce + s2p_in_bwd_apply); F256 / F512 / F1024 = one fused launch of that
 * many threads per (image, 64-channel slab); L<channels>X<chunks> = the register-resident large-plane forwards (bf16, plain
 * InstanceNorm); F1024_CS32 = the 32-channel variant of F1024, selectable in the diagnostics build only.  has_gb_img: gamma | beta
 * maps are passed; wants_dgb_img (backward only): their gradient is asked for.  A dry run of the entry points' own rule: no launch,
 * no device access; -1 (s2p_last_error) for a bad dtype, N <= 0, HW <= 0 or a C the entry points refuse.  For tests and tools:
 * which form a shape takes is not part of the contract. */
enum { S2P_NORM_FORM_PAIR = 0, S2P_NORM_FORM_F256 = 1, S2P_NORM_FORM_F512 = 2, S2P_NORM_FORM_F1024 = 3, S2P_NORM_FORM_L64X28 = 4,
       S2P_NORM_FORM_L32X14 = 5, S2P_NORM_FORM_L16X28 = 6, S2P_NORM_FORM_F1024_CS32 = 7 };
int s2p_in_norm_form(int dtype, int N, int HW, int C, int has_gb_img, int wants_dgb_img, int act, int backward);

/* Small fp32 linear layers of the state path (replaces F.linear + LeakyReLU and their autograd backward for the
 * StateMapping MLP and the per-norm state affine; batch M of a few dozen rows: latency-bound, csrc/linear_small.hip).
 * y[M][y_pitch] = act(x[M][K] . w[N][w_row]^T + bias[N]); columns [N, n_store) of y are written as zeros.
 * K, pitches and w_row must be multiples of 4 floats.  act: any of S2P_ACT_NONE .. S2P_ACT_SWISH (tanh as tanhf, swish as
 * v / (1 + exp(-v))); any other id is refused before the launch.  M == 0 (an empty batch) is a successful no-op that looks at
 * no pointer, here and in s2p_linear_bwd; M < 0, K <= 0 and N <= 0 are refused.            */
int s2p_linear_fwd(const float* x, int M, int K, int x_pitch, const float* w, int w_row, const float* bias, int N,
                   int act, float slope, float* y, int y_pitch, int n_store, void* stream);
/* Backward given dy = dL/dy and the layer OUTPUT y (needed when act != NONE; dpre = dy * act'(y)):
 *   dw[N][dw_row] += dpre^T . x (columns < k_real), db[N] += sum_m dpre (db may be NULL),
 *   dx[M][dx_pitch] = dpre . w  (dx may be NULL; needs w_bwd [K][wb_row], the transpose of w).
 * No atomics: fixed summation order.  workspace: s2p_linear_bwd_workspace(M,K,N) bytes (0 for N < 2048; needed only with dx);
 * a missing or short workspace is refused before anything is launched, dw and db included.
 * act: none / relu / lrelu; anything else is refused (the forward also takes tanh and swish).              */
size_t s2p_linear_bwd_workspace(int M, int K, int N);
int s2p_linear_bwd(const float* x, int x_pitch, const float* dy, int dy_pitch, const float* y, int y_pitch, int M,
                   int K, int k_real, int N, const float* w_bwd, int wb_row, int act, float slope, float* dw,
                   int dw_row, float* db, float* dx, int dx_pitch, void* workspace, size_t workspace_bytes,
                   void* stream);

/* ---- SLAC latent model: Gaussian heads, KL and likelihood terms (SPEC.md N3b; reference rlkit/torch/slac/network/
 *      latent.py:29-52, 239-311 and slac/utils.py:66-69; csrc/gauss.hip).  All fp32 except the image likelihood's mu / dmu.
 * Common to these entry points: every tensor argument comes with its own row pitch in ELEMENTS (pass the pointer already
 * offset to the first column), so a slice of a [B,S+1,288] sequence buffer is read or written in place; a negative size is
 * refused, a size of 0 is a successful no-op that looks at no pointer, NULL for a required tensor and a pitch shorter than the
 * row are refused before anything is launched (non-zero, s2p_last_error).  No atomics and a fixed summation order everywhere
 * except the loss word of s2p_gauss_ll_image (stated there).                                                              */
/* Gaussian head (replaces torch.chunk + F.softplus + `mean + randn_like(std) * std`): raw [M][raw_pitch >= 2 D] is the last
 * linear's output [mean | raw_std];  mean[m][d] = raw[m][d],  std = softplus(raw[m][D + d]) + 1e-5  (softplus evaluated as
 * max(r, 0) + log1p(exp(-|r|)): no overflow, never 0),  and with eps:  z = z2 = mean + eps * std.  Any of mean, std, z, z2 may
 * be NULL (at least one is not); z / z2 need eps.                                                                         */
int s2p_gauss_head_fwd(const float* raw, int raw_pitch, int M, int D, const float* eps, int eps_pitch, float* mean,
                       int mean_pitch, float* std, int std_pitch, float* z, int z_pitch, float* z2, int z2_pitch,
                       void* stream);
/* draw[m][0:D] = dmean + dz + dz2,  draw[m][D:2D] = (dstd + (dz + dz2) * eps) * sigmoid(raw[m][D:2D]);  any of dmean, dstd,
 * dz, dz2 may be NULL (= 0; dz and dz2 are the gradients arriving at the two copies of the sample); dz / dz2 need eps.    */
int s2p_gauss_head_bwd(const float* raw, int raw_pitch, int M, int D, const float* eps, int eps_pitch, const float* dmean,
                       int dmean_pitch, const float* dstd, int dstd_pitch, const float* dz, int dz_pitch, const float* dz2,
                       int dz2_pitch, float* draw, int draw_pitch, void* stream);
/* s2p_linear_fwd with an additive input:  y = act(x[M][K] . w[N][w_row]^T + add[M][add_pitch] + bias)  (add, bias may be
 * NULL; y may be the add buffer itself).  For a first layer whose input is a concatenation of which only some columns
 * change per time step: the other columns' product is one batched s2p_linear_fwd over all time steps, passed here as add.
 * K, x_pitch, w_row multiples of 4 floats, x and w 16-byte aligned; columns [N, n_store) of y are written as zeros.
 * The kernel is s2p_linear_fwd's (csrc/linear_small.hip): with add == NULL the two return the same bits.                  */
int s2p_linear_add_fwd(const float* x, int M, int K, int x_pitch, const float* w, int w_row, const float* bias, int N,
                       const float* add, int add_pitch, int act, float slope, float* y, int y_pitch, int n_store,
                       void* stream);
/* Its backward, every output optional (at least one), dpre = dy * act'(y) (act none / relu / lrelu, y = the layer OUTPUT):
 *   dadd[M][dadd_pitch] = dpre                       (the additive term's gradient, and what a weight-gradient pass that is
 *                                                    batched over all time steps after the chain takes as its dy)
 *   dw[N][dw_row] += dpre^T x (columns < k_real), db[N] += sum_m dpre     (s2p_linear_bwd's pass: N, pitches multiples of 4;
 *                                                    db needs dw)
 *   dx[M][dx_pitch] = dpre . w  or, with dx_accumulate != 0,  dx += dpre . w  (w_bwd [K][wb_row >= N] = the transpose of w;
 *                                                    N, dy_pitch, wb_row multiples of 4, dy / y / w_bwd 16-byte aligned)  */
int s2p_linear_add_bwd(const float* x, int x_pitch, const float* dy, int dy_pitch, const float* y, int y_pitch, int M,
                       int K, int k_real, int N, const float* w_bwd, int wb_row, int act, float slope, float* dw,
                       int dw_row, float* db, float* dx, int dx_pitch, int dx_accumulate, float* dadd, int dadd_pitch,
                       void* stream);
/* The whole forward of the reparameterised posterior chain (latent.py:250-281) for B rows and T time steps in ONE launch
 * (SPEC.md N3h; csrc/gauss_chain.hip): what the no-grad path otherwise runs as 8 T launches of s2p_linear_fwd /
 * s2p_linear_add_fwd / s2p_gauss_head_fwd, and BITWISE what those return (the same MFMA sequence per output element, K never
 * split, the same epilogues; a row's values do not depend on B).  No backward: nothing is kept.  feature 256, z1 32, z2 256,
 * hidden 256 are compile-time constants.
 *   feat   feat(0) of batch row b at feat + b * feat_pitch (feat_pitch = T * 256 inside a [B][T][256] tensor); 16-byte
 *          aligned, feat_pitch a multiple of 4 floats
 *   ra, rb [(T-1) * B][256], time-major (row (t-1) * B + b): the hoisted terms of the two chain MLPs' first layers, i.e.
 *          [feat(t) | a(t-1)] . w^T of z1_posterior and a(t-1) . w^T of z2_prior, without bias (one s2p_linear_fwd each over
 *          all time steps).  May be NULL when T == 1.
 *   eps    [B][T][eps_pitch >= 288], the noise of z1 | z2; row (b, t) at (b * T + t) * eps_pitch -- as mean, std, z below
 *   mlps   HOST array of 4 (copied into the kernel arguments): z1_posterior_init, z2_prior_init, z1_posterior, z2_prior
 *          (the last two are not looked at when T == 1).  w1 [256][w1_row >= k1] holds the CHAIN columns of the first layer only:
 *          k1 = 256 (feat), 32 (z1), 256 (z2(t-1)), 288 (z1(t) | z2(t-1)); w2 [256][256]; w3 [2 D][256] = [mean | raw_std] rows,
 *          D = 32, 256, 32, 256; the weights 16-byte aligned, w1_row a multiple of 4 floats.
 *   mean, std [B][T][pitch >= 32]  of z1;   z [B][T][z_pitch >= 288] = z1 | z2.  Nothing else is written to device memory.
 * A negative size is refused; B == 0 (or T == 0) is a successful no-op that looks at no pointer; T == 1 runs the two init MLPs
 * only; a NULL required tensor, a short pitch, another k1 and a misaligned operand are refused before the launch.           */
typedef struct {
  const float* w1; const float* b1; const float* w2; const float* b2; const float* w3; const float* b3;
  int32_t k1, w1_row;
} s2p_chain_mlp;
int s2p_posterior_chain_fwd(const float* feat, int feat_pitch, const float* ra, const float* rb, const float* eps,
                            int eps_pitch, const s2p_chain_mlp* mlps, float* mean, int mean_pitch, float* std, int std_pitch,
                            float* z, int z_pitch, int B, int T, void* stream);
/* Open-loop rollout of the generative model (SPEC.md N3i; latent.py:240-248 z1_prior, :270-277 z2_prior, fed their own samples) for B
 * rows and H steps in ONE launch, the kernel design and the step body of s2p_posterior_chain_fwd.  For h = 1..H:
 *   (mu1, sd1) = z1_prior([z2(h-1) | a(h-1)]),  z1(h) = mu1 + eps1(h) sd1;
 *   (mu2, sd2) = z2_prior([z1(h) | z2(h-1) | a(h-1)]),  z2(h) = mu2 + eps2(h) sd2;   the slot of step h is h - 1.
 * Both first layers are pre = (acc + add) + bias with acc the MFMA sum over the chain columns only (K = 256, 288) and add the action
 * columns' product: BITWISE the per-layer path out of s2p_linear_add_fwd / s2p_linear_fwd / s2p_gauss_head_fwd.
 *   z2_0   z2(0) of batch row b at z2_0 + b * z2_0_pitch (a column slice of a [B][288] z(0) is read in place); 16-byte aligned,
 *          the pitch >= 256 and a multiple of 4 floats
 *   rc, rb [H * B][256], time-major (row (h-1) * B + b): a(h-1) . w^T of z1_prior's and of z2_prior's action columns, no bias
 *   eps    [B][H][eps_pitch >= 288], the noise of z1(h) | z2(h); row (b, h-1) at (b * H + h - 1) * eps_pitch -- as mean, std, z
 *   mlps   HOST array of 2: z1_prior with k1 == 256 (w1 may be the packed [256][pad4(256 + A)] matrix, w1_row its pitch: the
 *          chain columns are read in place), z2_prior with k1 == 288; other fields as for s2p_posterior_chain_fwd
 *   mean, std [B][H][pitch >= 32]  of z1;   z [B][H][z_pitch >= 288] = z1 | z2.  Nothing else is written to device memory.
 * A negative size is refused; B == 0 (or H == 0) is a successful no-op that looks at no pointer; a NULL tensor, a short pitch,
 * another k1, a short or odd w1_row and a misaligned operand are refused before the launch.                                   */
int s2p_prior_chain_fwd(const float* z2_0, int z2_0_pitch, const float* rc, const float* rb, const float* eps, int eps_pitch,
                        const s2p_chain_mlp* mlps, float* mean, int mean_pitch, float* std, int std_pitch, float* z, int z_pitch,
                        int B, int H, void* stream);
/* Closed-loop rollout (SPEC.md N3j): a deterministic tanh policy inside the loop of s2p_prior_chain_fwd, B rows and H steps in ONE
 * launch.  For h = 0..H-1, z(0) = z0:
 *   a(h) = tanh(last_fc(relu(fc1(relu(fc0(z(h)))))));  (mu1, sd1) = z1_prior([z2(h) | a(h)]),  z1(h+1) = mu1 + eps1 sd1;
 *   (mu2, sd2) = z2_prior([z1(h+1) | z2(h) | a(h)]),  z2(h+1) = mu2 + eps2 sd2;   slot h holds a(h) and z(h+1).
 * BITWISE the per-layer path: the policy layers as s2p_linear_fwd (relu, relu, tanh on the first A rows of w3), the two action
 * terms as s2p_linear_fwd of a(h) [B][pad4(A)] on wc / wb without bias, then the step of s2p_prior_chain_fwd.
 *   z0     [B][z0_pitch >= 288] = z1(0) | z2(0), 16-byte aligned, the pitch a multiple of 4 floats
 *   eps    [B][H][eps_pitch >= 288], the noise of z1(h+1) | z2(h+1) in slot h
 *   mlps   HOST array of 2: z1_prior with k1 == 256 (read in place, as s2p_prior_chain_fwd), z2_prior with k1 == 288
 *   wc, wb [256][row >= pad4(A)]: the action columns of z1_prior's and z2_prior's first layers, zero-padded, 16-byte aligned
 *   policy HOST struct: w1 [W][w1_row >= 288], w2 [W][W], w3 [>= A][W] (the last_fc rows first), biases; W = width, a multiple of
 *          128 from 128 to 1024; 1 <= A <= 8; the weights 16-byte aligned
 *   act    [B][H][act_pitch >= A]: exactly A columns are written;  mean, std, z as for s2p_prior_chain_fwd.  Nothing else is written.
 * A negative size is refused; B == 0 (or H == 0) is a successful no-op that looks at no pointer; a NULL pointer, another k1, an
 * unsupported W or A, a short pitch, a short or odd w*_row and a misaligned operand are refused before the launch.              */
typedef struct {
  const float* w1; const float* b1; const float* w2; const float* b2; const float* w3; const float* b3;
  int32_t w1_row, width;
} s2p_policy_mlp;
int s2p_imagine_chain_fwd(const float* z0, int z0_pitch, const float* eps, int eps_pitch, const s2p_chain_mlp* mlps, const float* wc,
                          int wc_row, const float* wb, int wb_row, int A, const s2p_policy_mlp* policy, float* act, int act_pitch,
                          float* mean, int mean_pitch, float* std, int std_pitch, float* z, int z_pitch, int B, int H, void* stream);
/* The posterior chain under grad (SPEC.md N3k): s2p_posterior_chain_fwd that also stores what the backward reads, and the
 * sequential part of that backward, ONE launch each, one workgroup per 16 batch rows.  Both are BITWISE the per-layer path.
 * s2p_chain_state: the activations of the chain for B rows and S = T - 1 steps, every buffer dense fp32, 16-byte aligned:
 *   a0_*, b0_*  (h1 [B][256], h2 [B][256], raw [B][64 | 512]) of z1_posterior_init and z2_prior_init at t = 0
 *   h1a, h2a [S][B][256], rawa [S][B][64]; h1b, h2b [S][B][256], rawb [S][B][512]: z1_posterior and z2_prior at t = 1..S in slot t - 1;
 *   raw = [mean | raw_std], the last layer's acc + bias
 *   xz [S][B][288]: slot t - 1 = z1(t) | z2(t-1), the input rows of both first layers
 * s2p_chain_grads: what the backward chain writes, time-major like the state: drawa [S][B][64], drawb [S][B][512], dh2a, dh1a, dh2b,
 *   dh1b [S][B][256] (the gradient at each layer's OUTPUT, before its activation derivative) and dxz [S][B][288], slot t - 1 = the
 *   gradient at z1(t) | z2(t-1) from the steps t .. S (without dz).
 * s2p_chain_mlp_bwd: the transposed packs of one chain MLP: w1t [k1][w1t_row >= 256] (row k = column k of the first layer's chain
 *   columns), w2t [256][256], w3t [256][2 D], all 16-byte aligned, w1t_row a multiple of 4 floats.
 * s2p_posterior_chain_fwd_save: the arguments and refusals of s2p_posterior_chain_fwd, and a HOST `state` whose t = 0 buffers (and,
 *   with T > 1, chain buffers) are written for the rows < B; a NULL or misaligned one is refused.  mean, std, z as without it.
 * s2p_posterior_chain_bwd: the steps t = T-1 .. 1 of the backward.  eps, dz [B][T][pitch >= 288], dmean, dstd [B][T][pitch >= 32]
 *   (rows (b, t) at (b * T + t) * pitch; slot 0 is not read); mlps: HOST array of 2, z1_posterior (k1 256) and z2_prior (k1 288);
 *   state: h1a .. rawb are read; grads: all seven are written, nothing else is.  A negative size, a NULL pointer, another k1, a short
 *   pitch, a short or odd w1t_row and a misaligned operand are refused; B == 0 and T < 2 are no-ops that look at no pointer.     */
typedef struct {
  float* a0_h1; float* a0_h2; float* a0_raw; float* b0_h1; float* b0_h2; float* b0_raw;
  float* h1a; float* h2a; float* rawa; float* h1b; float* h2b; float* rawb; float* xz;
} s2p_chain_state;
typedef struct { float* drawa; float* dh2a; float* dh1a; float* drawb; float* dh2b; float* dh1b; float* dxz; } s2p_chain_grads;
typedef struct { const float* w1t; const float* w2t; const float* w3t; int32_t k1, w1t_row; } s2p_chain_mlp_bwd;
int s2p_posterior_chain_fwd_save(const float* feat, int feat_pitch, const float* ra, const float* rb, const float* eps,
                                 int eps_pitch, const s2p_chain_mlp* mlps, float* mean, int mean_pitch, float* std, int std_pitch,
                                 float* z, int z_pitch, const s2p_chain_state* state, int B, int T, void* stream);
int s2p_posterior_chain_bwd(const float* eps, int eps_pitch, const float* dmean, int dmean_pitch, const float* dstd, int dstd_pitch,
                            const float* dz, int dz_pitch, const s2p_chain_mlp_bwd* mlps, const s2p_chain_state* state,
                            const s2p_chain_grads* grads, int B, int T, void* stream);
/* The two fused no-grad chains in bf16 compute (SPEC.md N3m; csrc/gauss_chain_bf16.hip): the arguments, no-ops and refusals of
 * s2p_posterior_chain_fwd and s2p_prior_chain_fwd, ONE launch each.  Every tensor stays fp32 except the weight operands:
 * s2p_chain_mlp_bf16 holds w1 [256][w1_row >= k1] (the CHAIN columns of the first layer only; for z1_prior a pack of its 256 z2
 * columns), w2 [256][256] and w3 [2 D][256] as bf16 bits, each the fp32 parameter rounded to nearest even, 16-byte aligned, w1_row in
 * bf16 elements and a multiple of 8; the biases are fp32.  Per layer: both operands bf16 (the activations are rounded where the kernel
 * writes them to LDS), acc = the fp32 sum of the exact products on v_mfma_f32_16x16x32_bf16 with k ascending in steps of 32 and K never
 * split, then (acc + add) + bias or acc + bias, LeakyReLU 0.2 and the head in fp32 as in the fp32 chains; z is stored unrounded.  A
 * row's values do not depend on B; two identical calls are bitwise equal.  Nothing but mean, std and z is written.            */
typedef struct {
  const uint16_t* w1; const float* b1; const uint16_t* w2; const float* b2; const uint16_t* w3; const float* b3;
  int32_t k1, w1_row;
} s2p_chain_mlp_bf16;
int s2p_posterior_chain_fwd_bf16(const float* feat, int feat_pitch, const float* ra, const float* rb, const float* eps,
                                 int eps_pitch, const s2p_chain_mlp_bf16* mlps, float* mean, int mean_pitch, float* std,
                                 int std_pitch, float* z, int z_pitch, int B, int T, void* stream);
int s2p_prior_chain_fwd_bf16(const float* z2_0, int z2_0_pitch, const float* rc, const float* rb, const float* eps, int eps_pitch,
                             const s2p_chain_mlp_bf16* mlps, float* mean, int mean_pitch, float* std, int std_pitch, float* z,
                             int z_pitch, int B, int H, void* stream);
/* The closed-loop rollout in bf16 compute (SPEC.md N3n; csrc/gauss_chain_bf16.hip): the arguments, no-ops and refusals of
 * s2p_imagine_chain_fwd, ONE launch.  Every tensor stays fp32 (z0, eps, wc, wb, act, mean, std, z, the biases) except the weight
 * operands: mlps as for s2p_prior_chain_fwd_bf16 (z1_prior: the pack of its 256 z2 columns, k1 == 256; z2_prior: k1 == 288), and
 * s2p_policy_mlp_bf16 holds w1 [W][w1_row >= 288], w2 [W][W], w3 [>= A][W] (the last_fc rows first) as bf16 bits, each the fp32
 * parameter rounded to nearest even, 16-byte aligned, w1_row in bf16 elements and a multiple of 8.  The latent half follows the rule
 * above.  The policy's first layer reads z(h) as the kernel holds it in bf16; its two hidden activations are rounded to bf16 where
 * they are written to LDS; per layer acc = the fp32 sum of the exact products on v_mfma_f32_16x16x32_bf16, k ascending in steps of 32,
 * K never split, then relu(acc + bias) resp. tanh(acc + bias) in fp32.  a(h) is NOT rounded: the two action terms are bitwise
 * s2p_linear_fwd of a(h) [B][pad4(A)] on wc / wb without bias, the first layers (acc + add) + bias.  A row's values do not depend on B;
 * two identical calls are bitwise equal.  Nothing but act (exactly A columns), mean, std and z is written.                          */
typedef struct {
  const uint16_t* w1; const float* b1; const uint16_t* w2; const float* b2; const uint16_t* w3; const float* b3;
  int32_t w1_row, width;
} s2p_policy_mlp_bf16;
int s2p_imagine_chain_fwd_bf16(const float* z0, int z0_pitch, const float* eps, int eps_pitch, const s2p_chain_mlp_bf16* mlps,
                               const float* wc, int wc_row, const float* wb, int wb_row, int A, const s2p_policy_mlp_bf16* policy,
                               float* act, int act_pitch, float* mean, int mean_pitch, float* std, int std_pitch, float* z, int z_pitch,
                               int B, int H, void* stream);
/* The posterior chain under grad in bf16 compute (SPEC.md N3p; csrc/gauss_chain_bf16.hip): ordinary mixed precision for
 * s2p_posterior_chain_fwd_save / s2p_posterior_chain_bwd, ONE launch each.  Every tensor the caller sees, the state and the
 * gradients stay fp32; only the chain's own GEMMs multiply bf16 operands on v_mfma_f32_16x16x32_bf16.
 * s2p_posterior_chain_fwd_save_bf16: the arguments of s2p_posterior_chain_fwd_save with the mlps of s2p_posterior_chain_fwd_bf16.
 *   mean, std and z are BITWISE those of s2p_posterior_chain_fwd_bf16; the 13 state buffers get the UNROUNDED fp32 values (h1, h2
 *   after LeakyReLU, raw = acc + bias, xz[t-1] = z1(t) | z2(t-1)) in the fp32 form's layout, rows >= B never stored.  No-ops and
 *   refusals: those of s2p_posterior_chain_fwd_bf16, then the state refusals of the fp32 save form.
 * s2p_chain_mlp_bwd_bf16: w1t [k1][w1t_row >= 256], w2t [256][256], w3t [256][2 D] as bf16 bits, the TRANSPOSES of the forward's
 *   bf16 packs (the same rounded values), 16-byte aligned, w1t_row in bf16 elements and a multiple of 8.
 * s2p_posterior_chain_bwd_bf16: the arguments, no-ops (B == 0, T < 2) and refusals of s2p_posterior_chain_bwd.  A head backward is
 *   the fp32 one on fp32 inputs.  An input gradient is acc = sum_n bf16(g[m][n]) * bf16(wt[k][n]), g = draw for a last layer, else
 *   dh * act'(h) (one fp32 multiply, rounded where it is written to LDS), fp32 sums with n ascending in steps of 32, the reduction
 *   (512, 256 or 64) never split, then acc + 0, or (acc + dx_old) + 0 for the accumulating one.  The carried gradient at z1(t) |
 *   z2(t-1) stays fp32.  The seven buffers of `grads` are written in fp32, unrounded, and nothing else is.
 * s2p_chain_pack_bf16: ONE launch makes bf16 packs of `n_jobs` fp32 matrices.  A job reads src [rows][cols] (row pitch src_pitch
 *   floats; the pointer may stand at a column group of a wider matrix) and writes dst [rows][dst_pitch] and / or its transpose
 *   dst_t [cols][dst_t_pitch] as bf16 bits (pitches in elements; a NULL output is not made, one of the two is required).  Rounding
 *   is to nearest even, bit for bit a cast of the fp32 value for every finite value, +-0 and +-inf; NaN stays NaN.  Elements past
 *   `cols` / `rows` of a pitch are not written.  n_jobs == 0 and a job with rows == 0 or cols == 0 are no-ops that look at no
 *   pointer; a negative size, a NULL jobs / src, no output, or a pitch below its row are refused before the launch.
 * A row's values do not depend on B; two identical calls are bitwise equal.                                                      */
typedef struct { const uint16_t* w1t; const uint16_t* w2t; const uint16_t* w3t; int32_t k1, w1t_row; } s2p_chain_mlp_bwd_bf16;
typedef struct {
  const float* src; uint16_t* dst; uint16_t* dst_t;
  int32_t rows, cols, src_pitch, dst_pitch, dst_t_pitch;
} s2p_bf16_pack_job;
int s2p_posterior_chain_fwd_save_bf16(const float* feat, int feat_pitch, const float* ra, const float* rb, const float* eps,
                                      int eps_pitch, const s2p_chain_mlp_bf16* mlps, float* mean, int mean_pitch, float* std,
                                      int std_pitch, float* z, int z_pitch, const s2p_chain_state* state, int B, int T,
                                      void* stream);
int s2p_posterior_chain_bwd_bf16(const float* eps, int eps_pitch, const float* dmean, int dmean_pitch, const float* dstd,
                                 int dstd_pitch, const float* dz, int dz_pitch, const s2p_chain_mlp_bwd_bf16* mlps,
                                 const s2p_chain_state* state, const s2p_chain_grads* grads, int B, int T, void* stream);
int s2p_chain_pack_bf16(const s2p_bf16_pack_job* jobs, int n_jobs, void* stream);
/* KL(p || q) of diagonal Gaussians, value and all four gradients in one pass (slac/utils.py:66-69):
 *   loss[0] += scale * sum 0.5 ((sp/sq)^2 + ((mp-mq)/sq)^2 - 1 - log (sp/sq)^2),  d* = scale * dKL/d*  (overwritten; any NULL).
 * p: [B][T][p_pitch >= D].  const_first == 0: q is [B][T][q_pitch]; const_first != 0: q is [B][T-1][q_pitch] and holds the
 * steps 1..T-1, step 0 is compared with the constant N(0, I) (no gradient, nothing materialised).  dmu_p / dstd_p share
 * dp_pitch and p's row order, dmu_q / dstd_q share dq_pitch and q's.  One workgroup, plain add into loss.                 */
int s2p_gauss_kl(const float* mu_p, const float* std_p, int p_pitch, const float* mu_q, const float* std_q, int q_pitch,
                 int B, int T, int D, int const_first, float scale, float* loss, float* dmu_p, float* dstd_p,
                 int dp_pitch, float* dmu_q, float* dstd_q, int dq_pitch, void* stream);
/* Masked Gaussian negative log-likelihood of n scalars (the reward term, latent.py:303-310):
 *   nll_i = 0.5 ((target_i - mu_i) / (std_i + 1e-8))^2 + log std_i + 0.5 log 2 pi,  loss[0] += scale * sum (1 - done_i) nll_i,
 *   dmu[i], dstd[i] = scale (1 - done_i) d nll_i / d*  (contiguous, overwritten; may be NULL).  mu / std element i at
 *   i * pitch; target, done (NULL: no mask) contiguous.  One workgroup, plain add into loss.                             */
int s2p_gauss_ll(const float* mu, int mu_pitch, const float* std, int std_pitch, const float* target, const float* done,
                 int64_t n, float scale, float* loss, float* dmu, float* dstd, void* stream);
/* The same for images with a constant sigma (latent.py:296-300).  mu: NHWC [N][HW][pitch] in `dtype` (the decoder's output:
 * pitch a multiple of the 16-byte chunk, 16-byte aligned); target: fp32 NCHW [N][C][HW] (target_u8 == 0) or uint8 NHWC
 * [N][HW][C] read as u8 / 255 (target_u8 != 0) -- always at full precision, never from a compute-dtype copy;
 * dmu (may be NULL): scale * d nll / d mu in mu's layout and dtype, channels [C, pitch) written as zeros.
 * loss[0] += scale * sum nll ends in ONE fp32 atomicAdd per workgroup (as s2p_l1_loss): the value may differ in its last
 * bits from call to call, dmu does not.                                                                                   */
int s2p_gauss_ll_image(int dtype, const void* mu, int pitch, const void* target, int target_u8, int N, int C, int HW,
                       float sigma, float scale, float* loss, void* dmu, void* stream);

/* ---- pooling / resize / layout ---------------------------------------------------- */
/* Common to the entry points from here to the small elementwise helpers at the end: a negative size and an unknown dtype are
 * refused; a call that covers no element (a size of 0) returns 0 without a launch and without looking at its pointers;
 * otherwise NULL tensors are refused.  Alignment: where stated below the kernel moves whole 16-byte chunks and an unaligned
 * pointer is refused; the avg-pool, s2p_l1_loss and s2p_add take any element-aligned pointer (per-element form).
 * Every refusal happens before anything is launched (non-zero return, s2p_last_error).                                   */
/* F.avg_pool2d(k=3,s=2,p=1,count_include_pad=False) and its backward                   */
int s2p_avgpool3x3s2_fwd(int dtype, const void* x, int N, int H, int W, int C, void* y, void* stream);
int s2p_avgpool3x3s2_bwd(int dtype, const void* dy, int N, int H, int W, int C, void* dx,
                         int accumulate, void* stream);
/* F.max_pool2d(2,2) (floor) and backward fused with the producer's ReLU mask: x is a ReLU output (negative values and
 * -0.0 count as 0), dx = dy at the FIRST maximum of each window in (row, column) order if that maximum is > 0, else 0;
 * rows / columns of an odd H / W outside every window get 0.  C a multiple of the 16-byte chunk, all pointers 16-byte
 * aligned.                                                                              */
int s2p_maxpool2x2_fwd(int dtype, const void* x, int N, int H, int W, int C, void* y, void* stream);
int s2p_maxpool2x2_bwd(int dtype, const void* dy, const void* x, int N, int H, int W, int C,
                       void* dx, void* stream);
/* F.interpolate(mode='nearest') on NHWC                                                 */
int s2p_resize_nearest(int dtype, const void* x, int N, int H, int W, int C, void* y, int Ho, int Wo,
                       void* stream);
/* fp32 NCHW [N,C,H,W]  ->  NHWC dtype with channel pitch, written at channel offset c_off (c_off + C <= y_pitch);
 * zero_pad != 0: every other channel of the pitch is written as zero (y 16-byte aligned if the pitch is a whole number
 * of chunks), zero_pad == 0: the other channels are left untouched.  And back (accumulate != 0: y += ...).              */
int s2p_nchw_to_nhwc(int dtype, const float* x, int N, int C, int H, int W, void* y, int y_pitch,
                     int c_off, int zero_pad, void* stream);
int s2p_nhwc_to_nchw(int dtype, const void* x, int x_pitch, int c_off, int N, int C, int H, int W,
                     float* y, int accumulate, void* stream);
/* dataset frames: uint8 NHWC [pixels][C] (the layout rlkit/torch/slac/algo.py:189-190 reads) ->
 * NHWC dtype in [-1,1] with zero-padded pitch (v = u8/127.5 - 1), and back
 * (u8 = clamp(round((v+1)*127.5))); the round trip is exact on all 256 values.          */
int s2p_u8_to_nhwc(int dtype, const void* x, int64_t pixels, int C, void* y, int y_pitch, void* stream);
int s2p_nhwc_to_u8(int dtype, const void* x, int x_pitch, int64_t pixels, int C, void* y, void* stream);
/* SLAC sequence replay buffer (SPEC.md N3c): gather the frames of B sampled windows out of a uint8 frame pool.
 *   pool   uint8 [n_slots][frame_pixels * C]   NHWC frames, each stored once
 *   table  int32 [n_windows][T]                frame slots of every window
 *   win    int64 [B]                           window ids (the caller checks them against n_windows)
 *   x      dtype [B*T][frame_pixels][x_pitch]  from_f32((float)u8 / 255.0f) (true division); channels C..x_pitch are zero.  Nullable.
 *   u8_out uint8 [B*T][frame_pixels * C]       the gathered frames unchanged.  Nullable (not both).
 * Every source byte is read once for both outputs; all byte offsets are 64-bit.  A slot < 0 or >= n_slots reads as an all-zero
 * frame and is never dereferenced.  Any frame_pixels >= 1, 1 <= C <= x_pitch and any alignment of the pool are accepted; C == 3 with
 * frame_pixels % 4 == 0 (4-byte aligned pool / u8_out, x_pitch a whole number of 16-byte chunks) moves 4 pixels per thread step
 * with dword loads and 16-byte stores.  x must be 16-byte aligned.  B * T == 0 is a successful no-op.                  */
int s2p_window_gather_u8(int dtype, const void* pool, int64_t n_slots, int64_t frame_pixels, int C, const int32_t* table, int T,
                         const int64_t* win, int B, void* x, int x_pitch, void* u8_out, void* stream);
/* Decoded frame -> observed frame (SPEC.md N3o): the hand-off from the decoder to the encoder inside an imagined rollout.
 *   y      dtype [pixels_total][y_pitch]  the decoder's NHWC output; channels < C are read, each as float v
 *   x      dtype [pixels_total][x_pitch]  the encoder's NHWC input; channels C..x_pitch are exactly 0.  Nullable.
 *   u8_out uint8 [pixels_total][C]        the frame an environment would hand out.  Nullable (not both).
 * The byte is q = min(max(rintf(v * 255.0f), 0), 255): one fp32 multiply, ties to even, a NaN gives 0.  u8_out always holds q.
 * quantize != 0: x holds from_f32((float)q / 255.0f), a true IEEE division -- the value s2p_window_gather_u8 writes for the byte q.
 * quantize == 0: x holds from_f32(min(max(v, 0), 1)); a NaN and -0.0 give +0.
 * Every source element is read once for both outputs; all offsets are 64-bit.  Any C >= 1 with C <= y_pitch (and <= x_pitch where x
 * is given) is accepted; C == 3 with pixels_total % 4 == 0, both pitches whole numbers of 16-byte chunks, 16-byte aligned y and 4-byte
 * aligned u8_out moves 4 pixels per thread step with 16-byte loads and stores and three dword stores.  x must be 16-byte aligned, y
 * aligned to its element.  pixels_total == 0 is a successful no-op that looks at no pointer.                                        */
int s2p_decoded_to_frames(int dtype, const void* y, int y_pitch, int64_t pixels_total, int C, int quantize, void* x, int x_pitch,
                          void* u8_out, void* stream);
/* Cached encoder features of the replay buffer (SPEC.md N3g): with a frozen encoder a frame's feature row is a constant, kept in a
 * table beside the frame pool; one launch turns B sampled window ids into everything an RL step on a frozen latent model reads.
 *   feat        fp32  [n_slots][feat_pitch]    feature row of every pool slot, F floats used
 *   table / win                                as above; T = S + 1 >= 2; for row b: w = win[b], slot_t = table[w][t]
 *   action_     fp32  [n_windows][T-1][A]      reward_, done_  fp32 [n_windows][T-1]
 *   feature_    fp32  [B][T][F]                row (b, t) = feat[slot_t][0..F)
 *   fa          fp32  [B][fa_pitch]            [f_0 .. f_{T-2} | a_0 .. a_{T-3} | 0 pad]
 *   next_fa     fp32  [B][fa_pitch]            [f_1 .. f_{T-1} | a_1 .. a_{T-2} | 0 pad]   (create_feature_actions, features first)
 *   action_seq  fp32  [B][T-1][A]              action_[w]
 *   action_last fp32  [B][action_last_pitch]   action_[w][T-2], pad columns 0
 *   reward, terminal fp32 [B]                  reward_[w][T-2], done_[w][T-2]
 * Every output is nullable (all null is refused); an input is needed only by the outputs that read it.  Each feature row is read
 * once for its up to three destinations; all byte offsets are 64-bit.  A slot < 0 or >= n_slots reads as a zero row and is never
 * dereferenced; window ids are the caller's to check.  F % 4 == 0, feat_pitch % 4 == 0, feat_pitch >= F, fa_pitch % 4 == 0 and
 * >= (T-1) F + (T-2) A, A <= action_last_pitch; feat, feature_, fa, next_fa 16-byte aligned.  B * T == 0 is a successful no-op.  */
int s2p_feature_window_gather(const float* feat, int64_t n_slots, int feat_pitch, int F, const int32_t* table, int T,
                              const int64_t* win, int B, const float* action_, const float* reward_, const float* done_, int A,
                              float* feature_, float* fa, float* next_fa, int fa_pitch, float* action_seq, float* action_last,
                              int action_last_pitch, float* reward, float* terminal, void* stream);
/* S2P training set on the device (SPEC.md N1d): frame numbers -> the batch the generator's train step takes, in one launch.
 *   pool    uint8 [n_frames][H][W][C]          the dataset's image_observations as stored (NHWC)
 *   states  fp32  [n_frames][S]                its observations
 *   idx     int64 [B]                          device array of frame numbers t
 *   prev    fp32  [B][C][out_h][out_w]         frame t     (NCHW)
 *   image   fp32  [B][C][out_h][out_w]         frame t + 1.  Nullable.
 *   state   fp32  [B][S]                       states[t + 1].  Nullable.
 * Value: (float)u8 / 127.5f - 1.0f, the quotient and the difference each rounded in fp32 (torch's `.float() / 127.5 - 1.0`).
 * Resize: torch's `nearest`: source row = min((int)floorf(y * ((float)H / (float)out_h)), H - 1), columns likewise; out == source
 * size is the identity.  A row with t < 0 or t + 1 >= n_frames writes zeros to all its outputs and dereferences nothing; all byte
 * offsets are 64-bit.  B == 0 is a successful no-op that looks at no pointer.  Refused before the launch: a negative size, C < 1,
 * H, W, out_h or out_w < 1, a null pool / idx / prev, a null states with a state output, an fp32 pointer that is not 4-byte aligned.
 * C == 3 with out_w % 4 == 0, a 4-byte aligned pool, H * W * 3 a multiple of 4 and 16-byte aligned prev / image makes 4 pixels per
 * thread step from whole dwords with one 16-byte store per plane; anything else takes a one-pixel-per-thread path.               */
int s2p_frame_pair_gather(const void* pool, int64_t n_frames, int H, int W, int C, const float* states, int S, const int64_t* idx,
                          int B, int out_h, int out_w, float* prev, float* image, float* state, void* stream);
/* generic cast copy between dtypes (n elements)                                         */
int s2p_cast(int src_dtype, const void* src, int dst_dtype, void* dst, int64_t n, void* stream);

/* ---- losses (forward value + gradient seed in one pass) ---------------------------- */
/* loss_out[0] += scale * sum|a-b| ; if grad_a: grad_a = (accumulate? grad_a:0) + scale*sign(a-b)  (sign(0) = 0)
 * a,b: `count` elements each (dtype); any alignment (16-byte chunks only when a, b and grad_a are all aligned) */
int s2p_l1_loss(int dtype, const void* a, const void* b, int64_t count, float scale,
                float* loss_out, void* grad_a, int accumulate, void* stream);
/* n_jobs (<= S2P_L1_MAX_JOBS) such terms in one launch (the feature-matching maps of all PatchGAN scales, the VGG taps);
 * `jobs` is a HOST array (copied into the kernel arguments).  Pointers 16-byte aligned, counts a multiple of the 16-byte
 * chunk (8 bf16 / 4 fp32), an empty job is refused; grad_a is overwritten (no accumulate form).                      */
#define S2P_L1_MAX_JOBS 16
typedef struct { const void* a; const void* b; void* grad_a; int64_t count; float scale; float* loss_out; } s2p_l1_job;
int s2p_l1_loss_multi(int dtype, const s2p_l1_job* jobs, int n_jobs, void* stream);
/* hinge terms on a D logit map x (count elements):
 *   mode 0: loss += scale*sum(relu(1+x)), grad = scale*(1+x>0)      (D on fake)
 *   mode 1: loss += scale*sum(relu(1-x)), grad = -scale*(1-x>0)     (D on real)
 *   mode 2: loss += -scale*sum(x),       grad = -scale              (G)                */
int s2p_hinge_loss(int dtype, const void* x, int64_t count, int mode, float scale,
                   float* loss_out, void* grad_x, void* stream);
/* the same on an NHWC map x [pixels][pitch] whose channel 0 is the logit (the discriminator heads' output layout);
 * grad_x (same layout, may be NULL): gradient in channel 0, zeros in the other channels.  pitch a multiple of the 16-byte
 * chunk, grad_x 16-byte aligned                                                                                       */
int s2p_hinge_loss_strided(int dtype, const void* x, int64_t pixels, int pitch, int mode, float scale,
                           float* loss_out, void* grad_x, void* stream);

/* ---- ensemble state-dynamics head (reference gaussian_ensemble.py:83-96 and
 *      state_transition_rollout.py:192-204) ------------------------------------------------
 * raw   : fp32 [B][E*2*D] output of the last ensemble layer (member e at columns e*2D: mu | logstd)
 * xin   : fp32 [B][x_pitch] normalised (obs, action); obs_dim = D-1 leading columns
 * mean/std: fp32 [E][B][D] (may be NULL): mu (obs part + input obs, 'local' mode) and
 *         exp(soft_clamp(logstd, min_logstd, max_logstd))
 * pick  : int32 [B] member index per sample; next_obs [B][D-1] = mean[pick]*obs_std+obs_mean,
 *         reward [B] = mean[pick][D-1]*rew_std+rew_mean
 * disagreement[B] = max_e || mean_e[:D-1] - avg_e mean[:D-1] ||_2 ; aleatoric[B] = max_e || std_e ||_2
 * Argument checking as for the training entry points below: B < 0, a required NULL tensor, raw_pitch < E*2*D and
 * x_pitch < D-1 are refused before any launch (non-zero, s2p_last_error); B == 0 is a successful no-op that looks at no
 * pointer.  2 <= D <= 33, E >= 1.  pick[b] outside [0, E): nothing is read out of range, that row of next_obs and its reward
 * are written as NaN (a poisoned row stays visible downstream); the other rows and the other outputs are unaffected.  */
int s2p_ensemble_head(const float* raw, int raw_pitch, const float* xin, int x_pitch, int B, int E, int D,
                      const float* min_logstd, const float* max_logstd, float* mean, float* std,
                      const int32_t* pick, const float* obs_mean, const float* obs_std, float rew_mean,
                      float rew_std, float* next_obs, float* reward, float* disagreement, float* aleatoric,
                      void* stream);

/* ---- ensemble state-dynamics TRAINING (SPEC.md N2b; reference gaussian_ensemble.py:21-96; csrc/ensemble_train.hip).
 * All fp32 on v_mfma_f32_32x32x2_f32, group = ensemble member, every entry point ONE launch for all members, no atomics, fixed
 * summation order (two identical calls give bitwise identical results).
 * Layouts: activations [B][pitch >= G*N], group g at columns g*N (what s2p_ensemble_head reads); weights, biases and their
 * gradients PACKED [E][N][K] / [E][N] -- K = the input width padded to a multiple of 4, i.e. the TRANSPOSE of the reference's
 * [E, in, out] (the layout the grouped conv forward consumes).  `member` is a HOST array of G slot indices in [0, E) (copied
 * into the kernel arguments; NULL: 0..G-1): group g uses slot member[g] of the [E] arrays, the activations are compact in g.
 * x: group g, row m at x + g * x_gstride + m * x_pitch (x_gstride 0: every member reads the same [B][K] input; B * x_pitch: a
 * per-member [G][B][K] batch; N_prev with x_pitch = G * N_prev: the previous layer's activations).
 * Argument checking as stated above s2p_gauss_head_fwd: negative sizes, a required NULL tensor, a short pitch are refused
 * before any launch; a size of 0 (G, B or N) is a successful no-op that looks at no pointer.  1 <= G <= E <= 8.
 * K, N, the pitches and x_gstride multiples of 4 floats; x, w, dpre 16-byte aligned.                                          */
/* pre[m][g*N+n] = sum_k x[g][m][k] w[e][n][k] + bias[e][n];  act = pre * sigmoid(pre).  pre and/or act (at least one): the
 * backward of Swish needs pre, the next layer reads act.                                                                      */
int s2p_ensemble_linear_fwd(const float* x, int64_t x_gstride, int x_pitch, const float* w, const float* bias,
                            const int32_t* member, int G, int E, int B, int K, int N, float* pre, float* act, int y_pitch,
                            void* stream);
/* From dpre [B][dpre_pitch] of a layer: dw[e][n][k] = sum_m dpre[m][g*N+n] x[g][m][k] (packed orientation, OVERWRITTEN for the
 * listed members, other slots untouched), db[e][n] = sum_m dpre, and with dprev != NULL
 * dprev[m][g*K+k] = (sum_n dpre[m][g*N+n] w[e][n][k]) * swish'(pre_prev[m][g*K+k])  (pre_prev, dprev share prev_pitch).
 * Rows are summed in row order by one wave per tile at any B: there is no row split, hence no workspace.                  */
int s2p_ensemble_linear_bwd(const float* x, int64_t x_gstride, int x_pitch, const float* dpre, int dpre_pitch,
                            const float* w, const int32_t* member, int G, int E, int B, int K, int N, float* dw, float* db,
                            const float* pre_prev, float* dprev, int prev_pitch, void* stream);
/* Fused Gaussian NLL head.  raw [B][raw_pitch >= G*2D] (group g: mu | logstd), xin / target with a group stride like x above
 * (0: shared by the groups), bounds [D].  mu = raw_mu (+ xin for the D-1 obs outputs, 'local' mode), ls = soft_clamp(raw_ls),
 * nll = 0.5 ((target - mu) / exp(ls))^2 + ls + 0.5 log 2 pi.  Outputs, each optional:
 *   sums [2G]: sum nll per group, then sum (mu - target)^2 per group;   loss[0] = scale * sum nll + bound_reg * sum_d (max - min)
 *   draw [B][draw_pitch] = scale * d sum nll / d raw (both soft-clamp factors included)
 *   dmin_logstd / dmax_logstd [D] (together) = scale * d sum nll / d bound -/+ bound_reg
 *   mean / std [G][B][D] (the forward alone: target may then be NULL).  A call with no output at all is refused.
 * The caller owns the scaling: scale = 1 / (G B D), bound_reg = 0.01 / D give the loss of SPEC.md N2b.  2 <= D <= 33.     */
int s2p_ensemble_nll(const float* raw, int raw_pitch, const float* xin, int64_t x_gstride, int x_pitch, const float* target,
                     int64_t t_gstride, int t_pitch, int B, int G, int D, const float* min_logstd, const float* max_logstd,
                     float scale, float bound_reg, float* sums, float* loss, float* draw, int draw_pitch, float* dmin_logstd,
                     float* dmax_logstd, float* mean, float* std, void* stream);

/* ---- state-transition rollout input (SPEC.md N2c; reference state_transition_rollout.py:149, 180; csrc/transition.hip).
 * Raw observations [rows][obs_pitch] and actions [rows][act_pitch] of a whole dataset -> the ensemble's first-layer input
 *   x[r][j] = (obs[r][j] - obs_mean[j]) / obs_std[j]   j < obs_dim
 *           = action[r][j - obs_dim]                   the next act_dim columns
 *           = 0                                        every remaining column up to x_pitch
 * in ONE launch, row offsets 64-bit.  The subtraction and the division are separately rounded IEEE fp32 operations (a true
 * division), so x equals numpy's fp32 `(obs - mean) / std` bit for bit.  x_pitch % 4 == 0 with a 16-byte aligned x takes
 * 16-byte stores; any other pitch or alignment a per-element kernel.  Negative sizes, a required NULL pointer and a pitch
 * shorter than its row (x_pitch < obs_dim + act_dim, obs_pitch < obs_dim, act_pitch < act_dim) are refused before any launch;
 * rows == 0 is a successful no-op that looks at no pointer.                                                                  */
int s2p_transition_pack(const float* obs, int obs_pitch, const float* action, int act_pitch, const float* obs_mean,
                        const float* obs_std, int64_t rows, int obs_dim, int act_dim, float* x, int x_pitch, void* stream);

/* ---- IQL on SLAC latents (SPEC.md N3d; reference rlkit/torch/sac/iql_trainer.py:209-435; the grouped layers s2p_mlp_linear_* in
 * csrc/mlp.hip, the heads and the Polyak update in csrc/iql.hip).
 * All fp32, the wide layers on v_mfma_f32_32x32x2_f32, no atomics, a fixed summation order (two identical calls give bitwise
 * identical results).  Argument checking as stated above s2p_gauss_head_fwd: negative sizes, a required NULL tensor, a short
 * pitch and a misaligned operand are refused before any launch; a size of 0 is a successful no-op that looks at no pointer.  */
/* Grouped linear layer, group = network.  `groups` is a HOST array of G <= 8 views (copied into the kernel arguments): the
 * groups share N and the activation but each has its own row count, input width K (padded to a multiple of 4 floats) and
 * buffers, so networks of unequal input width, and vf on z and next_z (2 B rows) beside the Q networks on B rows, are ONE launch,
 * grid z = group.  A group with rows == 0 is skipped.  Weights [N][K] with K contiguous: torch's nn.Linear orientation.
 *   pre[m][n] = sum_k x[m][k] w[n][k] + bias[n];  act = relu(pre) (S2P_ACT_RELU) or pre (S2P_ACT_NONE);  pre and/or act.
 * N > 16: the 32 x 64 MFMA wave tiles of the ensemble entry points.  N <= 16 (the N = 1 and N = 2 A last layers, where such a
 * tile is mostly padding): a dot-product kernel, one wave per row.  Both: K, x_pitch multiples of 4, x and w 16-byte aligned. */
typedef struct {
  const float* x; const float* w; const float* bias; float* pre; float* act;
  int32_t x_pitch, y_pitch, rows, K;
} s2p_mlp_fwd_group;
int s2p_mlp_linear_fwd(const s2p_mlp_fwd_group* groups, int G, int N, int act, void* stream);
/* Its backward from dpre [rows][dpre_pitch]: dw[n][k] = sum_m dpre[m][n] x[m][k] and db[n] = sum_m dpre[m][n] (OVERWRITTEN, rows
 * summed in row order), and with dprev != NULL  dprev[m][k] = (sum_n dpre[m][n] w[n][k]) * [pre_prev[m][k] > 0]  for act_prev =
 * S2P_ACT_RELU (pre_prev: the producer's pre-activation or its ReLU output -- only the sign is used), unmasked for S2P_ACT_NONE
 * (pre_prev may then be NULL).  pre_prev and dprev share prev_pitch.  N > 16: N, dpre_pitch multiples of 4 and dpre 16-byte
 * aligned (MFMA tiles); N <= 16: no such demand (plain kernel, four row lanes added in lane order).  rows * K < 2^31.        */
typedef struct {
  const float* x; const float* dpre; const float* w; float* dw; float* db; const float* pre_prev; float* dprev;
  int32_t x_pitch, dpre_pitch, prev_pitch, rows, K;
} s2p_mlp_bwd_group;
int s2p_mlp_linear_bwd(const s2p_mlp_bwd_group* groups, int G, int N, int act_prev, void* stream);
/* Fused IQL critic head (iql_trainer.py:232-257, 309-314), every tensor fp32 [B] contiguous, one launch:
 *   q_target = reward_scale * reward + (1 - terminal) * discount * v_next
 *   losses[0..2] = mean (q1 - q_target)^2, mean (q2 - q_target)^2, mean w vf_err^2   with vf_err = v - min(tq1, tq2),
 *                  w = 1 - quantile where vf_err > 0, else quantile
 *   dq1, dq2, dv = d (losses[0] + losses[1] + losses[2]) / d (q1, q2, v)   (the 1 / B of the means included)
 *   adv = min(tq1, tq2) - v,  weights = min(exp(adv / beta), clip_score)   (pass +inf for no clip)
 * The eight inputs are required; every output is optional (at least one).  beta > 0.                                          */
int s2p_iql_critic_head(const float* q1, const float* q2, const float* tq1, const float* tq2, const float* v,
                        const float* v_next, const float* reward, const float* terminal, int B, float reward_scale,
                        float discount, float quantile, float beta, float clip_score, float* losses, float* dq1, float* dq2,
                        float* dv, float* weights, float* adv, float* q_target, void* stream);
/* Fused policy head: log-probability of TanhNormal at a GIVEN action and the advantage-weighted loss (iql_trainer.py:307-315,
 * rlkit/torch/distributions.py:339-354, gaussian_policy.py:119-123).  raw [B][raw_pitch >= 2 A] = (mu | raw log sigma):
 *   v = clamp(action, +-0.999999),  u = log(1 + v) / 2 - log(1 - v) / 2,  ls = clamp(raw log sigma, -20, 2)
 *   logp[b] = sum_d [-0.5 ((u - mu) / exp(ls))^2 - ls - 0.5 log 2 pi] - 2 sum_d [log 2 - u - softplus(-2 u)]
 *   loss[0] = mean_b (-logp[b] weights[b]);   draw [B][draw_pitch] = d loss / d raw  (zero for a raw log sigma outside [-20, 2])
 * softplus(x) = max(x, 0) + log1p(exp(-|x|)).  loss, draw, logp: each optional, at least one.                                */
int s2p_tanh_gauss_policy_head(const float* raw, int raw_pitch, const float* action, int action_pitch, const float* weights,
                               int B, int A, float* loss, float* draw, int draw_pitch, float* logp, void* stream);
/* Polyak update of flat fp32 buffers: target[i] = target[i] * (1 - tau) + source[i] * tau, each product and the sum rounded on
 * its own (torch's three element-wise operations: no fused multiply-add), 1 - tau formed in double and rounded once.  16-byte
 * groups with a one-by-one tail like s2p_adam_step: target and source 16-byte aligned, any n.                               */
int s2p_soft_update(float* target, const float* source, int64_t n, float tau, void* stream);

/* ---- CQL on SLAC latents (SPEC.md N3e; reference rlkit/torch/sac/cql_trainer.py:234-418, 576-585; the two further
 * s2p_mlp_linear_* entry points in csrc/mlp.hip, the sampling and the heads in csrc/cql.hip).
 * All fp32, no atomics, a fixed summation order (two identical calls give bitwise identical results).  Argument checking as
 * stated above s2p_gauss_head_fwd: negative sizes, a required NULL tensor, a short pitch and a misaligned operand are refused
 * before any launch; a size of 0 is a successful no-op that looks at no pointer.  Tensors with a pitch take the pointer already
 * offset to their first column.                                                                                            */
/* The input-gradient half of s2p_mlp_linear_bwd alone, for both of its forms:  dprev[m][k] = (sum_n dpre[m][n] w[n][k]) *
 * [pre_prev[m][k] > 0]  (act_prev = S2P_ACT_RELU; unmasked and pre_prev unused for S2P_ACT_NONE, the first layer), tile for tile
 * what s2p_mlp_linear_bwd writes (bitwise).  dpre, w and dprev are required; x, dw and db are IGNORED and may be NULL: nothing
 * but dprev is written, so a loss can be differentiated through a network down to its input (the SAC policy loss through qf1
 * and qf2 to the action columns) while the network's gradient buffers keep what they hold.                                */
int s2p_mlp_linear_dgrad(const s2p_mlp_bwd_group* groups, int G, int N, int act_prev, void* stream);
/* s2p_mlp_linear_bwd (its MFMA-tile form: N > 16) with the rows of each weight tile divided into S contiguous chunks of
 * ceil(ceil(rows / S) / 16) * 16 rows (the last one shorter; a chunk past the last row holds zeros): S waves per weight tile
 * where s2p_mlp_linear_bwd has one, each summing its rows in row order into partial s of the caller-owned workspace
 * ([S][dw [N][K] | db [N]] per group, groups in order); a second launch adds the partials in the order s = 0 .. S - 1 into dw /
 * db.  For layers run on many rows, where the weight tiles alone do not fill the chip and one wave per tile means a summation
 * chain as long as the batch.  S = 1 gives bitwise the result of s2p_mlp_linear_bwd; the input-gradient tiles are unchanged.
 * 1 <= S <= 64.  The library never allocates: the workspace holds at least s2p_mlp_linear_bwd_split_workspace bytes, else
 * the call is refused.  The query looks at sizes only -- rows, K, N, S -- and answers 0 for a NULL table and for G, N or S
 * outside what the call takes; pitches, pointers and alignment are the call's to check.                                  */
size_t s2p_mlp_linear_bwd_split_workspace(const s2p_mlp_bwd_group* groups, int G, int N, int S);
int s2p_mlp_linear_bwd_split(const s2p_mlp_bwd_group* groups, int G, int N, int act_prev, int S, void* workspace,
                             size_t workspace_bytes, void* stream);
/* ---- bf16 compute for the wide grouped layers (SPEC.md N3l): s2p_mlp_linear_fwd / _bwd / _dgrad / _bwd_split with the
 * products on the bf16 matrix cores.  Signatures, group tables and argument checks are those of the fp32 entry points; the
 * workspace of _bwd_split_bf16 is that of s2p_mlp_linear_bwd_split_workspace.
 *  - Every tensor stays fp32 in memory: x, w, bias, pre, act, dpre, dw, db, pre_prev, dprev.  Nothing is repacked and no shadow
 *    copy of the weights exists: a state_dict, Adam, the Polyak update and the loss heads see what they see with the fp32 entries.
 *  - Both operands of every product are rounded to bf16, round-to-nearest-even, when a tile loads them; the products are
 *    summed in fp32 on v_mfma_f32_32x32x16_bf16:
 *      pre   = sum_k bf16(x) bf16(w) + bias
 *      dw    = sum_m bf16(dpre) bf16(x)
 *      dprev = (sum_n bf16(dpre) bf16(w)) * [pre_prev > 0]
 *  - The bias add, ReLU, the mask and all stores are fp32.  db = sum_m dpre is an fp32 sum of the UNROUNDED values in the fp32
 *    kernel's order (bitwise the fp32 entry point's db).
 *  - The MFMA-tile form only: N <= 16 is refused before any launch (the narrow last layers keep the fp32 dot-product kernels).
 *  - K, x_pitch, N, dpre_pitch multiples of 4 and the operands 16-byte aligned, as for the fp32 entries, and no further demand:
 *    a step of 16 along the summation index that is partly past its end loads zeros.
 *  - No atomics, a fixed summation order: two identical calls give bitwise identical results.  _bwd_split_bf16 at S = 1 is bitwise
 *    _bwd_bf16; _dgrad_bf16 is tile for tile the dprev of _bwd_bf16.  The split chunks are the fp32 entry's multiples of 16 rows:
 *    one bf16 step of the weight tile.
 *  - A group with rows == 0 is skipped; a size of 0 is a successful no-op that looks at no pointer.                            */
int s2p_mlp_linear_fwd_bf16(const s2p_mlp_fwd_group* groups, int G, int N, int act, void* stream);
int s2p_mlp_linear_bwd_bf16(const s2p_mlp_bwd_group* groups, int G, int N, int act_prev, void* stream);
int s2p_mlp_linear_dgrad_bf16(const s2p_mlp_bwd_group* groups, int G, int N, int act_prev, void* stream);
int s2p_mlp_linear_bwd_split_bf16(const s2p_mlp_bwd_group* groups, int G, int N, int act_prev, int S, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* Reparameterised TanhNormal sample and its log-probability from the pre-tanh value (rlkit/torch/distributions.py:339-386).
 * raw [M][raw_pitch >= 2 A] = (mu | raw log sigma), eps [M * rep][eps_pitch >= A], rep >= 1.  For the row m * rep + r:
 *   ls = clamp(raw log sigma[m], -20, 2),  u = mu[m] + exp(ls) * eps,  action = tanh(u),
 *   logp = sum_d [-0.5 eps^2 - ls - 0.5 log 2 pi] - 2 sum_d [log 2 - u - softplus(-2 u)]
 * (log 2 the fp32 constant, softplus(x) = max(x, 0) + log1p(exp(-|x|)) as in s2p_tanh_gauss_policy_head).
 *   action: row m * action_group + r of a buffer of pitch action_pitch, A columns written and no other -- with the pointer offset
 *           to the action columns of a Q-input buffer, the samples land where the critics read them; action_group >= rep is the
 *           number of buffer rows per m (rep: compact; 3 rep: one of three column blocks of a [M][3 rep] row group)
 *   logp  : element m * logp_group + r (logp_group >= rep);   u [M * rep][u_pitch].   Each optional, at least one.
 * rep lets the policy trunk run on M rows where the reference runs it on M * rep repeated rows.                            */
int s2p_tanh_gauss_rsample(const float* raw, int raw_pitch, const float* eps, int eps_pitch, int M, int A, int rep,
                           float* action, int action_pitch, int action_group, float* logp, int logp_group, float* u,
                           int u_pitch, void* stream);
/* Its backward at rep = 1, from dlogp [M] and the optional daction, daction2 [M][daction_pitch] (added: the action's gradient
 * arrives once from each critic; daction2 needs daction) to draw [M][draw_pitch >= 2 A]:
 *   du = (daction + daction2) (1 - tanh^2 u) + dlogp 2 tanh u,   d mu = du,
 *   d raw log sigma = (du exp(ls) eps - dlogp) * [-20 <= raw log sigma <= 2]    (torch.clamp passes the gradient on [min, max])
 * accumulate == 0: draw is overwritten; != 0: added to (the behaviour-cloning branch adds to what
 * s2p_tanh_gauss_policy_head wrote with unit weights).                                                                    */
int s2p_tanh_gauss_rsample_bwd(const float* raw, int raw_pitch, const float* eps, int eps_pitch, const float* dlogp,
                               const float* daction, const float* daction2, int daction_pitch, int M, int A, float* draw,
                               int draw_pitch, int accumulate, void* stream);
/* Fused SAC policy head with the entropy-temperature step (cql_trainer.py:263-292), one launch of one workgroup, no host
 * synchronisation.  logp [B]; q1, q2 [B] optional (together); log_alpha_state [3] = (log_alpha, Adam m, Adam v) and step_dev
 * [1] in device memory.  In this order:
 *   1. tune != 0: alpha_loss = -mean(log_alpha (logp + target_entropy)); ONE Adam step on log_alpha from that gradient (taken
 *      at the old log_alpha; the arithmetic of s2p_adam_step_dev, the counter incremented first)
 *   2. alpha[0] = exp(log_alpha) AFTER the step (tune == 0: alpha[0] = 1, alpha_loss = 0, the state is not looked at)
 *   3. losses[0..3] = alpha_loss, mean(alpha logp - min(q1, q2)), mean(alpha logp), mean(logp - min(q1, q2)) -- the SAC policy
 *      loss, its entropy part alone (the behaviour-cloning loss adds s2p_tanh_gauss_policy_head's to it) and the reference's
 *      'Policy Loss' statistic, which leaves alpha out (cql_trainer.py:600).  With q1 == NULL the min term is 0.
 *   4. dlogp [B] = alpha / B
 *   5. dq1, dq2 [B] = -1 / B to the smaller of q1, q2 and 0 to the other; on a tie -1 / (2 B) to each, as the backward of
 *      torch.min(a, b) splits it.
 * losses, dlogp, dq1, dq2: each optional.                                                                                 */
int s2p_sac_policy_head(const float* logp, const float* q1, const float* q2, int B, int tune, float target_entropy, float lr,
                        float beta1, float beta2, float eps, float* log_alpha_state, int* step_dev, float* alpha,
                        float* losses, float* dlogp, float* dq1, float* dq2, void* stream);
/* Fused CQL critic head (cql_trainer.py:303-398, min_q_version 3), one launch of one workgroup, any B.  Network i of a
 * two-network tensor lies i * its stride (in elements) behind network 0:
 *   q_pred [2][B];  q_samp [2][B][3 R], column blocks random | next | current;  logp_samp [B][2 R] = next | current;
 *   tq [2][B] contiguous (the target networks at the next latent and action);  new_log_pi, reward, terminal [B];  alpha [1].
 *   q_target = reward_scale reward + (1 - terminal) discount (min(tq1, tq2) - alpha new_log_pi)   (deterministic_backup != 0:
 *              without the alpha term; new_log_pi and alpha may then be NULL)
 *   cat_i = [random - log 0.5^A | next - logp_next | current - logp_current] / temp,   lse max-shifted
 *   min_qf_i = mean_b lse(cat_i) min_q_weight temp - mean(q_pred_i) min_q_weight;   qf_i = mean (q_pred_i - q_target)^2 + min_qf_i
 * Outputs, each optional, at least one:  losses [4] = qf1, qf2, min_qf1, min_qf2;  dq_pred [2][B] = d (qf1 + qf2) / d q_pred;
 * dq_samp [2][B][3 R] = softmax(cat_i) min_q_weight / B;  q_target [B];  std_mean [2] = mean_b of the unbiased standard
 * deviation of (random, q_pred, next, current) per row (the 'Std QF values' statistics).  temp > 0, R >= 1.               */
int s2p_cql_critic_head(const float* q_pred, int64_t q_pred_stride, const float* q_samp, int64_t q_samp_stride,
                        const float* logp_samp, const float* tq, const float* new_log_pi, const float* alpha,
                        const float* reward, const float* terminal, int B, int R, int A, float reward_scale, float discount,
                        float temp, float min_q_weight, int deterministic_backup, float* losses, float* dq_pred,
                        int64_t dq_pred_stride, float* dq_samp, int64_t dq_samp_stride, float* q_target, float* std_mean,
                        void* stream);

/* ---- the acting step of a SLAC policy (SPEC.md N3f; reference rlkit/torch/slac/trainer.py:12-47, slac/algo.py:75-81,
 * rlkit/samplers/rollout_functions.py:127-205; csrc/actor.hip).  All fp32 (the frame conversion writes bf16 too), no atomics, a
 * fixed summation order.  Argument checking as stated above s2p_gauss_head_fwd: negative sizes, a required NULL pointer, a short
 * pitch and a misaligned operand are refused before any launch; a size of 0 is a successful no-op that looks at no pointer.    */
/* uint8 frames [N][C][H][W], the layout an environment hands out, -> the encoder's NHWC input [N][H][W][y_pitch] in fp32 or bf16:
 * channels < C hold float(x) / 255.0f, a true IEEE division (torch's `.float().div_(255.0)` bit for bit in fp32, that value
 * rounded to nearest-even in bf16); channels C .. y_pitch - 1 are exactly 0.  H * W % 4 == 0 with a 4-byte aligned x reads
 * dwords, anything else bytes.  N <= 65535.                                                                                */
int s2p_u8_chw_to_nhwc01(int dtype, const void* x, int N, int C, int H, int W, void* y, int y_pitch, void* stream);
/* The policy-input rows as the observation state of N environments.  Row n of src / dst [N][pitch] is
 * [f_0 .. f_{S-1} | a_0 .. a_{S-2} | 0 pad]: S F + (S - 1) A values, pitch a multiple of 4 floats (`SlacAlgorithm.preprocess`'s
 * layout).  dst is written from src, feat [N][feat_pitch >= F], action [N][action_pitch >= A] and the row's reset code:
 *   reset[n] == 0 (or reset == NULL): features shifted left by F with feat[n] last, actions shifted left by A with action[n] last
 *                                     (`SlacObservation.append`)
 *   reset[n] == 1: S - 1 copies of fill [F], then feat[n]; all actions 0   (`reset_episode`; fill = the feature of a zero frame)
 *   reset[n] == 2: S copies of feat[n]; all actions 0                      (`reset_w_same_obs=True`)
 * Pad columns are written as 0.  src is not modified and may not overlap dst (the caller ping-pongs two buffers); both 16-byte
 * aligned.  action is not looked at for rows with a reset code.  N <= 65535.                                                */
int s2p_feature_action_push(const float* src, float* dst, int pitch, int N, int S, int F, int A, const float* feat,
                            int feat_pitch, const float* action, int action_pitch, const int32_t* reset, const float* fill,
                            void* stream);
/* s2p_mlp_linear_fwd -- the same group table, activations and contract -- for rows <= 16 in every group (a larger group is
 * refused before any launch), any N: one wave per output column reads its weight row once (lane l the k = 4 l .. 4 l + 3 of
 * every 256, in k order), keeps one fused-multiply-add accumulator per row and reduces each in the same 64-lane butterfly.  N
 * waves whatever the row count, each weight byte read once, no LDS.  ROW INVARIANCE: the value of a row does not depend on how
 * many other rows the launch has (bitwise), so a batch of environments computes what each environment alone computes.  Not
 * bitwise s2p_mlp_linear_fwd's result (another summation order).                                                            */
int s2p_mlp_linear_fwd_skinny(const s2p_mlp_fwd_group* groups, int G, int N, int act, void* stream);

/* ---- optimizer + weight packing ---------------------------------------------------- */
/* torch.optim.Adam step on flat fp32 buffers; g is multiplied by grad_scale first.  All three forms move 16-byte groups:
 * p, g, m, v must be 16-byte aligned (a sub-range of a flat buffer starts at a multiple of 4 elements), else the call is
 * refused; n need not be a multiple of 4 (the last 1..3 elements go one by one); n == 0 is a no-op (no tick either).  */
int s2p_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                  float beta2, float eps, int step, float grad_scale, void* stream);
/* same update with the step counter in DEVICE memory (incremented on the device first), so the launch
 * can be captured in a hipGraph and replayed                                             */
int s2p_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                      float beta2, float eps, int* step_dev, float grad_scale, void* stream);
/* the same update of a RANGE of a flat buffer; tick != 0 increments the device step counter first.  One optimizer step
 * applied in several launches (the first with tick = 1, the others with tick = 0: they read the counter the first one
 * wrote, so order them behind it) -- e.g. the part of a gradient buffer that is final early, under the rest of the backward */
int s2p_adam_step_dev_part(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                           float beta2, float eps, int* step_dev, float grad_scale, int tick, void* stream);
/* one packing job: src fp32 [R][T][C] (channels-last master weight: R rows, T taps, C
 * channels) -> dst_fwd[r][t][c] (row length T*Cpad, zero pad c>=C)  and/or
 * dst_bwd[c][t][r_off + r] (row length T*Rrow; untouched elements must be pre-zeroed)    */
typedef struct {
  const float* src; void* dst_fwd; void* dst_bwd;
  int32_t R, T, C;
  int32_t Cpad;        /* fwd: padded channel count                                     */
  int32_t Rrow;        /* bwd: row length (in r) of the transposed matrix               */
  int32_t r_off;       /* bwd: column offset of this job inside a fused matrix          */
  int32_t dtype;
} s2p_pack_job;
/* jobs: DEVICE array of n_jobs descriptors (caller-owned)                               */
int s2p_pack_weights(const s2p_pack_job* jobs, int n_jobs, int max_elems, void* stream);
/* the same packing with a per-job scale: sigma is a DEVICE array of n_jobs pointers to device fp32 scalars; job i packs
 * src / *sigma[i] (an fp32 division, then the dtype's round-to-nearest-even cast), or src unscaled where sigma[i] is
 * NULL (the spectral-norm operands W / sigma, SPEC.md D5s)                                                           */
int s2p_pack_weights_scaled(const s2p_pack_job* jobs, const float* const* sigma, int n_jobs, int max_elems,
                            void* stream);

/* ---- spectral normalization (torch.nn.utils.spectral_norm: one power iteration, eps 1e-12; SPEC.md D5s) ------ */
/* one SN weight: w fp32 master [R][K] (K = taps * channels, in the master's (tap, channel) column order); u [R],
 * v [K] and sigma [1] are updated in place; ws: caller-owned fp32 workspace of s2p_sn_workspace_floats(R, K) floats,
 * one per job; grad [R][K]: the projection's operand (NULL for the power iteration)                                 */
typedef struct {
  const float* w; float* u; float* v; float* sigma; float* ws; float* grad;
  int32_t R, K;
} s2p_sn_job;
int64_t s2p_sn_workspace_floats(int R, int K);
/* jobs: DEVICE array of n_jobs descriptors; max_R / max_K bound every job's R / K (they size the grid).
 * training != 0: v = normalize(W^T u), u = normalize(W v), sigma = u . (W v)  (3 launches);
 * training == 0: u and v untouched, sigma = u . (W v) (2 launches).  No atomics, fixed summation order: a job's
 * results are bitwise independent of the other jobs in the table and reproducible call to call                     */
int s2p_sn_power_iter(const s2p_sn_job* jobs, int n_jobs, int max_R, int max_K, int training, void* stream);
/* grad <- (grad - <grad, w / sigma> u v^T) / sigma in place: dL/dW from dL/dW_sn with u, v held constant
 * (2 launches: per-row-block partials of <grad, w>, then the apply)                                                 */
int s2p_sn_project_grad(const s2p_sn_job* jobs, int n_jobs, int max_R, int max_K, void* stream);

/* ---- small elementwise helpers ------------------------------------------------------ */
/* dx = dy * act'(y)   (y = activation OUTPUT; act none / relu / lrelu / tanh -- swish' cannot be formed from the
 * output: S2P_ACT_SWISH and unknown ids are refused, as they are for aux_act of s2p_conv2d_dgrad) */
int s2p_act_bwd(int dtype, const void* dy, const void* y, int64_t n, int act, float slope, void* dx,
                void* stream);
/* x *= *scale  (device fp32 scalar: applies an upstream grad_output without a host sync) */
int s2p_scale(int dtype, void* x, int64_t n, const float* scale, void* stream);
/* out = a + b (n elements; out may alias a or b)                                         */
int s2p_add(int dtype, const void* a, const void* b, void* out, int64_t n, void* stream);
/* dst[p][dst_off+c] (+)= src[p][src_off+c] for c<C, p<pixels  (torch.cat(dim=1) on NHWC and
 * its backward slice); src_off + C <= src_pitch and dst_off + C <= dst_pitch             */
int s2p_copy_channels(int dtype, const void* src, int src_pitch, int src_off, void* dst,
                      int dst_pitch, int dst_off, int C, int64_t pixels, int accumulate, void* stream);

/* ---- image-fidelity metrics (the paper's PSNR / SSIM, rebuttal.md:50 -- no reference code) ----
 * a, b: fp32 NCHW [N,C,H,W].  sq_err_sum[n] += sum over the image of (a-b)^2;  ssim_sum[n] += sum over channels and
 * over the (H-10)x(W-10) fully covered positions of the 11x11 Gaussian-window (sigma 1.5) SSIM index with
 * C1 = (0.01 R)^2, C2 = (0.03 R)^2, R = data_range.  Both accumulators are caller-zeroed fp32 [N].
 * PSNR = 10 log10(R^2 C H W / sq_err_sum);  SSIM = ssim_sum / (C (H-10) (W-10)).  Requires H, W >= 11.            */
int s2p_image_metrics(const float* a, const float* b, int N, int C, int H, int W, float data_range,
                      float* sq_err_sum, float* ssim_sum, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
