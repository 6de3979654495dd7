// The state path: positional encoding -> 4 x (Linear + LeakyReLU) -> per-norm affine
// Linear(256 -> 12*2C), all fp32, M = batch (64) rows.  0.6 MFLOP per image: these layers are LATENCY-bound, and the
// generic implicit-GEMM conv kernel spends ~45 us per layer on them (2 workgroups, a 16..23-step staged K loop).
// Here a layer is one short launch of many small workgroups, on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: fp32 operands,
// fp32 accumulate), operands straight from global memory into the MFMA registers -- NO LDS at all (round 3; the LDS-staged
// VALU form these replaced took ~20 us per layer, and it was the kernel family the LDS co-residency hazard of DESIGN.md
// section 4 was found on: a kernel without LDS accesses is outside that class by construction):
//   forward / dgrad : y[M][N] = f(x)[M][Kr] . W[N][Kr]^T (+ bias, activation)   a wave owns a 16 x 16 tile, a workgroup the
//                     four 16-row tiles of a 64-row block (they share the W rows); optional split of the reduction Kr over
//                     blockIdx.z with partial tiles in a workspace and a fixed-order reduce (the 6144-deep dgrad of the
//                     affine layer);
//   wgrad (+ bias)  : dW[N][K] += sum_m dpre[m][n] x[m][k]                       a wave owns 16 n x 16 k, loop over the batch;
// where f / dpre fold the LeakyReLU derivative of the layer's saved OUTPUT into the operand staging, so the backward of a
// layer is two short launches (wgrad + bias grad; dgrad) -- no act_bwd pass, no atomics, fixed summation order.
// (One launch per layer, not one per chain: a layer needs every output COLUMN of the previous one, and on this chip a kernel
// boundary (~1.5 us, hipGraph) is cheaper than an in-kernel grid barrier (~4-7 us).  That holds wherever the rows of a layer are
// spread over workgroups: the state path, and the SLAC posterior chain as it runs by default.  The chain's batch rows never meet, so
// it can also give a workgroup 16 rows and ALL columns and then needs workgroup barriers only: gauss_chain.hip runs the no-grad
// chains as one launch, and with LatentModel.fused_chain_grad the chain under grad as one launch forward and one backward, whose
// dgrad elements are this file's lin_fwd_kernel through lin_dgrad_args, bit for bit.)
//
// The SLAC Gaussian MLPs' variant of a layer is here too (s2p_linear_add_fwd / s2p_linear_add_bwd): the same forward kernel with an
// additive [M][N] term in its epilogue, y = act(f(x) . W^T + add + bias).  The part of a first layer's pre-activation that does not
// depend on the posterior chain (features, actions) is ONE batched GEMM before the chain and comes in as `add`; in the dgrad `add` is
// the gradient already accumulated at the destination.  lin_actgrad_kernel (dpre = dy * act'(y)) is the additive term's gradient,
// and the operand of the batched weight gradient that runs once after the chain.  There is ONE forward tile: s2p_linear_fwd and
// s2p_linear_add_fwd with add == NULL are the same launch, and the fused chain (gauss_chain.hip) promises the bits of both.
#include "gauss_dev.h"

struct LinArgs {
  const float* x; const float* xact; const float* w; const float* bias; const float* add; float* y; float* part;
  // backward extras
  const float* dy; const float* yact; const float* xin; float* dw; float* db;
  int M, Kr, N, x_pitch, xact_pitch, w_row, add_pitch, y_pitch, n_store;
  int act, in_act; float slope;
  int ksplit, k_per_split;
  // wgrad
  int K, xin_pitch, dy_pitch, yact_pitch, dw_row, k_real;
};

// y tile of  act(x'[M][Kr] . W[N][Kr]^T + add + bias),  x' = x * act'(xact) when xact != nullptr.
// MFMA 16x16x4 f32 operand layout: lane l = 16 j + i holds A[row i][k j] and B[k j][col i]; the result register r of lane l is
// D[row 4 j + r][col i].  A k-chunk of 16 is loaded as ONE float4 per lane and operand (lane group j takes k = 16 t + 4 j .. + 3)
// and consumed by four MFMAs (MFMA e uses component e: the same k permutation on both operands, so the sum is the plain dot
// product).  U chunks are loaded before the first MFMA: 2 U (3 U with xact) independent 16-byte loads in flight per lane.
// Epilogue: (acc + add[m][n]) + bias, then the activation -- additions only, nothing a compiler could contract into a fused
// multiply-add.  y may be the same buffer as add (the accumulating dgrad): every element is read and written by one lane.  With
// ksplit > 1 the tile of split z goes to the workspace as it is (no add, bias or activation: the host never asks for those there).
#ifndef S2P_LIN_U
#define S2P_LIN_U 8
#endif
__global__ __launch_bounds__(256) void lin_fwd_kernel(const LinArgs a) {
  constexpr int U = S2P_LIN_U;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, j = lane >> 4;
  const int nb = blockIdx.x * 16, mb = blockIdx.y * 64 + wave * 16, z = blockIdx.z;
  if (mb >= a.M) return;                                   // (wave-uniform)
  // in_act is none / relu / lrelu, the backward entry points refuse every other id: spares act_grad_from_out's tanh arithmetic per
  // operand element
  __builtin_assume(a.in_act >= S2P_ACT_NONE && a.in_act <= S2P_ACT_LRELU);
  const int k0 = z * a.k_per_split, k1 = k0 + a.k_per_split < a.Kr ? k0 + a.k_per_split : a.Kr;
  const int m = mb + i, n = nb + i;
  const bool mok = m < a.M, nok = n < a.N;
  const float* xr = a.x + (size_t)(mok ? m : 0) * a.x_pitch;
  const float* ar = a.xact ? a.xact + (size_t)(mok ? m : 0) * a.xact_pitch : nullptr;
  const float* wr = a.w + (size_t)(nok ? n : 0) * a.w_row;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int kc = k0; kc < k1; kc += 16 * U) {
    f32x4 xv[U], wv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = kc + 16 * u + 4 * j;                   // Kr, k_per_split and the pitches are multiples of 4: a float4 is in or out
      xv[u] = (mok && k < k1) ? *(const f32x4*)(xr + k) : (f32x4){0.f, 0.f, 0.f, 0.f};
      wv[u] = (nok && k < k1) ? *(const f32x4*)(wr + k) : (f32x4){0.f, 0.f, 0.f, 0.f};
      if (ar && mok && k < k1) {
        const f32x4 yv = *(const f32x4*)(ar + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) xv[u][e] *= act_grad_from_out(yv[e], a.in_act, a.slope);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) acc = lin_mfma_chunk(xv[u], wv[u], acc);
  }
  if (n >= a.n_store) return;
  const float b = (a.bias && nok && a.ksplit <= 1) ? a.bias[n] : 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int mo = mb + 4 * j + r;
    if (mo >= a.M) continue;
    if (a.ksplit > 1) { a.part[((size_t)z * a.M + mo) * a.n_store + n] = acc[r]; continue; }   // partial tile -> workspace [z][M][n_store]
    float v = 0.f;                                         // columns [N, n_store): zeros
    if (nok) {
      v = acc[r];
      if (a.add) v += a.add[(size_t)mo * a.add_pitch + n];
      v = act_fwd(v + b, a.act, a.slope);
    }
    a.y[(size_t)mo * a.y_pitch + n] = v;
  }
}

// y[m][n] = sum over the K splits, in split order
__global__ __launch_bounds__(256) void lin_splitk_reduce_kernel(const LinArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)a.M * a.n_store) return;
  const int m = (int)(i / a.n_store), n = (int)(i - (long long)m * a.n_store);
  float s = 0.f;
  for (int z = 0; z < a.ksplit; ++z) s += a.part[((size_t)z * a.M + m) * a.n_store + n];
  a.y[(size_t)m * a.y_pitch + n] = s;
}

// dW[N][K] += dpre^T x, db[N] += sum_m dpre   (dpre = dy * act'(y)).  D[n][k] = sum_m A[n][m] B[m][k]: per MFMA (4 batch rows)
// a lane loads ONE dpre value and ONE x value (16 lanes = 64 contiguous bytes of a row); the bias gradient is a second MFMA
// against a column of ones (no cross-lane reduction).  All of a 64-row batch's loads are in flight before the first MFMA.
__global__ __launch_bounds__(256) void lin_wgrad_kernel(const LinArgs a) {
  constexpr int U = 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, j = lane >> 4;
  const int kt_n = (a.K + 63) / 64;
  const int nb = (blockIdx.x / kt_n) * 16, kb = (blockIdx.x % kt_n) * 64 + wave * 16;
  if (kb >= a.K) return;                                   // (wave-uniform)
  __builtin_assume(a.act >= S2P_ACT_NONE && a.act <= S2P_ACT_LRELU);         // (as in lin_fwd_kernel: every other id is refused)
  const int n = nb + i, k = kb + i;
  const bool nok = n < a.N, kok = k < a.K;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};
  const bool want_b = a.db && kb == 0;
  for (int m0 = 0; m0 < a.M; m0 += 4 * U) {
    float dv[U], xv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int m = m0 + 4 * u + j;
      const bool mok = m < a.M;
      dv[u] = (mok && nok) ? a.dy[(size_t)m * a.dy_pitch + n] : 0.f;
      if (a.yact && mok && nok) dv[u] *= act_grad_from_out(a.yact[(size_t)m * a.yact_pitch + n], a.act, a.slope);
      xv[u] = (mok && kok) ? a.xin[(size_t)m * a.xin_pitch + k] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[u], xv[u], acc, 0, 0, 0);
      if (want_b) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[u], 1.f, accb, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int no = nb + 4 * j + r;
    if (no >= a.N) continue;
    if (k < a.k_real) a.dw[(size_t)no * a.dw_row + k] += acc[r];
    if (want_b && i == 0) a.db[no] += accb[r];
  }
}

// ---- host side: ONE place fills the forward arguments, ONE turns a backward call into them, ONE launches ---------------------------
// y[M][y_pitch] = act(x[M][Kr] . w[N][w_row]^T + add + bias), columns [N, n_store) zero; add and bias may be nullptr
static LinArgs lin_fwd_args(const float* x, int x_pitch, int M, int Kr, const float* w, int w_row, const float* bias, int N,
                            const float* add, int add_pitch, int act, float slope, float* y, int y_pitch, int n_store) {
  LinArgs a{}; a.x = x; a.x_pitch = x_pitch; a.M = M; a.Kr = Kr; a.w = w; a.w_row = w_row; a.bias = bias; a.N = N; a.add = add;
  a.add_pitch = add_pitch; a.act = act; a.slope = slope; a.y = y; a.y_pitch = y_pitch; a.n_store = n_store;
  a.ksplit = 1; a.k_per_split = Kr;
  return a;
}

// dx columns a dgrad writes: K rounded up to 4 (the padding columns as zeros) where the row has room for them, else K
static inline int lin_dx_cols(int K, int dx_pitch) { const int kcols = (K + 3) / 4 * 4; return kcols <= dx_pitch ? kcols : K; }

// The input gradient as a forward: "x" = dy with the activation derivative of the saved output y folded in (ya = nullptr: none),
// reduction over N, output columns = the K inputs, weights = the transpose.  accumulate: dx += (add = dx itself, exactly K columns).
static LinArgs lin_dgrad_args(const float* dy, int dy_pitch, const float* ya, int y_pitch, int M, int N, const float* w_bwd, int wb_row,
                              int K, int act, float slope, float* dx, int dx_pitch, bool accumulate) {
  LinArgs g = lin_fwd_args(dy, dy_pitch, M, N, w_bwd, wb_row, nullptr, K, accumulate ? dx : nullptr, dx_pitch, S2P_ACT_NONE, slope, dx,
                           dx_pitch, accumulate ? K : lin_dx_cols(K, dx_pitch));
  g.xact = ya; g.xact_pitch = y_pitch; g.in_act = act;
  return g;
}

// ks > 1: the reduction in about ks parts (multiples of 64), partial tiles in `part` [ksplit][M][n_store], then the fixed-order reduce
static int lin_fwd_launch(LinArgs a, float* part, int ks, hipStream_t st) {
  if (ks > 1) { a.part = part; a.k_per_split = (cdiv(a.Kr, ks) + 63) / 64 * 64; a.ksplit = cdiv(a.Kr, a.k_per_split); }
  hipLaunchKernelGGL(lin_fwd_kernel, dim3(cdiv(a.n_store, 16), cdiv(a.M, 64), a.ksplit), dim3(256), 0, st, a);
  S2P_CHECK_LAUNCH("lin_fwd_kernel");
  if (a.ksplit > 1) {
    hipLaunchKernelGGL(lin_splitk_reduce_kernel, dim3(cdiv((long long)a.M * a.n_store, 256)), dim3(256), 0, st, a);
    S2P_CHECK_LAUNCH("lin_splitk_reduce_kernel");
  }
  return 0;
}

static int lin_check(const char* who, int M, int K, int N, int xp) {
  if (M < 0 || K <= 0 || N <= 0) S2P_FAIL(-1, "%s: empty problem", who);
  if (K % 4 || xp % 4) S2P_FAIL(-1, "%s: K and pitches must be multiples of 4 floats", who);
  return 0;
}

// y[M][y_pitch] = act(x[M][K] . w[N][w_row]^T + bias); columns [N, n_store) are written as zeros (channel padding)
extern "C" int s2p_linear_fwd(const float* x, int M, int K, int x_pitch, const float* w, int w_row, const float* bias, int N,
                              int act, float slope, float* y, int y_pitch, int n_store, void* stream) {
  if (M == 0) return 0;                                    // an empty batch: a no-op that looks at no pointer
  int rc = lin_check("s2p_linear_fwd", M, K, N, x_pitch); if (rc) return rc;
  if (!x || !w || !y || w_row % 4 || n_store < N || n_store > y_pitch) S2P_FAIL(-1, "s2p_linear_fwd: bad arguments");
  if (act < S2P_ACT_NONE || act > S2P_ACT_SWISH) S2P_FAIL(-1, "s2p_linear_fwd: unknown activation %d", act);
  return lin_fwd_launch(lin_fwd_args(x, x_pitch, M, K, w, w_row, bias, N, nullptr, 0, act, slope, y, y_pitch, n_store), nullptr, 1,
                        (hipStream_t)stream);
}

extern "C" size_t s2p_linear_bwd_workspace(int M, int K, int N) {
  const int ks = N >= 2048 ? cdiv(N, 512) : 1;
  return ks > 1 ? (size_t)ks * M * ((K + 3) / 4 * 4) * sizeof(float) : 0;
}

// Backward of y = act(x . w^T + b) given dy = dL/dy and the layer's OUTPUT y (act != NONE):
//   dw[N][dw_row] += dpre^T x (columns < k_real), db[N] += sum_m dpre, dx[M][dx_pitch] = dpre . w  (dx may be NULL),
// dpre = dy * act'(y).  w_bwd: [K][wb_row] = the transpose of w (row k holds w[:, k]).
extern "C" int s2p_linear_bwd(const float* x, int x_pitch, const float* dy, int dy_pitch, const float* y, int y_pitch, int M,
                              int K, int k_real, int N, const float* w_bwd, int wb_row, int act, float slope, float* dw,
                              int dw_row, float* db, float* dx, int dx_pitch, void* workspace, size_t workspace_bytes,
                              void* stream) {
  if (M == 0) return 0;                                    // an empty batch: nothing to add to dw / db, no row of dx
  int rc = lin_check("s2p_linear_bwd", M, K, N, x_pitch); if (rc) return rc;
  if (!x || !dy || !dw || dy_pitch % 4 || N % 4) S2P_FAIL(-1, "s2p_linear_bwd: bad arguments (N and pitches must be multiples of 4)");
  if (act != S2P_ACT_NONE && act != S2P_ACT_RELU && act != S2P_ACT_LRELU)      // (as s2p_linear_add_bwd)
    S2P_FAIL(-1, "s2p_linear_bwd: activation %d has no backward here (none / relu / lrelu only)", act);
  if (act != S2P_ACT_NONE && (!y || y_pitch % 4)) S2P_FAIL(-1, "s2p_linear_bwd: the activation output is needed");
  if (dx && (!w_bwd || wb_row % 4)) S2P_FAIL(-1, "s2p_linear_bwd: dx needs w_bwd");
  // the split-K input gradient's geometry and its workspace, settled before anything is launched
  const int ks = N >= 2048 ? cdiv(N, 512) : 1;
  const size_t need = (size_t)ks * M * lin_dx_cols(K, dx_pitch) * sizeof(float);
  if (dx && ks > 1 && (!workspace || workspace_bytes < need)) S2P_FAIL(-1, "s2p_linear_bwd: workspace of %zu bytes needed", need);
  hipStream_t st = (hipStream_t)stream;
  const float* ya = act != S2P_ACT_NONE ? y : nullptr;
  LinArgs a{};                                             // the weight (+ bias) gradient
  a.M = M; a.act = act; a.slope = slope; a.xin = x; a.xin_pitch = x_pitch; a.dy = dy; a.dy_pitch = dy_pitch; a.yact = ya;
  a.yact_pitch = y_pitch; a.dw = dw; a.dw_row = dw_row; a.db = db; a.K = K; a.k_real = k_real; a.N = N;
  hipLaunchKernelGGL(lin_wgrad_kernel, dim3(cdiv(N, 16) * cdiv(K, 64)), dim3(256), 0, st, a);
  S2P_CHECK_LAUNCH("lin_wgrad_kernel");
  if (!dx) return 0;
  return lin_fwd_launch(lin_dgrad_args(dy, dy_pitch, ya, y_pitch, M, N, w_bwd, wb_row, K, act, slope, dx, dx_pitch, false),
                        (float*)workspace, ks, st);
}

// ---- the same layer with an additive term (the SLAC Gaussian MLPs) ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void lin_actgrad_kernel(const float* dy, int dy_pitch, const float* y, int y_pitch, int M, int N,
                                                          int act, float slope, float* out, int out_pitch) {
  const long long total = (long long)M * N;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int m = (int)(idx / N), n = (int)(idx - (long long)m * N);
    float v = dy[(size_t)m * dy_pitch + n];
    if (y) v *= act_grad_from_out(y[(size_t)m * y_pitch + n], act, slope);
    out[(size_t)m * out_pitch + n] = v;
  }
}

// What these two entry points refuse of a forward launch and s2p_linear_fwd / s2p_linear_bwd do not, in the launch's own terms
// (for the dgrad "x" is dy, "K" the reduction over N and "N" the K inputs)
static int lin_add_check(const char* who, const LinArgs& a) {
  S2P_REQUIRE(a.Kr % 4 == 0 && a.x_pitch % 4 == 0 && a.w_row % 4 == 0 && a.x_pitch >= a.Kr && a.w_row >= a.Kr,
              "%s: K, x_pitch and w_row must be multiples of 4 floats, the pitches at least K", who);
  S2P_REQUIRE(s2p_al16(a.x) && s2p_al16(a.w) && (!a.xact || (s2p_al16(a.xact) && a.xact_pitch % 4 == 0 && a.xact_pitch >= a.Kr)),
              "%s: x, w (and the activation output) must be 16-byte aligned", who);
  S2P_REQUIRE(a.n_store >= a.N && a.n_store <= a.y_pitch, "%s: N <= n_store <= y_pitch is required", who);
  S2P_REQUIRE(!a.add || a.add_pitch >= a.N, "%s: add_pitch is below N", who);
  return 0;
}

extern "C" int s2p_linear_add_fwd(const float* x, int M, int K, int x_pitch, const float* w, int w_row, const float* bias, int N,
                                  const float* add, int add_pitch, int act, float slope, float* y, int y_pitch, int n_store,
                                  void* stream) {
  S2P_REQUIRE(M >= 0 && K >= 0 && N >= 0, "s2p_linear_add_fwd: negative size");
  if (M == 0 || N == 0) return 0;
  S2P_REQUIRE(K > 0, "s2p_linear_add_fwd: empty reduction");
  S2P_REQUIRE(x && w && y, "s2p_linear_add_fwd: null pointer");
  S2P_REQUIRE(act >= S2P_ACT_NONE && act <= S2P_ACT_SWISH, "s2p_linear_add_fwd: unknown activation %d", act);
  const LinArgs a = lin_fwd_args(x, x_pitch, M, K, w, w_row, bias, N, add, add_pitch, act, slope, y, y_pitch, n_store);
  int rc = lin_add_check("s2p_linear_add_fwd", a); if (rc) return rc;
  return lin_fwd_launch(a, nullptr, 1, (hipStream_t)stream);
}

extern "C" int s2p_linear_add_bwd(const float* x, int x_pitch, const float* dy, int dy_pitch, const float* y, int y_pitch, int M,
                                  int K, int k_real, int N, const float* w_bwd, int wb_row, int act, float slope, float* dw,
                                  int dw_row, float* db, float* dx, int dx_pitch, int dx_accumulate, float* dadd, int dadd_pitch,
                                  void* stream) {
  S2P_REQUIRE(M >= 0 && K >= 0 && N >= 0, "s2p_linear_add_bwd: negative size");
  if (M == 0 || N == 0 || K == 0) return 0;
  S2P_REQUIRE(dy && dy_pitch >= N, "s2p_linear_add_bwd: dy is NULL or its pitch is below N");
  S2P_REQUIRE(act == S2P_ACT_NONE || act == S2P_ACT_RELU || act == S2P_ACT_LRELU,
              "s2p_linear_add_bwd: activation %d has no backward here (none / relu / lrelu only)", act);
  S2P_REQUIRE(act == S2P_ACT_NONE || (y && y_pitch >= N), "s2p_linear_add_bwd: the activation output is needed");
  S2P_REQUIRE(dw || dx || dadd, "s2p_linear_add_bwd: no output");
  S2P_REQUIRE(!dadd || dadd_pitch >= N, "s2p_linear_add_bwd: dadd_pitch is below N");
  S2P_REQUIRE(!dw || (x && dw_row >= k_real && k_real >= 0 && k_real <= K), "s2p_linear_add_bwd: dw needs x and k_real <= dw_row, K");
  S2P_REQUIRE(!db || dw, "s2p_linear_add_bwd: db is produced by the weight-gradient pass (dw is NULL)");
  S2P_REQUIRE(!dx || (w_bwd && dx_pitch >= K && N % 4 == 0 && dy_pitch % 4 == 0 && s2p_al16(dy)),
              "s2p_linear_add_bwd: dx needs w_bwd, dx_pitch >= K, N and dy_pitch multiples of 4, dy 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const float* ya = act != S2P_ACT_NONE ? y : nullptr;
  if (dadd) {
    const long long blocks = ((long long)M * N + 255) / 256;
    hipLaunchKernelGGL(lin_actgrad_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, st, dy, dy_pitch, ya, y_pitch, M,
                       N, act, slope, dadd, dadd_pitch);
    S2P_CHECK_LAUNCH("lin_actgrad_kernel");
  }
  if (dw) {
    int rc = s2p_linear_bwd(x, x_pitch, dy, dy_pitch, y, y_pitch, M, K, k_real, N, nullptr, 0, act, slope, dw, dw_row, db, nullptr, 0,
                            nullptr, 0, stream);
    if (rc) return rc;
  }
  if (dx) {
    const LinArgs g = lin_dgrad_args(dy, dy_pitch, ya, y_pitch, M, N, w_bwd, wb_row, K, act, slope, dx, dx_pitch, dx_accumulate != 0);
    int rc = lin_add_check("s2p_linear_add_bwd", g); if (rc) return rc;
    return lin_fwd_launch(g, nullptr, 1, st);
  }
  return 0;
}
