// Training of the ensemble state-dynamics model (SPEC.md N2b; reference gaussian_ensemble.py:21-96): grouped linear forward that
// keeps the pre-activations, grouped linear backward (weight + bias gradient and the input gradient with the producer's Swish
// derivative fused) and the fused Gaussian NLL head.  Group = ensemble member: every entry point is ONE launch for all members.
// All fp32 on the exact-fp32 matrix instruction v_mfma_f32_32x32x2_f32 (lane l holds A[row l & 31][k = l >> 5] and
// B[k = l >> 5][col l & 31]; result register r of lane l is D[row (r & 3) + 8 (r >> 2) + 4 (l >> 5)][col l & 31]), operands straight
// from global memory into the MFMA registers (no LDS in the GEMM kernels), no atomics, a fixed summation order: two identical
// calls give bitwise identical results.
//
// Layouts.  Activations of a layer: [B][G * N], group g at columns g * N (the layout the grouped conv path and s2p_ensemble_head
// use).  Weights and their gradients: PACKED [E][N][K], K = the (padded) input width, contiguous -- the transpose of the
// reference's [E, in, out].  `member[g]` maps group g to its slot e in the [E] arrays (set_select); activations are compact in g.
#include "s2p_common.h"

#define ENS_MAX_G 8
struct EnsSel { int m[ENS_MAX_G]; };

__device__ __forceinline__ float ens_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }
// d/dp [p sigmoid(p)]: needs the PRE-activation (not a function of swish's output)
__device__ __forceinline__ float ens_swish_grad(float p) { const float s = ens_sigmoid(p); return s * (1.f + p * (1.f - s)); }
__device__ __forceinline__ int ens_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// ---- forward: pre[m][g N + n] = sum_k x[g][m][k] W[e][n][k] + b[e][n];  act = swish(pre) ---------------------------------------
// A wave owns 32 rows x 64 columns (two accumulators share the x operand), a workgroup four such row tiles.  A k-chunk of 8 is one
// float4 per lane and operand (lane half h takes k = 8 t + 4 h .. + 3) consumed by four MFMAs (MFMA c uses component c of both
// operands: the same k permutation on both sides, so the sum is the plain dot product).
struct EnsFwdArgs {
  const float* x; long long xg; int xp; const float* w; const float* bias; float* pre; float* act; int yp, B, K, N; EnsSel sel;
};
__global__ __launch_bounds__(256) void ens_fwd_kernel(const EnsFwdArgs a) {
  constexpr int U = 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, h = lane >> 5;
  const int g = blockIdx.z, e = a.sel.m[g];
  const int nb = blockIdx.x * 64, mb = blockIdx.y * 128 + wave * 32;
  if (mb >= a.B) return;                                     // (wave-uniform)
  const bool two = nb + 32 < a.N;                            // (wave-uniform)
  const int m = mb + i, n0 = nb + i, n1 = nb + 32 + i;
  const bool mok = m < a.B, n0ok = n0 < a.N, n1ok = two && n1 < a.N;
  const float* xr = a.x + (size_t)g * a.xg + (size_t)(mok ? m : 0) * a.xp;
  const float* w0 = a.w + ((size_t)e * a.N + (n0ok ? n0 : 0)) * a.K;
  const float* w1 = a.w + ((size_t)e * a.N + (n1ok ? n1 : 0)) * a.K;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x16 acc0 = {}, acc1 = {};
  for (int kc = 0; kc < a.K; kc += 8 * U) {
    f32x4 xv[U], wv0[U], wv1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = kc + 8 * u + 4 * h;                      // K and the pitches are multiples of 4: a float4 is in or out
      const bool in = k < a.K;
      xv[u] = (mok && in) ? *(const f32x4*)(xr + k) : z4;
      wv0[u] = (n0ok && in) ? *(const f32x4*)(w0 + k) : z4;
      wv1[u] = (n1ok && in) ? *(const f32x4*)(w1 + k) : z4;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[u][c], wv0[u][c], acc0, 0, 0, 0);
        if (two) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[u][c], wv1[u][c], acc1, 0, 0, 0);
      }
  }
  auto store = [&](const f32x16& acc, int n, bool nok) {
    if (!nok) return;
    const float b = a.bias[(size_t)e * a.N + n];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int mo = mb + ens_row(r, h);
      if (mo >= a.B) continue;
      const float v = acc[r] + b;
      const size_t o = (size_t)mo * a.yp + (size_t)g * a.N + n;
      if (a.pre) a.pre[o] = v;
      if (a.act) a.act[o] = v / (1.f + expf(-v));
    }
  };
  store(acc0, n0, n0ok);
  store(acc1, n1, n1ok);
}

// ---- backward: one launch, two kinds of wave tiles ------------------------------------------------------------------------------
//   weight tiles: dW[e][n][k] = sum_m dpre[m][g N + n] x[g][m][k]   (32 n x 64 k per wave, the whole batch in row order: no row
//                 split, so no partial sums and no second pass at any B);  db[e][n] = sum_m dpre  from the same operand values
//                 (per lane in row order, then the two lane halves);
//   input tiles : dprev[m][g K + k] = (sum_n dpre[m][g N + n] W[e][n][k]) * swish'(pre_prev[m][g K + k])   (32 m x 64 k per wave).
struct EnsBwdArgs {
  const float* x; long long xg; int xp; const float* dpre; int dp; const float* w; float* dw; float* db;
  const float* pre_prev; float* dprev; int pp, B, K, N, G, w_tiles, w_blocks; EnsSel sel;
};
__global__ __launch_bounds__(256) void ens_bwd_kernel(const EnsBwdArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, h = lane >> 5;
  const int tk = (a.K + 63) / 64;
  if ((int)blockIdx.x < a.w_blocks) {
    constexpr int U = 8;
    const int tn = (a.N + 31) / 32;
    int id = blockIdx.x * 4 + wave;
    if (id >= a.w_tiles) return;                             // (wave-uniform)
    const int g = id / (tn * tk); id -= g * tn * tk;
    const int nb = (id / tk) * 32, kb = (id % tk) * 64, e = a.sel.m[g];
    const bool two = kb + 32 < a.K;                          // (wave-uniform)
    const int n = nb + i, k0 = kb + i, k1 = kb + 32 + i;
    const bool nok = n < a.N, k0ok = k0 < a.K, k1ok = two && k1 < a.K;
    const float* dcol = a.dpre + (size_t)g * a.N + (nok ? n : 0);
    const float* xcol = a.x + (size_t)g * a.xg;
    f32x16 acc0 = {}, acc1 = {};
    float bsum = 0.f;
    for (int m0 = 0; m0 < a.B; m0 += 2 * U) {
      float dv[U], x0[U], x1[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int m = m0 + 2 * u + h;
        const bool mok = m < a.B;
        dv[u] = (mok && nok) ? dcol[(size_t)m * a.dp] : 0.f;
        x0[u] = (mok && k0ok) ? xcol[(size_t)m * a.xp + k0] : 0.f;
        x1[u] = (mok && k1ok) ? xcol[(size_t)m * a.xp + k1] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[u], x0[u], acc0, 0, 0, 0);
        if (two) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[u], x1[u], acc1, 0, 0, 0);
        bsum += dv[u];
      }
    }
    if (kb == 0) {
      const float s = bsum + __shfl_xor(bsum, 32, 64);       // (half 0 + half 1 in both halves: one fixed order)
      if (h == 0 && nok) a.db[(size_t)e * a.N + n] = s;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int no = nb + ens_row(r, h);
      if (no >= a.N) continue;
      float* row = a.dw + ((size_t)e * a.N + no) * a.K;
      if (k0ok) row[k0] = acc0[r];
      if (k1ok) row[k1] = acc1[r];
    }
    return;
  }
  constexpr int U = 2;
  const int tm = (a.B + 127) / 128;
  int id = blockIdx.x - a.w_blocks;
  const int g = id / (tm * tk); id -= g * tm * tk;
  const int mb = (id / tk) * 128 + wave * 32, kb = (id % tk) * 64, e = a.sel.m[g];
  if (mb >= a.B) return;                                     // (wave-uniform)
  const bool two = kb + 32 < a.K;
  const int m = mb + i, k0 = kb + i, k1 = kb + 32 + i;
  const bool mok = m < a.B, k0ok = k0 < a.K, k1ok = two && k1 < a.K;
  const float* dr = a.dpre + (size_t)(mok ? m : 0) * a.dp + (size_t)g * a.N;
  const float* wc0 = a.w + (size_t)e * a.N * a.K + (k0ok ? k0 : 0);
  const float* wc1 = a.w + (size_t)e * a.N * a.K + (k1ok ? k1 : 0);
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x16 acc0 = {}, acc1 = {};
  for (int nc = 0; nc < a.N; nc += 8 * U) {
    f32x4 dv[U], w0[U], w1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int n = nc + 8 * u + 4 * h;                      // N and dp are multiples of 4: a float4 of dpre is in or out
      const bool in = n < a.N;
      dv[u] = (mok && in) ? *(const f32x4*)(dr + n) : z4;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        w0[u][c] = (in && k0ok) ? wc0[(size_t)(n + c) * a.K] : 0.f;
        w1[u][c] = (in && k1ok) ? wc1[(size_t)(n + c) * a.K] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[u][c], w0[u][c], acc0, 0, 0, 0);
        if (two) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[u][c], w1[u][c], acc1, 0, 0, 0);
      }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int mo = mb + ens_row(r, h);
    if (mo >= a.B) continue;
    const size_t o = (size_t)mo * a.pp + (size_t)g * a.K;
    if (k0ok) a.dprev[o + k0] = acc0[r] * ens_swish_grad(a.pre_prev[o + k0]);
    if (k1ok) a.dprev[o + k1] = acc1[r] * ens_swish_grad(a.pre_prev[o + k1]);
  }
}

// ---- fused NLL head ---------------------------------------------------------------------------------------------------------------
// One workgroup of 1024 threads.  A thread owns ONE (group, output) pair and every R-th row of it (R = 1024 / (G D) row lanes), so its
// four running sums (nll, squared error, d/dmin, d/dmax) belong to one member and one output; they are then added through LDS in a
// fixed order: per member over (row lane, output), per output over (group, row lane).
__device__ __forceinline__ float ens_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }   // F.softplus (threshold 20)
struct EnsNllArgs {
  const float* raw; int rp; const float* xin; long long xg; int xp; const float* tgt; long long tg; int tp; int B, G, D;
  const float* mn; const float* mx; float scale, reg; float* sums; float* loss; float* draw; int dwp; float* dmin; float* dmax;
  float* mean; float* std;
};
__global__ __launch_bounds__(1024) void ens_nll_kernel(const EnsNllArgs a) {
  __shared__ float red[4][1024];
  const int t = threadIdx.x, P = a.G * a.D, R = 1024 / P;
  float s_nll = 0.f, s_se = 0.f, s_mn = 0.f, s_mx = 0.f;
  if (t < P * R) {
    const int pair = t % P, r0 = t / P, g = pair / a.D, d = pair - g * a.D;
    const float mn = a.mn[d], mx = a.mx[d];
    for (int b = r0; b < a.B; b += R) {
      const float* r = a.raw + (size_t)b * a.rp + (size_t)g * 2 * a.D;
      const float mu = r[d] + (d < a.D - 1 ? a.xin[(size_t)g * a.xg + (size_t)b * a.xp + d] : 0.f);   // 'local' mode: the obs part is a delta
      const float up = mx - r[a.D + d], u = mx - ens_softplus(up);                                       // soft_clamp upper, then lower
      const float lo = u - mn, ls = mn + ens_softplus(lo);
      if (a.mean) a.mean[((size_t)g * a.B + b) * a.D + d] = mu;
      if (a.std) a.std[((size_t)g * a.B + b) * a.D + d] = expf(ls);
      if (!a.tgt) continue;
      const float inv = expf(-ls), diff = mu - a.tgt[(size_t)g * a.tg + (size_t)b * a.tp + d], z = diff * inv;
      s_nll += 0.5f * z * z + ls + 0.91893853320467274f;     // 0.5 log 2 pi
      s_se += diff * diff;
      const float gl = a.scale * (1.f - z * z);              // d loss / d logstd (after the clamp)
      const float sg_lo = ens_sigmoid(lo), sg_up = ens_sigmoid(up);
      s_mn += gl * ens_sigmoid(-lo);                         // d ls / d min = 1 - sigmoid(lo)
      s_mx += gl * sg_lo * ens_sigmoid(-up);                 // d ls / d max = sigmoid(lo) (1 - sigmoid(up))
      if (a.draw) {
        float* o = a.draw + (size_t)b * a.dwp + (size_t)g * 2 * a.D;
        o[d] = a.scale * z * inv;
        o[a.D + d] = gl * sg_lo * sg_up;
      }
    }
  }
  if (!a.tgt) return;                                        // (launch-uniform)
  red[0][t] = s_nll; red[1][t] = s_se; red[2][t] = s_mn; red[3][t] = s_mx;
  __syncthreads();
  __shared__ float tot[ENS_MAX_G];
  if (t < a.G) {                                             // member t: row lanes outer, outputs inner
    float n = 0.f, s = 0.f;
    for (int r = 0; r < R; ++r)
      for (int d = 0; d < a.D; ++d) { n += red[0][r * P + t * a.D + d]; s += red[1][r * P + t * a.D + d]; }
    if (a.sums) { a.sums[t] = n; a.sums[a.G + t] = s; }
    tot[t] = n;
  }
  if (a.dmin && t >= 64 && t < 64 + a.D) {                   // output d: groups outer, row lanes inner
    const int d = t - 64;
    float n = 0.f, x = 0.f;
    for (int g = 0; g < a.G; ++g)
      for (int r = 0; r < R; ++r) { n += red[2][r * P + g * a.D + d]; x += red[3][r * P + g * a.D + d]; }
    a.dmin[d] = n - a.reg; a.dmax[d] = x + a.reg;
  }
  __syncthreads();
  if (a.loss && t == 0) {                                    // scale * sum_g nll_g + reg * sum_d (max_d - min_d), in index order
    float l = 0.f, b = 0.f;
    for (int g = 0; g < a.G; ++g) l += tot[g];
    for (int d = 0; d < a.D; ++d) b += a.mx[d] - a.mn[d];
    a.loss[0] = l * a.scale + a.reg * b;
  }
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------
static inline bool ens_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static int ens_sel(const char* who, const int32_t* member, int G, int E, EnsSel* s) {
  if (E < 1 || E > ENS_MAX_G || G > E) S2P_FAIL(-1, "%s: 1 <= G <= E <= %d needed (G %d, E %d)", who, ENS_MAX_G, G, E);
  for (int g = 0; g < ENS_MAX_G; ++g) s->m[g] = 0;
  for (int g = 0; g < G; ++g) {
    s->m[g] = member ? member[g] : g;
    if (s->m[g] < 0 || s->m[g] >= E) S2P_FAIL(-1, "%s: member[%d] = %d is outside [0, %d)", who, g, s->m[g], E);
  }
  return 0;
}

extern "C" int s2p_ensemble_linear_fwd(const float* x, int64_t x_gstride, int x_pitch, const float* w, const float* bias,
                                       const int32_t* member, int G, int E, int B, int K, int N, float* pre, float* act,
                                       int y_pitch, void* stream) {
  const char* who = "s2p_ensemble_linear_fwd";
  if (G < 0 || B < 0 || K < 0 || N < 0 || x_gstride < 0) S2P_FAIL(-1, "%s: negative size", who);
  if (G == 0 || B == 0 || N == 0) return 0;
  EnsSel sel; if (int rc = ens_sel(who, member, G, E, &sel)) return rc;
  if (!x || !w || !bias || (!pre && !act)) S2P_FAIL(-1, "%s: null tensor (x, w, bias and one of pre / act are required)", who);
  if (K == 0 || K % 4 || x_pitch % 4 || x_gstride % 4 || !ens_al16(x) || !ens_al16(w))
    S2P_FAIL(-1, "%s: K, x_pitch, x_gstride must be multiples of 4 floats (K > 0), x and w 16-byte aligned", who);
  if (x_pitch < K || (int64_t)y_pitch < (int64_t)G * N) S2P_FAIL(-1, "%s: pitch shorter than the row", who);
  EnsFwdArgs a{x, (long long)x_gstride, x_pitch, w, bias, pre, act, y_pitch, B, K, N, sel};
  hipLaunchKernelGGL(ens_fwd_kernel, dim3(cdiv(N, 64), cdiv(B, 128), G), dim3(256), 0, (hipStream_t)stream, a);
  S2P_CHECK_LAUNCH("ens_fwd_kernel");
  return 0;
}

extern "C" int s2p_ensemble_linear_bwd(const float* x, int64_t x_gstride, int x_pitch, const float* dpre, int dpre_pitch,
                                       const float* w, const int32_t* member, int G, int E, int B, int K, int N, float* dw,
                                       float* db, const float* pre_prev, float* dprev, int prev_pitch, void* stream) {
  const char* who = "s2p_ensemble_linear_bwd";
  if (G < 0 || B < 0 || K < 0 || N < 0 || x_gstride < 0) S2P_FAIL(-1, "%s: negative size", who);
  if (G == 0 || B == 0 || N == 0 || K == 0) return 0;
  EnsSel sel; if (int rc = ens_sel(who, member, G, E, &sel)) return rc;
  if (!x || !dpre || !dw || !db) S2P_FAIL(-1, "%s: null tensor (x, dpre, dw, db are required)", who);
  if (dprev && (!w || !pre_prev)) S2P_FAIL(-1, "%s: dprev needs w and pre_prev", who);
  if (K % 4 || N % 4 || dpre_pitch % 4 || !ens_al16(dpre))
    S2P_FAIL(-1, "%s: K, N, dpre_pitch must be multiples of 4 floats, dpre 16-byte aligned", who);
  if (x_pitch < K || (int64_t)dpre_pitch < (int64_t)G * N || (dprev && (int64_t)prev_pitch < (int64_t)G * K))
    S2P_FAIL(-1, "%s: pitch shorter than the row", who);
  const int tk = cdiv(K, 64), w_tiles = G * cdiv(N, 32) * tk, w_blocks = cdiv(w_tiles, 4);
  const int d_blocks = dprev ? G * cdiv(B, 128) * tk : 0;
  EnsBwdArgs a{x, (long long)x_gstride, x_pitch, dpre, dpre_pitch, w, dw, db, pre_prev, dprev, prev_pitch, B, K, N, G, w_tiles,
               w_blocks, sel};
  hipLaunchKernelGGL(ens_bwd_kernel, dim3(w_blocks + d_blocks), dim3(256), 0, (hipStream_t)stream, a);
  S2P_CHECK_LAUNCH("ens_bwd_kernel");
  return 0;
}

extern "C" int s2p_ensemble_nll(const float* raw, int raw_pitch, const float* xin, int64_t x_gstride, int x_pitch,
                                const float* target, int64_t t_gstride, int t_pitch, int B, int G, int D,
                                const float* min_logstd, const float* max_logstd, float scale, float bound_reg, float* sums,
                                float* loss, float* draw, int draw_pitch, float* dmin_logstd, float* dmax_logstd, float* mean,
                                float* std, void* stream) {
  const char* who = "s2p_ensemble_nll";
  if (G < 0 || B < 0 || D < 0 || x_gstride < 0 || t_gstride < 0) S2P_FAIL(-1, "%s: negative size", who);
  if (G == 0 || B == 0 || D == 0) return 0;
  if (G > ENS_MAX_G || D < 2 || D > 33) S2P_FAIL(-1, "%s: G <= %d and 2 <= D <= 33 needed (G %d, D %d)", who, ENS_MAX_G, G, D);
  if (!raw || !xin || !min_logstd || !max_logstd) S2P_FAIL(-1, "%s: null tensor (raw, xin and the two bounds are required)", who);
  if (!target && (sums || loss || draw || dmin_logstd || dmax_logstd)) S2P_FAIL(-1, "%s: the loss outputs need a target", who);
  if (!target && !mean && !std) S2P_FAIL(-1, "%s: no output", who);
  if (!dmin_logstd != !dmax_logstd) S2P_FAIL(-1, "%s: dmin_logstd and dmax_logstd come together", who);
  if ((int64_t)raw_pitch < (int64_t)G * 2 * D || x_pitch < D - 1 || (target && t_pitch < D) ||
      (draw && (int64_t)draw_pitch < (int64_t)G * 2 * D))
    S2P_FAIL(-1, "%s: pitch shorter than the row", who);
  EnsNllArgs a{raw, raw_pitch, xin, (long long)x_gstride, x_pitch, target, (long long)t_gstride, t_pitch, B, G, D, min_logstd,
               max_logstd, scale, bound_reg, sums, loss, draw, draw_pitch, dmin_logstd, dmax_logstd, mean, std};
  hipLaunchKernelGGL(ens_nll_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
  S2P_CHECK_LAUNCH("ens_nll_kernel");
  return 0;
}
