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
#include "ens_tile.h"

#define ENS_MAX_G 8
struct EnsSel { int m[ENS_MAX_G]; };

// ---- forward: pre[m][g N + n] = sum_k x[g][m][k] W[e][n][k] + b[e][n];  act = swish(pre) ---------------------------------------
// The wave tile is ens_fwd_tile (ens_tile.h): 32 rows x 64 columns per wave, a workgroup four such row tiles; grid z = group.
struct EnsFwdArgs {
  const float* x; long long xg; int xp; const float* w; const float* bias; float* pre; float* act; int yp, B, K, N; EnsSel sel;
};
__global__ __launch_bounds__(256) void ens_fwd_kernel(const EnsFwdArgs a) {
  const int wave = threadIdx.x >> 6, g = blockIdx.z, e = a.sel.m[g];
  const int nb = blockIdx.x * 64, mb = blockIdx.y * 128 + wave * 32;
  if (mb >= a.B) return;                                     // (wave-uniform)
  const size_t yo = (size_t)g * a.N;
  const EnsFwdTile t{a.x + (size_t)g * a.xg, a.w + (size_t)e * a.N * a.K, a.bias + (size_t)e * a.N, a.pre ? a.pre + yo : nullptr,
                     a.act ? a.act + yo : nullptr, a.xp, a.yp, a.B, a.K, a.N};
  ens_fwd_tile<ENS_ACT_SWISH>(t, mb, nb);
}

// ---- backward: one launch, the two kinds of wave tiles of ens_tile.h (weight tiles first, then the input tiles) -------------------
struct EnsBwdArgs {
  const float* x; long long xg; int xp; const float* dpre; int dp; const float* w; float* dw; float* db;
  const float* pre_prev; float* dprev; int pp, B, K, N, G, w_tiles, w_blocks; EnsSel sel;
};
__device__ __forceinline__ EnsBwdTile ens_bwd_view(const EnsBwdArgs& a, int g) {
  const int e = a.sel.m[g];
  const size_t wo = (size_t)e * a.N * a.K, po = (size_t)g * a.K;
  return EnsBwdTile{a.x + (size_t)g * a.xg, a.dpre + (size_t)g * a.N, a.w ? a.w + wo : nullptr, a.dw + wo, a.db + (size_t)e * a.N,
                    a.pre_prev ? a.pre_prev + po : nullptr, a.dprev ? a.dprev + po : nullptr, a.xp, a.dp, a.pp, a.B, a.K, a.N};
}
__global__ __launch_bounds__(256) void ens_bwd_kernel(const EnsBwdArgs a) {
  const int wave = threadIdx.x >> 6;
  const int tk = (a.K + 63) / 64;
  if ((int)blockIdx.x < a.w_blocks) {
    const int tn = (a.N + 31) / 32;
    int id = blockIdx.x * 4 + wave;
    if (id >= a.w_tiles) return;                             // (wave-uniform)
    const int g = id / (tn * tk); id -= g * tn * tk;
    ens_wgrad_tile(ens_bwd_view(a, g), (id / tk) * 32, (id % tk) * 64);
    return;
  }
  const int tm = (a.B + 127) / 128;
  int id = blockIdx.x - a.w_blocks;
  const int g = id / (tm * tk); id -= g * tm * tk;
  const int mb = (id / tk) * 128 + wave * 32, kb = (id % tk) * 64;
  if (mb >= a.B) return;                                     // (wave-uniform)
  ens_dgrad_tile<ENS_ACT_SWISH>(ens_bwd_view(a, g), mb, kb);
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
  if (K == 0 || K % 4 || x_pitch % 4 || x_gstride % 4 || !s2p_al16(x) || !s2p_al16(w))
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
  if (K % 4 || N % 4 || dpre_pitch % 4 || !s2p_al16(dpre))
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
  if (!sums && !loss && !draw && !dmin_logstd && !dmax_logstd && !mean && !std) S2P_FAIL(-1, "%s: no output", who);
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
