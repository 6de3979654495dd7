// IQL on SLAC latents (SPEC.md N3d; reference rlkit/torch/sac/iql_trainer.py:209-435): grouped ReLU linear layers forward and
// backward, the fused critic and tanh-Gaussian policy loss heads, and the Polyak update of the target networks.
// Group = network: qf1, qf2, target_qf1, target_qf2, vf and the policy are MLPs of one hidden width but of unequal input width and
// row count, so a call carries a table of per-group views (at most MLP_MAX_G, copied into the kernel arguments) and one launch
// serves all of them, grid z = group.  Wide layers run on the wave tiles of ens_tile.h (the tiles of the ensemble entry points,
// here with ReLU or identity); the N = 1 and N = 2 A last layers run on plain dot-product kernels (a 32 x 64 MFMA tile would be
// 98 % / 81 % padding there, and with one wave per row the reads are whole contiguous rows).  All fp32, no atomics, a fixed
// summation order: two identical calls give bitwise identical results.
#include "ens_tile.h"

#define MLP_MAX_G 8
#define MLP_DOT_MAX_N 16
struct MlpFwdArgs { EnsFwdTile g[MLP_MAX_G]; };
struct MlpBwdArgs { EnsBwdTile g[MLP_MAX_G]; };

// ---- wide layers: the MFMA wave tiles -------------------------------------------------------------------------------------------------
template <int ACT> __global__ __launch_bounds__(256) void mlp_fwd_kernel(const MlpFwdArgs a) {
  const EnsFwdTile t = a.g[blockIdx.z];
  const int wave = threadIdx.x >> 6, nb = blockIdx.x * 64, mb = blockIdx.y * 128 + wave * 32;
  if (mb >= t.B) return;                                     // (wave-uniform; a group of fewer rows than the widest one ends here)
  ens_fwd_tile<ACT>(t, mb, nb);
}
// grid x: the weight tiles of a group (four waves = four tiles per workgroup), then its input tiles; sized for the largest group
template <int ACT> __global__ __launch_bounds__(256) void mlp_bwd_kernel(const MlpBwdArgs a) {
  const EnsBwdTile t = a.g[blockIdx.z];
  const int wave = threadIdx.x >> 6;
  if (t.B == 0) return;
  const int tk = (t.K + 63) / 64, w_tiles = ((t.N + 31) / 32) * tk, w_blocks = (w_tiles + 3) / 4;
  if ((int)blockIdx.x < w_blocks) {
    const int id = blockIdx.x * 4 + wave;
    if (id >= w_tiles) return;                               // (wave-uniform)
    ens_wgrad_tile(t, (id / tk) * 32, (id % tk) * 64);
    return;
  }
  if (!t.dprev) return;
  const int id = blockIdx.x - w_blocks, tm = (t.B + 127) / 128;
  if (id >= tm * tk) return;
  const int mb = (id / tk) * 128 + wave * 32;
  if (mb >= t.B) return;                                     // (wave-uniform)
  ens_dgrad_tile<ACT>(t, mb, (id % tk) * 64);
}

// ---- narrow last layers (N <= MLP_DOT_MAX_N): dot products ----------------------------------------------------------------------------
// forward: one wave per row; lane l takes k = 4 l .. 4 l + 3 of every 256, in k order, then the 64 lane sums meet in a butterfly
template <int ACT> __global__ __launch_bounds__(256) void mlp_dot_fwd_kernel(const MlpFwdArgs a) {
  const EnsFwdTile t = a.g[blockIdx.z];
  const int lane = threadIdx.x & 63, m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= t.B) return;                                      // (wave-uniform)
  const float* xr = t.x + (size_t)m * t.xp;
  for (int n = 0; n < t.N; ++n) {
    const float* wr = t.w + (size_t)n * t.K;
    float s = 0.f;
    for (int k = lane * 4; k < t.K; k += 256) {              // K is a multiple of 4: a float4 is in or out
      const f32x4 xv = *(const f32x4*)(xr + k), wv = *(const f32x4*)(wr + k);
#pragma unroll
      for (int c = 0; c < 4; ++c) s += xv[c] * wv[c];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) {
      const float v = s + t.bias[n];
      const size_t o = (size_t)m * t.yp + n;
      if (t.pre) t.pre[o] = v;
      if (t.act) t.act[o] = ens_act<ACT>(v);
    }
  }
}
// backward.  Weight blocks: 64 input columns x 4 row lanes; row lane r sums the rows r, r + 4, ... in row order, then the four
// partial sums are added in lane order through LDS (db from the same loop, by the first block).  Input blocks: one thread per
// (row, column) of dprev, n in order.
template <int ACT> __global__ __launch_bounds__(256) void mlp_dot_bwd_kernel(const MlpBwdArgs a) {
  __shared__ float red[4][MLP_DOT_MAX_N + 1][64];
  const EnsBwdTile t = a.g[blockIdx.z];
  if (t.B == 0) return;
  const int col = threadIdx.x & 63, rl = threadIdx.x >> 6, wb = (t.K + 63) / 64;
  if ((int)blockIdx.x < wb) {
    const int k = blockIdx.x * 64 + col;
    const bool kok = k < t.K, bias_lane = blockIdx.x == 0 && col < t.N;
    float acc[MLP_DOT_MAX_N] = {}, bs = 0.f;
    for (int m = rl; m < t.B; m += 4) {
      const float xv = kok ? t.x[(size_t)m * t.xp + k] : 0.f;
      const float* dr = t.dpre + (size_t)m * t.dp;
#pragma unroll
      for (int n = 0; n < MLP_DOT_MAX_N; ++n)
        if (n < t.N) acc[n] += dr[n] * xv;
      if (bias_lane) bs += dr[col];
    }
#pragma unroll
    for (int n = 0; n < MLP_DOT_MAX_N; ++n) red[rl][n][col] = acc[n];
    red[rl][MLP_DOT_MAX_N][col] = bs;
    __syncthreads();
    if (rl != 0) return;
#pragma unroll
    for (int n = 0; n < MLP_DOT_MAX_N; ++n)
      if (n < t.N && kok) t.dw[(size_t)n * t.K + k] = ((red[0][n][col] + red[1][n][col]) + red[2][n][col]) + red[3][n][col];
    if (bias_lane)
      t.db[col] = ((red[0][MLP_DOT_MAX_N][col] + red[1][MLP_DOT_MAX_N][col]) + red[2][MLP_DOT_MAX_N][col]) + red[3][MLP_DOT_MAX_N][col];
    return;
  }
  if (!t.dprev) return;
  ens_dot_dgrad_elem<ACT>(t, (long long)(blockIdx.x - wb) * 256 + threadIdx.x);
}

// ---- loss heads: one workgroup of 1024 threads, thread t owns the rows t, t + 1024, ...; the per-thread sums are added through LDS
//      by a halving tree (a fixed order), as ens_nll_kernel adds its own -----------------------------------------------------------------
template <int S> __device__ __forceinline__ void iql_tree_sum(float (&red)[S][1024], int t) {
  for (int w = 512; w > 0; w >>= 1) {
    __syncthreads();
    if (t < w)
#pragma unroll
      for (int s = 0; s < S; ++s) red[s][t] += red[s][t + w];
  }
  __syncthreads();
}
struct IqlCriticArgs {
  const float *q1, *q2, *tq1, *tq2, *v, *v_next, *reward, *terminal; int B; float reward_scale, discount, quantile, beta, clip;
  float *losses, *dq1, *dq2, *dv, *weights, *adv, *q_target;
};
__global__ __launch_bounds__(1024) void iql_critic_head_kernel(const IqlCriticArgs a) {
  __shared__ float red[3][1024];
  const int t = threadIdx.x;
  const float inv_b = 1.f / (float)a.B;
  float s1 = 0.f, s2 = 0.f, sv = 0.f;
  for (int b = t; b < a.B; b += 1024) {
    const float qt = a.reward_scale * a.reward[b] + (1.f - a.terminal[b]) * a.discount * a.v_next[b];
    const float e1 = a.q1[b] - qt, e2 = a.q2[b] - qt;
    const float qp = fminf(a.tq1[b], a.tq2[b]);
    const float ve = a.v[b] - qp, w = ve > 0.f ? 1.f - a.quantile : a.quantile;
    s1 += e1 * e1; s2 += e2 * e2; sv += w * (ve * ve);
    if (a.dq1) a.dq1[b] = 2.f * e1 * inv_b;
    if (a.dq2) a.dq2[b] = 2.f * e2 * inv_b;
    if (a.dv) a.dv[b] = 2.f * w * ve * inv_b;
    if (a.weights) a.weights[b] = fminf(expf(-ve / a.beta), a.clip);           // adv = q_pred - vf = -vf_err
    if (a.adv) a.adv[b] = -ve;
    if (a.q_target) a.q_target[b] = qt;
  }
  if (!a.losses) return;                                     // (launch-uniform)
  red[0][t] = s1; red[1][t] = s2; red[2][t] = sv;
  iql_tree_sum<3>(red, t);
  if (t < 3) a.losses[t] = red[t][0] * inv_b;
}

// log pi(a) of TanhNormal(mu, exp(clamp(raw_ls, -20, 2))) at a given action (rlkit/torch/distributions.py:339-354), fp32 in the
// reference's own operation order: the clamp of the action, u = log(1 + v) / 2 - log(1 - v) / 2 (NOT log1p: 1 - v is rounded first,
// as torch rounds it), softplus as max(x, 0) + log1p(exp(-|x|)) (SPEC.md N3b).
struct IqlPolicyArgs { const float* raw; int rp; const float* action; int ap; const float* weights; int B, A; float* loss; float* draw; int dwp; float* logp; };
__global__ __launch_bounds__(1024) void iql_policy_head_kernel(const IqlPolicyArgs a) {
  __shared__ float red[1][1024];
  const int t = threadIdx.x;
  const float inv_b = 1.f / (float)a.B;
  float sl = 0.f;
  for (int b = t; b < a.B; b += 1024) {
    const float* r = a.raw + (size_t)b * a.rp;
    const float* ac = a.action + (size_t)b * a.ap;
    const float wgt = a.weights[b], gs = -wgt * inv_b;       // d loss / d logp of this row
    float lp = 0.f, corr = 0.f;
    for (int d = 0; d < a.A; ++d) {
      const float v = fminf(fmaxf(ac[d], -0.999999f), 0.999999f);
      const float u = logf(1.f + v) / 2.f - logf(1.f - v) / 2.f;
      const float mu = r[d], lr = r[a.A + d], ls = fminf(fmaxf(lr, -20.f), 2.f);
      const float inv = expf(-ls), z = (u - mu) * inv;
      lp += -0.5f * z * z - ls - 0.91893853320467274f;       // 0.5 log 2 pi
      const float x = -2.f * u;
      corr += 0.69314718055994531f - u - (fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))));
      if (a.draw) {
        float* o = a.draw + (size_t)b * a.dwp;
        o[d] = gs * z * inv;
        o[a.A + d] = (lr >= -20.f && lr <= 2.f) ? gs * (z * z - 1.f) : 0.f;   // torch.clamp passes the gradient on [min, max]
      }
    }
    const float l = lp - 2.f * corr;
    if (a.logp) a.logp[b] = l;
    sl += -l * wgt;
  }
  if (!a.loss) return;                                       // (launch-uniform)
  red[0][t] = sl;
  iql_tree_sum<1>(red, t);
  if (t == 0) a.loss[0] = red[0][0] * inv_b;
}

// ---- Polyak update: target = (1 - tau) target + tau source, each product and the sum rounded on its own (what torch's
//      `target * (1.0 - tau) + param * tau` does: no fused multiply-add), 16-byte groups and a scalar tail ---------------------------------
// a product the compiler cannot fuse into the following add (it contracts a * b + c into one rounding otherwise, __fmul_rn or not)
__device__ __forceinline__ float iql_rounded(float v) { asm volatile("" : "+v"(v)); return v; }
__global__ void iql_soft_update_kernel(float* tgt, const float* src, long long n4, long long n, float omt, float tau) {
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < n4; idx += (long long)gridDim.x * blockDim.x) {
    const long long i = idx * 4;
    if (i + 4 <= n) {
      f32x4 tv = *(const f32x4*)(tgt + i);
      const f32x4 sv = *(const f32x4*)(src + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) tv[e] = iql_rounded(tv[e] * omt) + iql_rounded(sv[e] * tau);
      *(f32x4*)(tgt + i) = tv;
      continue;
    }
    for (long long k = i; k < n; ++k) tgt[k] = iql_rounded(tgt[k] * omt) + iql_rounded(src[k] * tau);
  }
}

// ---- entry points -------------------------------------------------------------------------------------------------------------------
static inline bool iql_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static int iql_act(const char* who, int act) {
  if (act == S2P_ACT_NONE || act == S2P_ACT_RELU) return 0;
  S2P_FAIL(-1, "%s: activation %d (none and relu only)", who, act);
}

extern "C" int s2p_mlp_linear_fwd(const s2p_mlp_fwd_group* groups, int G, int N, int act, void* stream) {
  const char* who = "s2p_mlp_linear_fwd";
  if (G < 0 || N < 0) S2P_FAIL(-1, "%s: negative size", who);
  if (G == 0 || N == 0) return 0;
  if (!groups) S2P_FAIL(-1, "%s: null group table", who);
  if (G > MLP_MAX_G) S2P_FAIL(-1, "%s: at most %d groups (G %d)", who, MLP_MAX_G, G);
  if (int rc = iql_act(who, act)) return rc;
  MlpFwdArgs a{};
  int rows = 0;
  for (int g = 0; g < G; ++g) {
    const s2p_mlp_fwd_group& s = groups[g];
    if (s.rows < 0 || s.K < 0) S2P_FAIL(-1, "%s: group %d: negative size", who, g);
    if (s.rows == 0) continue;                               // (an empty group: B = 0 in the table, no pointer looked at)
    if (!s.x || !s.w || !s.bias || (!s.pre && !s.act)) S2P_FAIL(-1, "%s: group %d: null tensor (x, w, bias and one of pre / act are required)", who, g);
    if (s.K == 0 || s.K % 4 || s.x_pitch % 4 || !iql_al16(s.x) || !iql_al16(s.w))
      S2P_FAIL(-1, "%s: group %d: K, x_pitch must be multiples of 4 floats (K > 0), x and w 16-byte aligned", who, g);
    if (s.x_pitch < s.K || s.y_pitch < N) S2P_FAIL(-1, "%s: group %d: pitch shorter than the row", who, g);
    a.g[g] = EnsFwdTile{s.x, s.w, s.bias, s.pre, s.act, s.x_pitch, s.y_pitch, s.rows, s.K, N};
    rows = s.rows > rows ? s.rows : rows;
  }
  if (rows == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  if (N <= MLP_DOT_MAX_N) {
    const dim3 grid(cdiv(rows, 4), 1, G);
    if (act == S2P_ACT_RELU) hipLaunchKernelGGL(mlp_dot_fwd_kernel<ENS_ACT_RELU>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(mlp_dot_fwd_kernel<ENS_ACT_NONE>, grid, dim3(256), 0, st, a);
    S2P_CHECK_LAUNCH("mlp_dot_fwd_kernel");
    return 0;
  }
  const dim3 grid(cdiv(N, 64), cdiv(rows, 128), G);
  if (act == S2P_ACT_RELU) hipLaunchKernelGGL(mlp_fwd_kernel<ENS_ACT_RELU>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(mlp_fwd_kernel<ENS_ACT_NONE>, grid, dim3(256), 0, st, a);
  S2P_CHECK_LAUNCH("mlp_fwd_kernel");
  return 0;
}

extern "C" int s2p_mlp_linear_bwd(const s2p_mlp_bwd_group* groups, int G, int N, int act_prev, void* stream) {
  const char* who = "s2p_mlp_linear_bwd";
  if (G < 0 || N < 0) S2P_FAIL(-1, "%s: negative size", who);
  if (G == 0 || N == 0) return 0;
  if (!groups) S2P_FAIL(-1, "%s: null group table", who);
  if (G > MLP_MAX_G) S2P_FAIL(-1, "%s: at most %d groups (G %d)", who, MLP_MAX_G, G);
  if (int rc = iql_act(who, act_prev)) return rc;
  const bool dot = N <= MLP_DOT_MAX_N;
  if (!dot && N % 4) S2P_FAIL(-1, "%s: N above %d must be a multiple of 4 (N %d)", who, MLP_DOT_MAX_N, N);
  MlpBwdArgs a{};
  int blocks = 0;
  for (int g = 0; g < G; ++g) {
    const s2p_mlp_bwd_group& s = groups[g];
    if (s.rows < 0 || s.K < 0) S2P_FAIL(-1, "%s: group %d: negative size", who, g);
    if (s.rows == 0 || s.K == 0) continue;
    if (!s.x || !s.dpre || !s.dw || !s.db) S2P_FAIL(-1, "%s: group %d: null tensor (x, dpre, dw, db are required)", who, g);
    if (s.dprev && (!s.w || (act_prev != S2P_ACT_NONE && !s.pre_prev))) S2P_FAIL(-1, "%s: group %d: dprev needs w (and pre_prev with relu)", who, g);
    if (!dot && (s.dpre_pitch % 4 || !iql_al16(s.dpre)))
      S2P_FAIL(-1, "%s: group %d: dpre_pitch must be a multiple of 4 floats, dpre 16-byte aligned", who, g);
    if (s.x_pitch < s.K || s.dpre_pitch < N || (s.dprev && s.prev_pitch < s.K)) S2P_FAIL(-1, "%s: group %d: pitch shorter than the row", who, g);
    if ((int64_t)s.rows * s.K >= ((int64_t)1 << 31)) S2P_FAIL(-1, "%s: group %d: rows * K must stay below 2^31", who, g);
    a.g[g] = EnsBwdTile{s.x, s.dpre, s.w, s.dw, s.db, s.pre_prev, s.dprev, s.x_pitch, s.dpre_pitch, s.prev_pitch, s.rows, s.K, N};
    const int tk = cdiv(s.K, 64);
    const int b = dot ? tk + (s.dprev ? cdiv((int64_t)s.rows * s.K, 256) : 0)
                      : cdiv((int64_t)cdiv(N, 32) * tk, 4) + (s.dprev ? cdiv(s.rows, 128) * tk : 0);
    blocks = b > blocks ? b : blocks;
  }
  if (blocks == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid(blocks, 1, G);
  if (dot) {
    if (act_prev == S2P_ACT_RELU) hipLaunchKernelGGL(mlp_dot_bwd_kernel<ENS_ACT_RELU>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(mlp_dot_bwd_kernel<ENS_ACT_NONE>, grid, dim3(256), 0, st, a);
    S2P_CHECK_LAUNCH("mlp_dot_bwd_kernel");
    return 0;
  }
  if (act_prev == S2P_ACT_RELU) hipLaunchKernelGGL(mlp_bwd_kernel<ENS_ACT_RELU>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(mlp_bwd_kernel<ENS_ACT_NONE>, grid, dim3(256), 0, st, a);
  S2P_CHECK_LAUNCH("mlp_bwd_kernel");
  return 0;
}

extern "C" int s2p_iql_critic_head(const float* q1, const float* q2, const float* tq1, const float* tq2, const float* v,
                                   const float* v_next, const float* reward, const float* terminal, int B, float reward_scale,
                                   float discount, float quantile, float beta, float clip_score, float* losses, float* dq1,
                                   float* dq2, float* dv, float* weights, float* adv, float* q_target, void* stream) {
  const char* who = "s2p_iql_critic_head";
  if (B < 0) S2P_FAIL(-1, "%s: negative size", who);
  if (B == 0) return 0;
  if (!q1 || !q2 || !tq1 || !tq2 || !v || !v_next || !reward || !terminal) S2P_FAIL(-1, "%s: null tensor (the eight inputs are required)", who);
  if (!losses && !dq1 && !dq2 && !dv && !weights && !adv && !q_target) S2P_FAIL(-1, "%s: no output", who);
  if (!(beta > 0.f)) S2P_FAIL(-1, "%s: beta must be positive", who);
  IqlCriticArgs a{q1, q2, tq1, tq2, v, v_next, reward, terminal, B, reward_scale, discount, quantile, beta, clip_score,
                  losses, dq1, dq2, dv, weights, adv, q_target};
  hipLaunchKernelGGL(iql_critic_head_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
  S2P_CHECK_LAUNCH("iql_critic_head_kernel");
  return 0;
}

extern "C" int s2p_tanh_gauss_policy_head(const float* raw, int raw_pitch, const float* action, int action_pitch,
                                          const float* weights, int B, int A, float* loss, float* draw, int draw_pitch,
                                          float* logp, void* stream) {
  const char* who = "s2p_tanh_gauss_policy_head";
  if (B < 0 || A < 0) S2P_FAIL(-1, "%s: negative size", who);
  if (B == 0 || A == 0) return 0;
  if (!raw || !action || !weights) S2P_FAIL(-1, "%s: null tensor (raw, action, weights are required)", who);
  if (!loss && !draw && !logp) S2P_FAIL(-1, "%s: no output", who);
  if ((int64_t)raw_pitch < 2 * (int64_t)A || action_pitch < A || (draw && (int64_t)draw_pitch < 2 * (int64_t)A))
    S2P_FAIL(-1, "%s: pitch shorter than the row", who);
  IqlPolicyArgs a{raw, raw_pitch, action, action_pitch, weights, B, A, loss, draw, draw_pitch, logp};
  hipLaunchKernelGGL(iql_policy_head_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
  S2P_CHECK_LAUNCH("iql_policy_head_kernel");
  return 0;
}

extern "C" int s2p_soft_update(float* target, const float* source, int64_t n, float tau, void* stream) {
  const char* who = "s2p_soft_update";
  if (n < 0) S2P_FAIL(-1, "%s: negative size", who);
  if (n == 0) return 0;
  if (!target || !source) S2P_FAIL(-1, "%s: null pointer", who);
  if (!iql_al16(target) || !iql_al16(source)) S2P_FAIL(-1, "%s: buffers must be 16-byte aligned", who);
  const long long n4 = (n + 3) / 4;
  const long long want = (n4 + 255) / 256;
  hipLaunchKernelGGL(iql_soft_update_kernel, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, (hipStream_t)stream, target,
                     source, n4, (long long)n, (float)(1.0 - (double)tau), tau);
  S2P_CHECK_LAUNCH("iql_soft_update_kernel");
  return 0;
}
