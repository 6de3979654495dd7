// IQL on SLAC latents (SPEC.md N3d; reference rlkit/torch/sac/iql_trainer.py:209-435), beside the grouped layers of mlp.hip: the
// fused critic and tanh-Gaussian policy loss heads, and the Polyak update of the target networks.  All fp32, no atomics, a fixed
// summation order: two identical calls give bitwise identical results.
#include "rl_head.h"

// ---- loss heads: one workgroup of 1024 threads, thread t owns the rows t, t + 1024, ...; the per-thread sums are added through LDS
//      by the halving tree of rl_head.h --------------------------------------------------------------------------------------------------
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
  head_tree_sum<3>(red, t);
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
      corr += 0.69314718055994531f - u - head_softplus(x);
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
  head_tree_sum<1>(red, t);
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
  if (!s2p_al16(target) || !s2p_al16(source)) S2P_FAIL(-1, "%s: buffers must be 16-byte aligned", who);
  const long long n4 = (n + 3) / 4;
  const long long want = (n4 + 255) / 256;
  hipLaunchKernelGGL(iql_soft_update_kernel, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, (hipStream_t)stream, target,
                     source, n4, (long long)n, (float)(1.0 - (double)tau), tau);
  S2P_CHECK_LAUNCH("iql_soft_update_kernel");
  return 0;
}
