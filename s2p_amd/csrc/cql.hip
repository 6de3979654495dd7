// CQL on SLAC latents (SPEC.md N3e; reference rlkit/torch/sac/cql_trainer.py:234-418, 576-585): what the CQL step needs beyond the
// grouped layers of mlp.hip and the heads of iql.hip.  The reparameterised TanhNormal sample with its log-probability from the
// pre-tanh value, and its backward; the fused SAC policy head with the entropy-temperature step; the fused CQL critic head (backup,
// MSE, importance-weighted log-sum-exp, their gradients).  All fp32, no atomics, a fixed summation order: two identical calls give
// bitwise identical results.
#include "rl_head.h"

// ---- reparameterised TanhNormal sample (rlkit/torch/distributions.py:339-386, gaussian_policy.py:113-146): one thread per
//      output row m * rep + r, the A components in order ------------------------------------------------------------------------------
struct CqlSampleArgs {
  const float* raw; int rp; const float* eps; int ep; int M, A, rep;
  float* action; int ap, agroup; float* logp; int lgroup; float* u; int up;
};
__global__ __launch_bounds__(256) void cql_rsample_kernel(const CqlSampleArgs a) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= (long long)a.M * a.rep) return;
  const int m = (int)(row / a.rep), r = (int)(row - (long long)m * a.rep);
  const float* rw = a.raw + (size_t)m * a.rp;
  const float* e = a.eps + (size_t)row * a.ep;
  float* ac = a.action ? a.action + ((size_t)m * a.agroup + r) * a.ap : nullptr;
  float* uo = a.u ? a.u + (size_t)row * a.up : nullptr;
  float lp = 0.f, corr = 0.f;
  for (int d = 0; d < a.A; ++d) {
    const float ls = fminf(fmaxf(rw[a.A + d], -20.f), 2.f), ev = e[d];
    const float u = rw[d] + expf(ls) * ev;
    lp += -0.5f * ev * ev - ls - 0.91893853320467274f;       // 0.5 log 2 pi;  (u - mu) / sigma IS eps
    const float x = -2.f * u;
    corr += 0.69314718055994531f - u - head_softplus(x);
    if (ac) ac[d] = tanhf(u);
    if (uo) uo[d] = u;
  }
  if (a.logp) a.logp[(size_t)m * a.lgroup + r] = lp - 2.f * corr;
}
// its backward at rep = 1: one thread per row
struct CqlSampleBwdArgs {
  const float* raw; int rp; const float* eps; int ep; const float* dlogp; const float* da; const float* da2; int dap;
  int M, A; float* draw; int dwp; int add;
};
__global__ __launch_bounds__(256) void cql_rsample_bwd_kernel(const CqlSampleBwdArgs a) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= a.M) return;
  const float* rw = a.raw + (size_t)m * a.rp;
  const float* e = a.eps + (size_t)m * a.ep;
  float* o = a.draw + (size_t)m * a.dwp;
  const float dl = a.dlogp[m];
  for (int d = 0; d < a.A; ++d) {
    const float lr = rw[a.A + d], ls = fminf(fmaxf(lr, -20.f), 2.f), sig = expf(ls), ev = e[d];
    const float th = tanhf(rw[d] + sig * ev);
    float dact = 0.f;
    if (a.da) dact = a.da[(size_t)m * a.dap + d];
    if (a.da2) dact += a.da2[(size_t)m * a.dap + d];
    const float du = dact * (1.f - th * th) + dl * (2.f * th);
    const float dls = (lr >= -20.f && lr <= 2.f) ? du * sig * ev - dl : 0.f;   // torch.clamp passes the gradient on [min, max]
    if (a.add) { o[d] += du; o[a.A + d] += dls; }
    else { o[d] = du; o[a.A + d] = dls; }
  }
}

// ---- loss heads: one workgroup of 1024 threads, thread t owns the rows t, t + 1024, ...; the per-thread sums are added through LDS
//      by the halving tree of rl_head.h --------------------------------------------------------------------------------------------------
struct CqlSacArgs {
  const float *logp, *q1, *q2; int B, tune; float target_entropy, lr, beta1, beta2, eps;
  float* la; int* step; float* alpha; float* losses; float* dlogp; float* dq1; float* dq2;
};
__global__ __launch_bounds__(1024) void cql_sac_head_kernel(const CqlSacArgs a) {
  __shared__ float red[2][1024];
  __shared__ float sh_alpha;
  const int t = threadIdx.x;
  const float inv_b = 1.f / (float)a.B;
  float sl = 0.f;
  for (int b = t; b < a.B; b += 1024) sl += a.logp[b];
  red[0][t] = sl; red[1][t] = 0.f;
  head_tree_sum<2>(red, t);
  const float mean_lp = red[0][0] * inv_b;
  if (t == 0) {
    float alpha = 1.f, alpha_loss = 0.f;
    if (a.tune) {
      // alpha_loss = -mean(log_alpha (log_pi + target_entropy)); its gradient from the OLD log_alpha, then Adam in the arithmetic of
      // adam_dev_kernel (misc.hip), then alpha from the NEW log_alpha
      const float la = a.la[0], g = -(mean_lp + a.target_entropy);
      alpha_loss = la * g;
      const int st = a.step[0] + 1;
      a.step[0] = st;
      const float bc1 = 1.f - powf(a.beta1, (float)st), bc2 = 1.f - powf(a.beta2, (float)st);
      const float lr_bc1 = a.lr / bc1, inv_sqrt_bc2 = rsqrtf(bc2);
      const float mm = __builtin_fmaf(a.beta1, a.la[1], (1.f - a.beta1) * g);
      const float vv = __builtin_fmaf(a.beta2, a.la[2], (1.f - a.beta2) * g * g);
      const float den = __builtin_fmaf(__builtin_amdgcn_sqrtf(vv), inv_sqrt_bc2, a.eps);
      const float nla = __builtin_fmaf(-lr_bc1 * mm, __builtin_amdgcn_rcpf(den), la);
      a.la[0] = nla; a.la[1] = mm; a.la[2] = vv;
      alpha = expf(nla);
    }
    sh_alpha = alpha;
    a.alpha[0] = alpha;
    if (a.losses) { a.losses[0] = alpha_loss; a.losses[2] = alpha * mean_lp; }
  }
  __syncthreads();
  const float alpha = sh_alpha;
  float sp = 0.f, ss = 0.f;
  for (int b = t; b < a.B; b += 1024) {
    const float lp = a.logp[b];
    float qm = 0.f;
    if (a.q1) {
      const float x1 = a.q1[b], x2 = a.q2[b];
      qm = fminf(x1, x2);
      // torch.min(a, b) hands the gradient to the smaller operand and splits it in halves on a tie
      if (a.dq1) a.dq1[b] = x1 < x2 ? -inv_b : (x1 == x2 ? -0.5f * inv_b : 0.f);
      if (a.dq2) a.dq2[b] = x2 < x1 ? -inv_b : (x1 == x2 ? -0.5f * inv_b : 0.f);
    }
    sp += alpha * lp - qm; ss += lp - qm;
    if (a.dlogp) a.dlogp[b] = alpha * inv_b;
  }
  if (!a.losses) return;                                     // (launch-uniform)
  __syncthreads();
  red[0][t] = sp; red[1][t] = ss;
  head_tree_sum<2>(red, t);
  if (t == 0) { a.losses[1] = red[0][0] * inv_b; a.losses[3] = red[1][0] * inv_b; }
}

struct CqlCriticArgs {
  const float* q_pred; long long qp_stride; const float* q_samp; long long qs_stride; const float* logp_samp; const float* tq;
  const float *new_log_pi, *alpha, *reward, *terminal; int B, R; float density, reward_scale, discount, temp, min_q_weight; int det;
  float* losses; float* dq_pred; long long dqp_stride; float* dq_samp; long long dqs_stride; float* q_target; float* std_mean;
};
__global__ __launch_bounds__(1024) void cql_critic_head_kernel(const CqlCriticArgs a) {
  __shared__ float red[8][1024];
  const int t = threadIdx.x, R3 = 3 * a.R;
  const float inv_b = 1.f / (float)a.B, wb = a.min_q_weight * inv_b;
  const float alpha = a.det ? 0.f : a.alpha[0];
  float sum[8] = {};                                         // per network i: [i] squared error, [2 + i] lse, [4 + i] q_pred, [6 + i] std
  for (int b = t; b < a.B; b += 1024) {
    float tqv = fminf(a.tq[b], a.tq[a.B + b]);
    if (!a.det) tqv -= alpha * a.new_log_pi[b];
    const float qt = a.reward_scale * a.reward[b] + (1.f - a.terminal[b]) * a.discount * tqv;
    if (a.q_target) a.q_target[b] = qt;
    const float* lps = a.logp_samp + (size_t)b * 2 * a.R;          // column j >= R of the samples pairs with logp_samp[b][j - R]
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float qp = a.q_pred[i * a.qp_stride + b], e = qp - qt;
      const float* qs = a.q_samp + i * a.qs_stride + (size_t)b * R3;
      float mx = -INFINITY, mean = qp;
      for (int j = 0; j < R3; ++j) {
        const float q = qs[j];
        mx = fmaxf(mx, (q - (j < a.R ? a.density : lps[j - a.R])) / a.temp);
        mean += q;
      }
      mean /= (float)(R3 + 1);
      float se = 0.f, var = (qp - mean) * (qp - mean);
      for (int j = 0; j < R3; ++j) {
        const float q = qs[j];
        se += expf((q - (j < a.R ? a.density : lps[j - a.R])) / a.temp - mx);
        var += (q - mean) * (q - mean);
      }
      sum[i] += e * e; sum[2 + i] += mx + logf(se); sum[4 + i] += qp; sum[6 + i] += sqrtf(var / (float)R3);
      if (a.dq_pred) a.dq_pred[i * a.dqp_stride + b] = 2.f * e * inv_b - wb;
      if (a.dq_samp) {
        float* o = a.dq_samp + i * a.dqs_stride + (size_t)b * R3;
        const float sc = wb / se;
        for (int j = 0; j < R3; ++j) o[j] = expf((qs[j] - (j < a.R ? a.density : lps[j - a.R])) / a.temp - mx) * sc;
      }
    }
  }
  if (!a.losses && !a.std_mean) return;                      // (launch-uniform)
#pragma unroll
  for (int s = 0; s < 8; ++s) red[s][t] = sum[s];
  head_tree_sum<8>(red, t);
  if (t < 2) {
    const float min_qf = red[2 + t][0] * inv_b * a.min_q_weight * a.temp - red[4 + t][0] * inv_b * a.min_q_weight;
    if (a.losses) { a.losses[t] = red[t][0] * inv_b + min_qf; a.losses[2 + t] = min_qf; }
    if (a.std_mean) a.std_mean[t] = red[6 + t][0] * inv_b;
  }
}

// ---- entry points -------------------------------------------------------------------------------------------------------------------
extern "C" int s2p_tanh_gauss_rsample(const float* raw, int raw_pitch, const float* eps, int eps_pitch, int M, int A, int rep,
                                      float* action, int action_pitch, int action_group, float* logp, int logp_group, float* u,
                                      int u_pitch, void* stream) {
  const char* who = "s2p_tanh_gauss_rsample";
  if (M < 0 || A < 0 || rep < 0) S2P_FAIL(-1, "%s: negative size", who);
  if (M == 0 || A == 0 || rep == 0) return 0;
  if (!raw || !eps) S2P_FAIL(-1, "%s: null tensor (raw and eps are required)", who);
  if (!action && !logp && !u) S2P_FAIL(-1, "%s: no output", who);
  if ((int64_t)raw_pitch < 2 * (int64_t)A || eps_pitch < A || (action && action_pitch < A) || (u && u_pitch < A))
    S2P_FAIL(-1, "%s: pitch shorter than the row", who);
  if ((action && action_group < rep) || (logp && logp_group < rep)) S2P_FAIL(-1, "%s: a row group shorter than rep", who);
  if ((int64_t)M * rep >= ((int64_t)1 << 31)) S2P_FAIL(-1, "%s: M * rep must stay below 2^31", who);
  CqlSampleArgs a{raw, raw_pitch, eps, eps_pitch, M, A, rep, action, action_pitch, action_group, logp, logp_group, u, u_pitch};
  hipLaunchKernelGGL(cql_rsample_kernel, dim3(cdiv((int64_t)M * rep, 256)), dim3(256), 0, (hipStream_t)stream, a);
  S2P_CHECK_LAUNCH("cql_rsample_kernel");
  return 0;
}

extern "C" int s2p_tanh_gauss_rsample_bwd(const float* raw, int raw_pitch, const float* eps, int eps_pitch, const float* dlogp,
                                          const float* daction, const float* daction2, int daction_pitch, int M, int A,
                                          float* draw, int draw_pitch, int accumulate, void* stream) {
  const char* who = "s2p_tanh_gauss_rsample_bwd";
  if (M < 0 || A < 0) S2P_FAIL(-1, "%s: negative size", who);
  if (M == 0 || A == 0) return 0;
  if (!raw || !eps || !dlogp || !draw) S2P_FAIL(-1, "%s: null tensor (raw, eps, dlogp, draw are required)", who);
  if (daction2 && !daction) S2P_FAIL(-1, "%s: daction2 without daction", who);
  if ((int64_t)raw_pitch < 2 * (int64_t)A || eps_pitch < A || (int64_t)draw_pitch < 2 * (int64_t)A || (daction && daction_pitch < A))
    S2P_FAIL(-1, "%s: pitch shorter than the row", who);
  CqlSampleBwdArgs a{raw, raw_pitch, eps, eps_pitch, dlogp, daction, daction2, daction_pitch, M, A, draw, draw_pitch, accumulate != 0};
  hipLaunchKernelGGL(cql_rsample_bwd_kernel, dim3(cdiv(M, 256)), dim3(256), 0, (hipStream_t)stream, a);
  S2P_CHECK_LAUNCH("cql_rsample_bwd_kernel");
  return 0;
}

extern "C" int s2p_sac_policy_head(const float* logp, const float* q1, const float* q2, int B, int tune, float target_entropy,
                                   float lr, float beta1, float beta2, float eps, float* log_alpha_state, int* step_dev,
                                   float* alpha, float* losses, float* dlogp, float* dq1, float* dq2, void* stream) {
  const char* who = "s2p_sac_policy_head";
  if (B < 0) S2P_FAIL(-1, "%s: negative size", who);
  if (B == 0) return 0;
  if (!logp || !alpha) S2P_FAIL(-1, "%s: null tensor (logp and alpha are required)", who);
  if ((q1 == nullptr) != (q2 == nullptr)) S2P_FAIL(-1, "%s: q1 and q2 come together", who);
  if ((dq1 || dq2) && !q1) S2P_FAIL(-1, "%s: dq1 / dq2 need q1 and q2", who);
  if (tune && (!log_alpha_state || !step_dev)) S2P_FAIL(-1, "%s: tuning needs the log_alpha state and its step counter", who);
  CqlSacArgs a{logp, q1, q2, B, tune != 0, target_entropy, lr, beta1, beta2, eps, log_alpha_state, step_dev, alpha, losses, dlogp, dq1, dq2};
  hipLaunchKernelGGL(cql_sac_head_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
  S2P_CHECK_LAUNCH("cql_sac_head_kernel");
  return 0;
}

extern "C" int s2p_cql_critic_head(const float* q_pred, int64_t q_pred_stride, const float* q_samp, int64_t q_samp_stride,
                                   const float* logp_samp, const float* tq, const float* new_log_pi, const float* alpha,
                                   const float* reward, const float* terminal, int B, int R, int A, float reward_scale,
                                   float discount, float temp, float min_q_weight, int deterministic_backup, float* losses,
                                   float* dq_pred, int64_t dq_pred_stride, float* dq_samp, int64_t dq_samp_stride, float* q_target,
                                   float* std_mean, void* stream) {
  const char* who = "s2p_cql_critic_head";
  if (B < 0 || R < 0 || A < 0) S2P_FAIL(-1, "%s: negative size", who);
  if (B == 0) return 0;
  if (R == 0) S2P_FAIL(-1, "%s: num_random must be at least 1", who);
  if (!q_pred || !q_samp || !logp_samp || !tq || !reward || !terminal) S2P_FAIL(-1, "%s: null tensor (q_pred, q_samp, logp_samp, tq, reward, terminal are required)", who);
  if (!deterministic_backup && (!new_log_pi || !alpha)) S2P_FAIL(-1, "%s: the entropy backup needs new_log_pi and alpha", who);
  if (!losses && !dq_pred && !dq_samp && !q_target && !std_mean) S2P_FAIL(-1, "%s: no output", who);
  if (!(temp > 0.f)) S2P_FAIL(-1, "%s: temp must be positive", who);
  if (q_pred_stride < B || q_samp_stride < (int64_t)B * 3 * R || (dq_pred && dq_pred_stride < B) || (dq_samp && dq_samp_stride < (int64_t)B * 3 * R))
    S2P_FAIL(-1, "%s: a network stride shorter than the block", who);
  if ((int64_t)B * 3 * R >= ((int64_t)1 << 31)) S2P_FAIL(-1, "%s: B * 3 R must stay below 2^31", who);
  const float density = (float)log(pow(0.5, (double)A));     // np.log(0.5 ** A), rounded once as the reference's fp32 run rounds it
  CqlCriticArgs a{q_pred, q_pred_stride, q_samp, q_samp_stride, logp_samp, tq, new_log_pi, alpha, reward, terminal, B, R, density,
                  reward_scale, discount, temp, min_q_weight, deterministic_backup != 0, losses, dq_pred, dq_pred_stride, dq_samp,
                  dq_samp_stride, q_target, std_mean};
  hipLaunchKernelGGL(cql_critic_head_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
  S2P_CHECK_LAUNCH("cql_critic_head_kernel");
  return 0;
}
