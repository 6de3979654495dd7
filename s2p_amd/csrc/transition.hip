// State-transition rollout (SPEC.md N2c; reference state_transition_rollout.py:149, 180): raw observations and drawn actions of a
// whole dataset -> the ensemble's first-layer input  x = [(obs - obs_mean) / obs_std | action | 0 ...]  in ONE launch.
// The subtraction and the division are two separately rounded IEEE fp32 operations (a true division: no reciprocal, nothing to
// contract), so x is bit for bit numpy's fp32 `(obs - mean) / std`, which is what the reference feeds its network.
// Row offsets are 64-bit: a dataset is 5e5 .. 1e7 rows.
#include "s2p_common.h"

#pragma clang fp contract(off)

struct TransPackArgs {
  const float* obs; const float* action; const float* mean; const float* std; float* x;
  long long rows; int obs_pitch, act_pitch, obs_dim, act_dim, x_pitch;
};

__device__ __forceinline__ float trans_pack_elem(const TransPackArgs& a, long long r, int j) {
  if (j < a.obs_dim) {
    const float d = a.obs[(size_t)r * a.obs_pitch + j] - a.mean[j];
    return d / a.std[j];
  }
  if (j < a.obs_dim + a.act_dim) return a.action[(size_t)r * a.act_pitch + (j - a.obs_dim)];
  return 0.f;
}

// x_pitch % 4 == 0 and x 16-byte aligned: a thread step is one 16-byte chunk of a row (the form the ensemble layers read)
__global__ __launch_bounds__(256) void transition_pack4_kernel(const TransPackArgs a, bool fast) {
  const int c4 = a.x_pitch >> 2;
  const IdxDiv dv(c4, fast);
  const long long total = a.rows * c4;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    int ch;
    const long long r = dv.split(idx, ch);
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = trans_pack_elem(a, r, 4 * ch + e);
    Chunk<float> o; o.pack(v);
    *(u32x4*)(a.x + (size_t)r * a.x_pitch + 4 * ch) = o.raw;
  }
}

// any pitch, any alignment: one element per thread step
__global__ __launch_bounds__(256) void transition_pack1_kernel(const TransPackArgs a, bool fast) {
  const IdxDiv dv(a.x_pitch, fast);
  const long long total = a.rows * a.x_pitch;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    int j;
    const long long r = dv.split(idx, j);
    a.x[(size_t)r * a.x_pitch + j] = trans_pack_elem(a, r, j);
  }
}

extern "C" int s2p_transition_pack(const float* obs, int obs_pitch, const float* action, int act_pitch, const float* obs_mean,
                                   const float* obs_std, int64_t rows, int obs_dim, int act_dim, float* x, int x_pitch,
                                   void* stream) {
  const char* who = "s2p_transition_pack";
  if (rows < 0 || obs_dim < 0 || act_dim < 0 || obs_pitch < 0 || act_pitch < 0 || x_pitch < 0) S2P_FAIL(-1, "%s: negative size", who);
  if ((int64_t)x_pitch < (int64_t)obs_dim + act_dim || obs_pitch < obs_dim || act_pitch < act_dim)
    S2P_FAIL(-1, "%s: pitch shorter than the row", who);
  if (rows == 0 || x_pitch == 0) return 0;
  if (!x || (obs_dim && (!obs || !obs_mean || !obs_std)) || (act_dim && !action))
    S2P_FAIL(-1, "%s: null tensor (x, and obs / obs_mean / obs_std / action where their width is not 0)", who);
  if (rows > (int64_t)1 << 40) S2P_FAIL(-1, "%s: more than 2^40 rows", who);
  const TransPackArgs a{obs, action, obs_mean, obs_std, x, (long long)rows, obs_pitch, act_pitch, obs_dim, act_dim, x_pitch};
  const bool vec = x_pitch % 4 == 0 && s2p_al16(x);
  const long long total = (long long)rows * (vec ? x_pitch / 4 : x_pitch);
  const bool fast = total < ((long long)1 << 31);             // IdxDiv: the reciprocal split below 2^31, 64-bit division above
  long long blocks = (total + 255) / 256;
  const long long cap = (long long)s2p_num_cus() * 16;
  if (blocks > cap) blocks = cap;
  if (vec) hipLaunchKernelGGL(transition_pack4_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, fast);
  else hipLaunchKernelGGL(transition_pack1_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, fast);
  S2P_CHECK_LAUNCH("transition_pack_kernel");
  return 0;
}
