// The SLAC latent model's Gaussian heads and likelihood terms (SPEC.md N3b; rlkit/torch/slac/network/latent.py:174-311), all fp32.
// The posterior chain is 9 strictly sequential time steps of two 3-layer MLPs at M = batch rows: latency-bound like the state path
// (linear_small.hip).  By default a layer is one short launch.  A call that keeps no backward state can run the whole chain as ONE
// launch instead (gauss_chain.hip, LatentModel.fused_chain), and one that does keep it as one launch that also stores every
// activation, with the sequential part of its backward as one more (LatentModel.fused_chain_grad): all built from the same device
// functions (gauss_dev.h) and bitwise equal.  The chain's linear layers, with the additive term that takes the
// part of a first layer's input the chain does not produce, are in linear_small.hip.  This file holds the heads and the three
// losses, so that NO torch.cat / chunk / stack / element-wise kernel runs between the per-layer launches:
//   gauss_head_{fwd,bwd}_kernel : [mean | raw] -> mean, std = softplus(raw) + 1e-5, z = mean + eps * std, every output with its own
//                                 pitch and column offset (the sample to two places: the sequence buffer and the next MLP's input
//                                 row); backward [dmean + dz | (dstd + dz eps) sigmoid(raw)].
//   gauss_kl_kernel, gauss_ll_kernel, gauss_ll_image_kernel : loss value and every gradient in one pass.
// Reductions: the KL and the masked (reward) likelihood are ONE workgroup each, summed in a fixed order, no atomics.  The image
// likelihood (8.6 M elements at B = 32) ends in ONE fp32 atomicAdd per workgroup on the loss word, as s2p_l1_loss does: its VALUE
// can differ in the last bits between calls, its gradient cannot (element-wise).
#include "gauss_dev.h"

// ---- Gaussian head ---------------------------------------------------------------------------------------------------------------
struct HeadArgs {
  const float* raw; const float* eps; float* mean; float* std; float* z; float* z2;
  const float* dmean; const float* dstd; const float* dz; const float* dz2; float* draw;
  int M, D, raw_pitch, eps_pitch, mean_pitch, std_pitch, z_pitch, z2_pitch;
  int dmean_pitch, dstd_pitch, dz_pitch, dz2_pitch, draw_pitch;
};

__global__ __launch_bounds__(256) void gauss_head_fwd_kernel(const HeadArgs a) {
  const long long total = (long long)a.M * a.D;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int m = (int)(idx / a.D), d = (int)(idx - (long long)m * a.D);
    const float* r = a.raw + (size_t)m * a.raw_pitch;
    const float mu = r[d], sd = gauss_head_std(r[a.D + d]);
    if (a.mean) a.mean[(size_t)m * a.mean_pitch + d] = mu;
    if (a.std) a.std[(size_t)m * a.std_pitch + d] = sd;
    if (a.eps) {
      const float zv = gauss_head_sample(a.eps[(size_t)m * a.eps_pitch + d], sd, mu);
      if (a.z) a.z[(size_t)m * a.z_pitch + d] = zv;
      if (a.z2) a.z2[(size_t)m * a.z2_pitch + d] = zv;
    }
  }
}

__global__ __launch_bounds__(256) void gauss_head_bwd_kernel(const HeadArgs a) {
  const long long total = (long long)a.M * a.D;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int m = (int)(idx / a.D), d = (int)(idx - (long long)m * a.D);
    const GaussHeadGrad g = gauss_head_grad(a.dz, a.dz ? a.dz[(size_t)m * a.dz_pitch + d] : 0.f,
                                            a.dz2, a.dz2 ? a.dz2[(size_t)m * a.dz2_pitch + d] : 0.f,
                                            a.dmean, a.dmean ? a.dmean[(size_t)m * a.dmean_pitch + d] : 0.f,
                                            a.dstd, a.dstd ? a.dstd[(size_t)m * a.dstd_pitch + d] : 0.f,
                                            a.eps, a.eps ? a.eps[(size_t)m * a.eps_pitch + d] : 0.f,
                                            a.raw[(size_t)m * a.raw_pitch + a.D + d]);
    float* o = a.draw + (size_t)m * a.draw_pitch;
    o[d] = g.dmu;
    o[a.D + d] = g.draw_std;
  }
}

static inline int gauss_grid(long long total, int cap = 1024) {
  long long b = (total + 255) / 256; if (b > cap) b = cap; if (b < 1) b = 1; return (int)b;
}

extern "C" int s2p_gauss_head_fwd(const float* raw, int raw_pitch, int M, int D, const float* eps, int eps_pitch, float* mean,
                                  int mean_pitch, float* std, int std_pitch, float* z, int z_pitch, float* z2, int z2_pitch,
                                  void* stream) {
  S2P_REQUIRE(M >= 0 && D >= 0, "s2p_gauss_head_fwd: negative size");
  if (M == 0 || D == 0) return 0;
  S2P_REQUIRE(raw && raw_pitch >= 2 * D, "s2p_gauss_head_fwd: raw is NULL or its pitch is below 2 D");
  S2P_REQUIRE(mean || std || z || z2, "s2p_gauss_head_fwd: no output");
  S2P_REQUIRE((!z && !z2) || eps, "s2p_gauss_head_fwd: a sample needs eps");
  S2P_REQUIRE((!eps || eps_pitch >= D) && (!mean || mean_pitch >= D) && (!std || std_pitch >= D) && (!z || z_pitch >= D) &&
              (!z2 || z2_pitch >= D), "s2p_gauss_head_fwd: a pitch is below D");
  HeadArgs a{}; a.raw = raw; a.raw_pitch = raw_pitch; a.M = M; a.D = D; a.eps = eps; a.eps_pitch = eps_pitch; a.mean = mean;
  a.mean_pitch = mean_pitch; a.std = std; a.std_pitch = std_pitch; a.z = z; a.z_pitch = z_pitch; a.z2 = z2; a.z2_pitch = z2_pitch;
  hipLaunchKernelGGL(gauss_head_fwd_kernel, dim3(gauss_grid((long long)M * D)), dim3(256), 0, (hipStream_t)stream, a);
  S2P_CHECK_LAUNCH("gauss_head_fwd_kernel");
  return 0;
}

extern "C" int s2p_gauss_head_bwd(const float* raw, int raw_pitch, int M, int D, const float* eps, int eps_pitch,
                                  const float* dmean, int dmean_pitch, const float* dstd, int dstd_pitch, const float* dz,
                                  int dz_pitch, const float* dz2, int dz2_pitch, float* draw, int draw_pitch, void* stream) {
  S2P_REQUIRE(M >= 0 && D >= 0, "s2p_gauss_head_bwd: negative size");
  if (M == 0 || D == 0) return 0;
  S2P_REQUIRE(raw && raw_pitch >= 2 * D && draw && draw_pitch >= 2 * D, "s2p_gauss_head_bwd: raw / draw is NULL or its pitch is below 2 D");
  S2P_REQUIRE((!dz && !dz2) || eps, "s2p_gauss_head_bwd: the gradient of a sample needs eps");
  S2P_REQUIRE((!eps || eps_pitch >= D) && (!dmean || dmean_pitch >= D) && (!dstd || dstd_pitch >= D) && (!dz || dz_pitch >= D) &&
              (!dz2 || dz2_pitch >= D), "s2p_gauss_head_bwd: a pitch is below D");
  HeadArgs a{}; a.raw = raw; a.raw_pitch = raw_pitch; a.M = M; a.D = D; a.eps = eps; a.eps_pitch = eps_pitch; a.dmean = dmean;
  a.dmean_pitch = dmean_pitch; a.dstd = dstd; a.dstd_pitch = dstd_pitch; a.dz = dz; a.dz_pitch = dz_pitch; a.dz2 = dz2;
  a.dz2_pitch = dz2_pitch; a.draw = draw; a.draw_pitch = draw_pitch;
  hipLaunchKernelGGL(gauss_head_bwd_kernel, dim3(gauss_grid((long long)M * D)), dim3(256), 0, (hipStream_t)stream, a);
  S2P_CHECK_LAUNCH("gauss_head_bwd_kernel");
  return 0;
}

// ---- losses: value and gradients in one pass -----------------------------------------------------------------------------------------
// sum of the 256 threads' values in a fixed order (wave shuffles, then the four wave sums in wave order); valid in thread 0
__device__ __forceinline__ float gauss_block_sum(float v) {
  __shared__ float part[4];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return part[0] + part[1] + part[2] + part[3];
}

struct KlArgs {
  const float* mu_p; const float* std_p; const float* mu_q; const float* std_q;
  float* dmu_p; float* dstd_p; float* dmu_q; float* dstd_q; float* loss;
  int B, T, D, p_pitch, q_pitch, dp_pitch, dq_pitch, const_first; float scale;
};

// ONE workgroup: thread i takes the elements i, i + 256, ... in order; fixed-order block sum; loss[0] += scale * sum (a plain add)
__global__ __launch_bounds__(256) void gauss_kl_kernel(const KlArgs a) {
  const long long total = (long long)a.B * a.T * a.D;
  const int Tq = a.const_first ? a.T - 1 : a.T;
  float s = 0.f;
  for (long long idx = threadIdx.x; idx < total; idx += 256) {
    const int d = (int)(idx % a.D); const long long row = idx / a.D;
    const int t = (int)(row % a.T), b = (int)(row / a.T);
    const float mp = a.mu_p[(size_t)row * a.p_pitch + d], sp = a.std_p[(size_t)row * a.p_pitch + d];
    const bool cst = a.const_first && t == 0;
    const size_t qrow = cst ? 0 : (size_t)b * Tq + (a.const_first ? t - 1 : t);
    const float mq = cst ? 0.f : a.mu_q[qrow * a.q_pitch + d], sq = cst ? 1.f : a.std_q[qrow * a.q_pitch + d];
    const float rq = 1.f / sq, ratio = sp * rq, vr = ratio * ratio, dm = (mp - mq) * rq, t1 = dm * dm;
    s += 0.5f * (vr + t1 - 1.f - logf(vr));
    if (a.dmu_p) a.dmu_p[(size_t)row * a.dp_pitch + d] = a.scale * dm * rq;
    if (a.dstd_p) a.dstd_p[(size_t)row * a.dp_pitch + d] = a.scale * (sp * rq * rq - 1.f / sp);
    if (!cst) {
      if (a.dmu_q) a.dmu_q[qrow * a.dq_pitch + d] = -a.scale * dm * rq;
      if (a.dstd_q) a.dstd_q[qrow * a.dq_pitch + d] = a.scale * rq * (1.f - vr - t1);
    }
  }
  s = gauss_block_sum(s);
  if (threadIdx.x == 0) a.loss[0] += a.scale * s;
}

extern "C" int s2p_gauss_kl(const float* mu_p, const float* std_p, int p_pitch, const float* mu_q, const float* std_q, int q_pitch,
                            int B, int T, int D, int const_first, float scale, float* loss, float* dmu_p, float* dstd_p,
                            int dp_pitch, float* dmu_q, float* dstd_q, int dq_pitch, void* stream) {
  S2P_REQUIRE(B >= 0 && T >= 0 && D >= 0, "s2p_gauss_kl: negative size");
  if (B == 0 || T == 0 || D == 0) return 0;
  const bool need_q = !(const_first && T == 1);
  S2P_REQUIRE(mu_p && std_p && loss && p_pitch >= D, "s2p_gauss_kl: null pointer or p_pitch below D");
  S2P_REQUIRE(!need_q || (mu_q && std_q && q_pitch >= D), "s2p_gauss_kl: the prior is NULL or q_pitch below D");
  S2P_REQUIRE((!dmu_p && !dstd_p) || dp_pitch >= D, "s2p_gauss_kl: dp_pitch below D");
  S2P_REQUIRE((!dmu_q && !dstd_q) || dq_pitch >= D, "s2p_gauss_kl: dq_pitch below D");
  KlArgs a{}; a.mu_p = mu_p; a.std_p = std_p; a.p_pitch = p_pitch; a.mu_q = mu_q; a.std_q = std_q; a.q_pitch = q_pitch; a.B = B; a.T = T;
  a.D = D; a.const_first = const_first ? 1 : 0; a.scale = scale; a.loss = loss; a.dmu_p = dmu_p; a.dstd_p = dstd_p; a.dp_pitch = dp_pitch;
  a.dmu_q = dmu_q; a.dstd_q = dstd_q; a.dq_pitch = dq_pitch;
  hipLaunchKernelGGL(gauss_kl_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
  S2P_CHECK_LAUNCH("gauss_kl_kernel");
  return 0;
}

#define GAUSS_HALF_LOG_2PI 0.91893853320467274178f

// masked likelihood of n scalars (the reward term): ONE workgroup, fixed order, no atomics
__global__ __launch_bounds__(256) void gauss_ll_kernel(const float* mu, int mu_pitch, const float* sd, int sd_pitch, const float* target,
                                                       const float* done, long long n, float scale, float* loss, float* dmu,
                                                       float* dsd) {
  float s = 0.f;
  for (long long i = threadIdx.x; i < n; i += 256) {
    const float m = mu[(size_t)i * mu_pitch], sg = sd[(size_t)i * sd_pitch], keep = done ? 1.f - done[i] : 1.f;
    const float inv = 1.f / (sg + 1e-8f), nz = (target[i] - m) * inv;
    s += keep * (0.5f * nz * nz + logf(sg) + GAUSS_HALF_LOG_2PI);
    if (dmu) dmu[i] = -scale * keep * nz * inv;
    if (dsd) dsd[i] = scale * keep * (1.f / sg - nz * nz * inv);
  }
  s = gauss_block_sum(s);
  if (threadIdx.x == 0) loss[0] += scale * s;
}

extern "C" int s2p_gauss_ll(const float* mu, int mu_pitch, const float* std, int std_pitch, const float* target, const float* done,
                            int64_t n, float scale, float* loss, float* dmu, float* dstd, void* stream) {
  S2P_REQUIRE(n >= 0, "s2p_gauss_ll: negative size");
  if (n == 0) return 0;
  S2P_REQUIRE(mu && std && target && loss, "s2p_gauss_ll: null pointer");
  S2P_REQUIRE(mu_pitch >= 1 && std_pitch >= 1, "s2p_gauss_ll: a pitch is below 1");
  hipLaunchKernelGGL(gauss_ll_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, mu, mu_pitch, std, std_pitch, target, done,
                     (long long)n, scale, loss, dmu, dstd);
  S2P_CHECK_LAUNCH("gauss_ll_kernel");
  return 0;
}

// image likelihood with a constant sigma.  mu: NHWC [N][HW][pitch] in T (the decoder's output), target: fp32 NCHW [N][C][HW]
// (TU8 == 0) or uint8 NHWC [N][HW][C] read as u8 / 255 (TU8 == 1); dmu in mu's layout and dtype, padded channels written as zero.
// A thread owns a pixel: 16-byte chunks of mu / dmu, coalesced target reads per channel plane.
template <typename T, int TU8>
__global__ __launch_bounds__(256) void gauss_ll_image_kernel(const T* mu, int pitch, const void* target, long long pixels, int HW, int C,
                                                             float sigma, float scale, float* loss, T* dmu) {
  constexpr int CE = DT<T>::CE;
  const float inv = 1.f / (sigma + 1e-8f), cst = logf(sigma) + GAUSS_HALF_LOG_2PI;
  const IdxDiv dv(HW, pixels < (1ll << 31));
  float s = 0.f;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < pixels; p += (long long)gridDim.x * 256) {
    int hw; const long long n = dv.split(p, hw);
    for (int c0 = 0; c0 < pitch; c0 += CE) {
      Chunk<T> mv, gv;
      gv.raw = (u32x4){0u, 0u, 0u, 0u};
      mv.raw = *(const u32x4*)(mu + p * pitch + c0);
#pragma unroll
      for (int e = 0; e < CE; ++e) {
        const int c = c0 + e;
        float g = 0.f;
        if (c < C) {
          const float x = TU8 ? (float)((const unsigned char*)target)[p * C + c] * (1.f / 255.f)
                              : ((const float*)target)[(n * C + c) * HW + hw];
          const float nz = (x - mv.get(e)) * inv;
          s += 0.5f * nz * nz + cst;
          g = -scale * nz * inv;
        }
        gv.set(e, g);
      }
      if (dmu) *(u32x4*)(dmu + p * pitch + c0) = gv.raw;
    }
  }
  s = gauss_block_sum(s);
  if (threadIdx.x == 0) atomicAdd(loss, scale * s);
}

extern "C" int s2p_gauss_ll_image(int dtype, const void* mu, int pitch, const void* target, int target_u8, int N, int C, int HW,
                                  float sigma, float scale, float* loss, void* dmu, void* stream) {
  S2P_REQUIRE(s2p_is_dtype(dtype), "s2p_gauss_ll_image: bad dtype");
  S2P_REQUIRE(N >= 0 && C >= 0 && HW >= 0, "s2p_gauss_ll_image: negative size");
  if (N == 0 || C == 0 || HW == 0) return 0;
  const int ce = s2p_chunk_elems(dtype);
  S2P_REQUIRE(mu && target && loss, "s2p_gauss_ll_image: null pointer");
  S2P_REQUIRE(pitch >= C && pitch % ce == 0, "s2p_gauss_ll_image: pitch must be a multiple of %d and at least C", ce);
  S2P_REQUIRE(s2p_al16(mu, dmu), "s2p_gauss_ll_image: mu and dmu must be 16-byte aligned");
  S2P_REQUIRE(target_u8 || ((uintptr_t)target & 3) == 0, "s2p_gauss_ll_image: an fp32 target must be 4-byte aligned");
  S2P_REQUIRE(sigma > 0.f, "s2p_gauss_ll_image: sigma must be positive");
  const long long pixels = (long long)N * HW;
  const dim3 g(gauss_grid(pixels, 512));                   // one atomicAdd per workgroup on the loss word (see s2p_l1_loss)
  s2p_with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    auto kernel = target_u8 ? gauss_ll_image_kernel<T, 1> : gauss_ll_image_kernel<T, 0>;
    hipLaunchKernelGGL(kernel, g, dim3(256), 0, (hipStream_t)stream, (const T*)mu, pitch, target, pixels, HW, C, sigma, scale, loss, (T*)dmu);
  });
  S2P_CHECK_LAUNCH("gauss_ll_image_kernel");
  return 0;
}
