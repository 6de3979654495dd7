// Device functions shared by the kernels of the SLAC Gaussian heads (linear_small.hip, gauss.hip, and through gauss_chain_common.h
// gauss_chain.hip and gauss_chain_bf16.hip).  The fused
// posterior chain returns bitwise what the per-layer launches return BECAUSE both are made of these: the same MFMA sequence per
// k-chunk, the same softplus, the same sample -- and, for the backward chain, the same head gradient.
#pragma once
#include "s2p_common.h"

// One k-chunk of 16 of the fp32 16x16x4 MFMA tile: lane 16 j + i holds x[row i][16 c + 4 j .. + 3] and w[col i][16 c + 4 j .. + 3];
// MFMA e consumes component e of both.  An output element is acc after "for chunk c ascending: lin_mfma_chunk" from 0.
__device__ __forceinline__ f32x4 lin_mfma_chunk(const f32x4 xv, const f32x4 wv, f32x4 acc) {
#pragma unroll
  for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[e], wv[e], acc, 0, 0, 0);
  return acc;
}

__device__ __forceinline__ float gauss_softplus(float r) { return fmaxf(r, 0.f) + log1pf(expf(-fabsf(r))); }
__device__ __forceinline__ float gauss_sigmoid(float r) {
  const float e = expf(-fabsf(r));
  return r >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}
// std of a Gaussian head from its raw output, and the reparameterised sample
__device__ __forceinline__ float gauss_head_std(float raw) { return gauss_softplus(raw) + 1e-5f; }
__device__ __forceinline__ float gauss_head_sample(float eps, float sd, float mu) { return __builtin_fmaf(eps, sd, mu); }

// Backward of one head element -> the gradient at [mean | raw_std].  A term that is ABSENT (its flag false) is not added: x + 0 is
// not bitwise x for -0.  gauss_head_bwd_kernel (a flag = "the pointer was given") and the fused backward chain both call this.
struct GaussHeadGrad { float dmu, draw_std; };
__device__ __forceinline__ GaussHeadGrad gauss_head_grad(bool has_dz, float dz, bool has_dz2, float dz2, bool has_dmean, float dmean,
                                                         bool has_dstd, float dstd, bool has_eps, float eps, float raw_std) {
  float gz = 0.f;
  if (has_dz) gz = dz;
  if (has_dz2) gz += dz2;
  float gm = gz, gs = 0.f;
  if (has_dmean) gm += dmean;
  if (has_dstd) gs = dstd;
  if (has_eps) gs = __builtin_fmaf(gz, eps, gs);
  return {gm, gs * gauss_sigmoid(raw_std)};
}
