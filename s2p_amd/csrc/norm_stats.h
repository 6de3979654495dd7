// The InstanceNorm statistics buffer's format and the per-(image, channel) arithmetic that its producers and consumers must agree
// on bit for bit: norm.hip's kernels and the fused norm tails of the plane-resident convs (conv_plane_epi.h).  The single copy.
//   stats : fp32 buffer: STATS_HDR header words {S, rows per split, 0, 0}, then [N][C][S]{mean_b, M2_b}, the moments of the S pixel
//           splits of a plane (split b holds pixels [b rows, min(HW, (b + 1) rows))).  A fused launch writes S = 1, rows = HW.
#pragma once
#include "s2p_common.h"

constexpr int STATS_HDR = 4;        // header words in front of the partial moments

// the header: written by one thread of the launch that produces the moments
__device__ __forceinline__ void stats_store_header(float* stats, int S, int rows) { *(i32x4*)stats = (i32x4){S, rows, 0, 0}; }

// {mean_b, M2_b} of split s of channel c of image n, in a buffer of S splits
template <typename F>    // F: float or const float
__host__ __device__ __forceinline__ F* stats_slot(F* stats, int n, int C, int c, int S, unsigned s) { return stats + STATS_HDR + (((size_t)n * C + c) * S + s) * 2; }

// merge the per-split partial moments of channel c of image n with Chan's formula (fixed order: bitwise reproducible).  C, HW and eps
// by reference: a kernel argument is then read where the loop uses it, as in the copies of this loop the kernels had (read at the call,
// the same instructions come out in another order and with other registers)
__device__ __forceinline__ void stats_mean_rstd(const float* stats, int n, const int& C, int c, const int& HW, const float& eps,
                                                float& mean, float& rstd) {
  const int S = ((const int*)stats)[0], rows = ((const int*)stats)[1];
  const float* p = stats_slot(stats, n, C, c, S, 0);
  const float inv = 1.f / (float)HW;
  const float m0 = p[0];                               // merge about the first split's mean: the differences are O(std)
  float m = 0.f;
  for (int b = 1; b < S; ++b) { int nb = HW - b * rows; if (nb > rows) nb = rows; m += (float)nb * (p[2 * b] - m0); }
  m = m0 + m * inv;
  float M2 = 0.f;
  for (int b = 0; b < S; ++b) { int nb = HW - b * rows; if (nb > rows) nb = rows; const float d = p[2 * b] - m; M2 += p[2 * b + 1] + (float)nb * d * d; }
  mean = m; rstd = 1.f / sqrtf(M2 * inv + eps);
}

// the per-sample state affine of channel c of image n: (1 + gamma_st, beta_st); gbst = fp32 [N][pitch], gamma at [0, C), beta at
// [C, 2C); NULL: (1, 0).  (norm.hip's kernels; the conv tails read gbst through a pointer and keep their two selects: there the
// compiler may not merge the loads across the LDS stores, and the helper's one branch gives other instructions)
struct StateAffine { float g1, b1; };
__device__ __forceinline__ StateAffine state_affine(const float* gbst, int pitch, int n, int c, int C) {
  StateAffine s = {1.f, 0.f};
  if (gbst) { s.g1 = 1.f + gbst[(size_t)n * pitch + c]; s.b1 = gbst[(size_t)n * pitch + C + c]; }
  return s;
}

// the modulated value, written ONCE so that forward, backward-reduce and backward-apply round identically (the backward re-derives
// the activation mask from it).  _centred: from d = x - mean, for the kernels that keep the centred plane in registers
__device__ __forceinline__ float mat_value_centred(float d, float rstd, float gg, float bb, float& xh) { xh = d * rstd; return __builtin_fmaf(xh, gg, bb); }
__device__ __forceinline__ float mat_value(float x, float mean, float rstd, float gg, float bb, float& xh) { return mat_value_centred(x - mean, rstd, gg, bb, xh); }
