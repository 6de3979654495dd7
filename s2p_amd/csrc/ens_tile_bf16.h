// The wave tiles of ens_tile.h in bf16 compute (SPEC.md N3l), for the s2p_mlp_linear_*_bf16 entry points of mlp.hip.  Every tensor
// stays fp32 in memory; a tile rounds both operands of every product to bf16 (round-to-nearest-even, v_cvt_pk_bf16_f32) as it loads
// them and sums the products in fp32 on v_mfma_f32_32x32x16_bf16.  The lane map is that of ens_tile.h (lane l owns row / column
// l & 31, result register r is row ens_row(r, l >> 5)): lane half h holds EIGHT summation indices per MFMA where the fp32 tile holds
// one, the same eight on both operands, so the tile shapes, the grid mapping and every address stay those of the fp32 tiles.  The
// bias add, ReLU, the mask and the stores are fp32.  Operands straight from global memory (no LDS), no atomics, a fixed summation
// order.  Every operand load is UNCONDITIONAL from an address clamped into the tensor, and a lane outside the tile selects zero
// afterwards: a load under a condition becomes a branch with a wait of its own, which a 32-cycle MFMA does not hide.
#pragma once
#include "ens_tile.h"

// eight fp32 values -> one operand fragment, each rounded to nearest even
__device__ __forceinline__ bf16x8 ens_bf16x8(const f32x4& lo, const f32x4& hi) {
  bf16x8 r;
#pragma unroll
  for (int c = 0; c < 4; ++c) { r[c] = (__bf16)lo[c]; r[4 + c] = (__bf16)hi[c]; }
  return r;
}
__device__ __forceinline__ bf16x8 ens_bf16x8(const float (&v)[8]) {
  bf16x8 r;
#pragma unroll
  for (int c = 0; c < 8; ++c) r[c] = (__bf16)v[c];
  return r;
}

// ---- forward: pre[m][n] = sum_k bf16(x[m][k]) bf16(w[n][k]) + bias[n];  act = ACT(pre) ------------------------------------------------
// 32 rows x 64 columns per wave.  A k-step of 16 is two float4 per lane and operand (lane half h takes k = 16 t + 8 h .. + 7) and one
// MFMA per accumulator.  K is a multiple of 4: a float4 is in or out, and a step partly past K loads zeros.
template <int ACT> __device__ __forceinline__ void ens_fwd_tile_bf16(const EnsFwdTile& a, int mb, int nb) {
  constexpr int U = 2;
  const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
  const bool two = nb + 32 < a.N;                            // (wave-uniform)
  const int m = mb + i, n0 = nb + i, n1 = nb + 32 + i;
  const bool mok = m < a.B, n0ok = n0 < a.N, n1ok = two && n1 < a.N;
  const float* xr = a.x + (size_t)(mok ? m : 0) * a.xp;
  const float* w0 = a.w + (size_t)(n0ok ? n0 : 0) * a.K;
  const float* w1 = a.w + (size_t)(n1ok ? n1 : 0) * a.K;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x16 acc0 = {}, acc1 = {};
  for (int kc = 0; kc < a.K; kc += 16 * U) {
    f32x4 xv[U][2], wv0[U][2], wv1[U][2];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int k = kc + 16 * u + 8 * h + 4 * p;
        const bool in = k < a.K;
        const int kk = in ? k : 0;                           // (K >= 4: the first float4 of a row is always there)
        const f32x4 xl = *(const f32x4*)(xr + kk), l0 = *(const f32x4*)(w0 + kk), l1 = *(const f32x4*)(w1 + kk);
        xv[u][p] = (mok && in) ? xl : z4;
        wv0[u][p] = (n0ok && in) ? l0 : z4;
        wv1[u][p] = (n1ok && in) ? l1 : z4;
      }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bf16x8 xf = ens_bf16x8(xv[u][0], xv[u][1]);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xf, ens_bf16x8(wv0[u][0], wv0[u][1]), acc0, 0, 0, 0);
      if (two) acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xf, ens_bf16x8(wv1[u][0], wv1[u][1]), acc1, 0, 0, 0);
    }
  }
  auto store = [&](const f32x16& acc, int n, bool nok) {
    if (!nok) return;
    const float b = a.bias[n];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int mo = mb + ens_row(r, h);
      if (mo >= a.B) continue;
      const float v = acc[r] + b;
      const size_t o = (size_t)mo * a.yp + n;
      if (a.pre) a.pre[o] = v;
      if (a.act) a.act[o] = ens_act<ACT>(v);
    }
  };
  store(acc0, n0, n0ok);
  store(acc1, n1, n1ok);
}

// ---- backward: the two wave tiles of ens_tile.h ---------------------------------------------------------------------------------------
//   weight tile: dw[n][k] = sum_m bf16(dpre[m][n]) bf16(x[m][k])   (32 n x 64 k per wave, the rows [m_begin, min(m_end, B))).  An
//                m-step of 16 is one MFMA per accumulator; lane half h takes the rows m0 + 2 j + h, j = 0 .. 7 -- the rows, and the
//                order, in which the fp32 tile's lane half meets them, so  db[n] = sum_m dpre[m][n]  from the UNROUNDED values is the
//                fp32 tile's sum bit for bit;
//   input tile : dprev[m][k] = (sum_n bf16(dpre[m][n]) bf16(w[n][k])) * ACT'(pre_prev[m][k])   (32 m x 64 k per wave; N, dp multiples
//                of 4; an n-step of 16: lane half h takes n = 16 t + 8 h .. + 7).
__device__ __forceinline__ void ens_wgrad_tile_bf16(const EnsBwdTile& a, int nb, int kb, int m_begin = 0, int m_end = 0x7fffffff) {
  constexpr int U = 2;
  const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
  const bool two = kb + 32 < a.K;                            // (wave-uniform)
  const int n = nb + i, k0 = kb + i, k1 = kb + 32 + i;
  const bool nok = n < a.N, k0ok = k0 < a.K, k1ok = two && k1 < a.K;
  const float* dcol = a.dpre + (nok ? n : 0);
  const float* xc0 = a.x + (k0ok ? k0 : 0);
  const float* xc1 = a.x + (k1ok ? k1 : 0);
  f32x16 acc0 = {}, acc1 = {};
  float bsum = 0.f;
  const int me = m_end < a.B ? m_end : a.B;
  for (int m0 = m_begin; m0 < me; m0 += 16 * U) {
    float dv[U][8], x0[U][8], x1[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int m = m0 + 16 * u + 2 * j + h;
        const bool mok = m < me;
        const size_t mm = mok ? m : me - 1;                  // (m_begin <= me - 1 inside the loop: a row of the range)
        const float dl = dcol[mm * a.dp], l0 = xc0[mm * a.xp], l1 = xc1[mm * a.xp];
        dv[u][j] = (mok && nok) ? dl : 0.f;
        x0[u][j] = (mok && k0ok) ? l0 : 0.f;
        x1[u][j] = (mok && k1ok) ? l1 : 0.f;
      }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bf16x8 df = ens_bf16x8(dv[u]);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(df, ens_bf16x8(x0[u]), acc0, 0, 0, 0);
      if (two) acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(df, ens_bf16x8(x1[u]), acc1, 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 8; ++j) bsum += dv[u][j];
    }
  }
  if (kb == 0) {
    const float s = bsum + __shfl_xor(bsum, 32, 64);         // (half 0 + half 1 in both halves: one fixed order)
    if (h == 0 && nok) a.db[n] = s;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int no = nb + ens_row(r, h);
    if (no >= a.N) continue;
    float* row = a.dw + (size_t)no * a.K;
    if (k0ok) row[k0] = acc0[r];
    if (k1ok) row[k1] = acc1[r];
  }
}
template <int ACT> __device__ __forceinline__ void ens_dgrad_tile_bf16(const EnsBwdTile& a, int mb, int kb) {
  constexpr int U = 2;
  const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
  const bool two = kb + 32 < a.K;
  const int m = mb + i, k0 = kb + i, k1 = kb + 32 + i;
  const bool mok = m < a.B, k0ok = k0 < a.K, k1ok = two && k1 < a.K;
  const float* dr = a.dpre + (size_t)(mok ? m : 0) * a.dp;
  const float* wc0 = a.w + (k0ok ? k0 : 0);
  const float* wc1 = a.w + (k1ok ? k1 : 0);
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x16 acc0 = {}, acc1 = {};
  for (int nc = 0; nc < a.N; nc += 16 * U) {
    f32x4 dv[U][2];
    float w0[U][8], w1[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int n = nc + 16 * u + 8 * h + 4 * p;           // N and dp are multiples of 4: a float4 of dpre is in or out
        const bool in = n < a.N;
        const int nn = in ? n : 0;                           // (N >= 4: the first four rows of w are always there)
        const f32x4 dl = *(const f32x4*)(dr + nn);
        dv[u][p] = (mok && in) ? dl : z4;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float l0 = wc0[(size_t)(nn + c) * a.K], l1 = wc1[(size_t)(nn + c) * a.K];
          w0[u][4 * p + c] = (in && k0ok) ? l0 : 0.f;
          w1[u][4 * p + c] = (in && k1ok) ? l1 : 0.f;
        }
      }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bf16x8 df = ens_bf16x8(dv[u][0], dv[u][1]);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(df, ens_bf16x8(w0[u]), acc0, 0, 0, 0);
      if (two) acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(df, ens_bf16x8(w1[u]), acc1, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int mo = mb + ens_row(r, h);
    if (mo >= a.B) continue;
    const size_t o = (size_t)mo * a.pp;
    if (k0ok) a.dprev[o + k0] = ens_act_bwd<ACT>(acc0[r], a.pre_prev + o + k0);
    if (k1ok) a.dprev[o + k1] = ens_act_bwd<ACT>(acc1[r], a.pre_prev + o + k1);
  }
}
