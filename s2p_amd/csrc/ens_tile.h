// The wave tiles of the grouped fp32 linear layers, shared by the ensemble entry points (ensemble_train.hip: group = ensemble member,
// Swish) and the grouped MLP entry points (mlp.hip: group = network, ReLU or identity, a row count and an input width per group).  A tile
// function is handed ONE group's view -- base pointers already offset to the group's slot and column -- and the tile's origin;
// the caller's kernel only maps its grid onto groups and tiles.  All fp32 on v_mfma_f32_32x32x2_f32 (lane l holds
// A[row l & 31][k = l >> 5] and B[k = l >> 5][col l & 31]; result register r of lane l is
// D[row (r & 3) + 8 (r >> 2) + 4 (l >> 5)][col l & 31]), operands straight from global memory into the MFMA registers (no LDS), no
// atomics, a fixed summation order.
#pragma once
#include "s2p_common.h"

enum { ENS_ACT_SWISH = 0, ENS_ACT_RELU = 1, ENS_ACT_NONE = 2 };

__device__ __forceinline__ float ens_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }
__device__ __forceinline__ int ens_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
template <int ACT> __device__ __forceinline__ float ens_act(float v) {
  if constexpr (ACT == ENS_ACT_SWISH) return v / (1.f + expf(-v));
  else if constexpr (ACT == ENS_ACT_RELU) return v > 0.f ? v : 0.f;
  else return v;
}
// the activation's derivative from a tensor `p` of the producer: Swish needs the PRE-activation (d/dp [p sigmoid(p)] is not a
// function of swish's output); ReLU needs only its sign, so the pre-activation and the activation serve alike
__device__ __forceinline__ float ens_swish_grad(float p) { const float s = ens_sigmoid(p); return s * (1.f + p * (1.f - s)); }
// d * ACT'(*p): identity never looks at p (it may be NULL-based); ReLU selects, so a masked element is +0
template <int ACT> __device__ __forceinline__ float ens_act_bwd(float d, const float* p) {
  if constexpr (ACT == ENS_ACT_SWISH) return d * ens_swish_grad(*p);
  else if constexpr (ACT == ENS_ACT_RELU) return *p > 0.f ? d : 0.f;
  else return d;
}

// ---- forward: pre[m][n] = sum_k x[m][k] w[n][k] + bias[n];  act = ACT(pre) ----------------------------------------------------------
// A wave owns 32 rows x 64 columns (two accumulators share the x operand).  A k-chunk of 8 is one float4 per lane and operand (lane
// half h takes k = 8 t + 4 h .. + 3) consumed by four MFMAs (MFMA c uses component c of both operands: the same k permutation on
// both sides, so the sum is the plain dot product).  K and the pitches are multiples of 4: a float4 is in or out.
struct EnsFwdTile {
  const float* x; const float* w; const float* bias; float* pre; float* act;   // x [B][xp], w [N][K], bias [N], pre / act [B][yp]
  int xp, yp, B, K, N;
};
template <int ACT> __device__ __forceinline__ void ens_fwd_tile(const EnsFwdTile& a, int mb, int nb) {
  constexpr int U = 4;
  const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
  const bool two = nb + 32 < a.N;                            // (wave-uniform)
  const int m = mb + i, n0 = nb + i, n1 = nb + 32 + i;
  const bool mok = m < a.B, n0ok = n0 < a.N, n1ok = two && n1 < a.N;
  const float* xr = a.x + (size_t)(mok ? m : 0) * a.xp;
  const float* w0 = a.w + (size_t)(n0ok ? n0 : 0) * a.K;
  const float* w1 = a.w + (size_t)(n1ok ? n1 : 0) * a.K;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x16 acc0 = {}, acc1 = {};
  for (int kc = 0; kc < a.K; kc += 8 * U) {
    f32x4 xv[U], wv0[U], wv1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = kc + 8 * u + 4 * h;
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

// ---- backward: two kinds of wave tiles ----------------------------------------------------------------------------------------------
//   weight tile: dw[n][k] = sum_m dpre[m][n] x[m][k]   (32 n x 64 k per wave, the rows [m_begin, min(m_end, B)) in row order -- the
//                whole batch for the ensemble and IQL entry points: no row split, so no partial sums and no second pass at any B;
//                a row range for s2p_mlp_linear_bwd_split, whose caller points dw / db at a partial);  db[n] = sum_m dpre  from
//                the same operand values (per lane in row order, then the two lane halves), written by the tiles at k = 0;
//   input tile : dprev[m][k] = (sum_n dpre[m][n] w[n][k]) * ACT'(pre_prev[m][k])   (32 m x 64 k per wave; N, dp multiples of 4).
struct EnsBwdTile {
  const float* x; const float* dpre; const float* w; float* dw; float* db; const float* pre_prev; float* dprev;
  int xp, dp, pp, B, K, N;                                   // x [B][xp], dpre [B][dp], w / dw [N][K], db [N], pre_prev / dprev [B][pp]
};
__device__ __forceinline__ void ens_wgrad_tile(const EnsBwdTile& a, int nb, int kb, int m_begin = 0, int m_end = 0x7fffffff) {
  constexpr int U = 8;
  const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
  const bool two = kb + 32 < a.K;                            // (wave-uniform)
  const int n = nb + i, k0 = kb + i, k1 = kb + 32 + i;
  const bool nok = n < a.N, k0ok = k0 < a.K, k1ok = two && k1 < a.K;
  const float* dcol = a.dpre + (nok ? n : 0);
  const float* xcol = a.x;
  f32x16 acc0 = {}, acc1 = {};
  float bsum = 0.f;
  const int me = m_end < a.B ? m_end : a.B;
  for (int m0 = m_begin; m0 < me; m0 += 2 * U) {
    float dv[U], x0[U], x1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int m = m0 + 2 * u + h;
      const bool mok = m < me;
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
template <int ACT> __device__ __forceinline__ void ens_dgrad_tile(const EnsBwdTile& a, int mb, int kb) {
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
    const size_t o = (size_t)mo * a.pp;
    if (k0ok) a.dprev[o + k0] = ens_act_bwd<ACT>(acc0[r], a.pre_prev + o + k0);
    if (k1ok) a.dprev[o + k1] = ens_act_bwd<ACT>(acc1[r], a.pre_prev + o + k1);
  }
}

// ---- the input gradient of a narrow layer (N <= 16: plain dot products, no tile): element idx = m K + k of dprev, n in order.
//      Shared by the full backward and the input-gradient-only entry point of mlp.hip, which must agree bit for bit.
template <int ACT> __device__ __forceinline__ void ens_dot_dgrad_elem(const EnsBwdTile& t, long long idx) {
  if (idx >= (long long)t.B * t.K) return;
  const int m = (int)(idx / t.K), k = (int)(idx - (long long)m * t.K);
  const float* dr = t.dpre + (size_t)m * t.dp;
  float s = 0.f;
  for (int n = 0; n < t.N; ++n) s += dr[n] * t.w[(size_t)n * t.K + k];
  const size_t o = (size_t)m * t.pp + k;
  t.dprev[o] = ens_act_bwd<ACT>(s, t.pre_prev + o);
}
