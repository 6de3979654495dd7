// The no-grad SLAC posterior chain as ONE launch (SPEC.md N3h; rlkit/torch/slac/network/latent.py:250-281): all T time steps of the
// two 3-layer Gaussian MLPs, fp32.  linear_small.hip's argument for "a layer is a launch" is about COLUMNS (a layer needs every
// output column of the previous one); the batch ROWS of the chain never meet.  So a workgroup owns 16 rows -- one MFMA 16x16x4 row
// tile -- and every output column of every layer, and runs the whole chain with workgroup barriers only: no grid barrier, no
// cooperative launch, no traffic between workgroups.  grid = ceil(B / 16); at B = 256 that is 16 workgroups on 256 CUs, which is
// accepted: the unfused chain is 72 launches whose time is launch latency, not arithmetic.
//
// Bitwise the per-layer path (lin_fwd_kernel with and without its additive term, gauss_head_fwd_kernel): an output element is the
// accumulator after lin_mfma_chunk over the k-chunks in ascending order from 0 (gauss_dev.h, the function lin_fwd_kernel calls), K is
// never split, then (acc + add) + bias or acc + bias, LeakyReLU 0.2, and the head of gauss_dev.h.  A row of an MFMA tile depends on
// that row's operands alone, so which rows share a tile does not matter; rows >= B are zero operands and are never stored.
//
// 512 threads = 8 waves, two per SIMD.  The waves split the 16-column tiles of a layer: 2 tiles each in a 256-wide layer, and in a
// head layer (64 or 512 wide, [mean | raw_std]) a wave takes PAIRS of tiles (mean tile p, raw_std tile p + D/16), so the lane that
// holds mean[row][d] also holds raw_std[row][d] and the head is evaluated in registers: `raw` is never stored anywhere.  A wave
// reads its A operand (the activations) from LDS once per k-chunk and uses it for all of its tiles; the B operand (weights, 1.9 MB
// per time step, L2-resident) goes from global memory straight into the MFMA registers: a layer's first block of weights is asked
// for before the barrier that ends the previous layer, then the next block loads while the current one is multiplied.  One CU's
// fp32 MFMA rate bounds a 16-row step (13.4 MFLOP, ~52 k cycles), so more waves would only divide the same pipe; fewer (4) leave a
// SIMD idle whenever its one wave waits for weights.  Measured: 425 us per chain at 512 threads, 451-459
// at 256, 504 at 1 024 -- where the 128 VGPRs a lane then has no longer hold the double-buffered operands.  At 512 threads the three
// kernels sit AT the register ceiling (hipcc -Rpass-analysis=kernel-resource-usage): 256 VGPRs per lane, occupancy 2, and a few
// spilled registers -- 12 / 20 / 72 bytes of scratch per lane in the posterior / prior / imagination kernel.  Any edit of the device
// code is judged by that table and by the assembly, not by how it reads.
//
// LDS (51 968 bytes of the CU's 160 KiB, static, nothing aliased):
//   xz [16][292]  z1(t) | z2(t-1), the input row of both first layers (at t = 0 columns 32.. hold feat(0))
//   h1 [16][260]  first-layer output        h2 [16][260]  second-layer output
// Row pitches are K + 4 floats: lane 16 j + i reads row i at k = 16 c + 4 j as one 16-byte read; with a 1 024- or 1 152-byte pitch
// all 16 rows start on one bank, with +4 floats row i starts on bank 4 i (mod 64).  (The 16-lane groups a ds_read_b128 is served in
// are not the j groups, so one lane pair per group still collides; +8 removes that and measures the same: the LDS is not the limit.)
//
// The open-loop PRIOR chain (SPEC.md N3i; s2p_prior_chain_fwd) is the same kernel design around the same step: chain_step() is
// the posterior chain's t >= 1 body, and the prior chain runs it H times from z2(0) with z1_prior's weights in place of
// z1_posterior's and the action term rc in place of ra.  It is bitwise its own per-layer path for the same reason.
//
// The closed-loop IMAGINATION chain (SPEC.md N3j; s2p_imagine_chain_fwd) puts a deterministic tanh policy in front of that step: the
// three policy layers read xz = z(h), a(h) goes to global memory and to a 16 x 8 LDS tile, and the action terms of the two first
// layers are one MFMA chunk per column tile whose accumulator IS the additive value of ChainHidden (ChainAddRegs): they never leave
// the registers.  The policy's hidden activations ([16][W + 4], W <= 1 024) are the big LDS tiles; h1 / h2 of the latent half alias
// their heads -- the halves never overlap in time.  LDS: xz 18 688 + 2 x 65 792 + action tile 512 = 150 784 bytes, static.
//
// The posterior chain UNDER GRAD (SPEC.md N3k): s2p_posterior_chain_fwd_save is the posterior kernel with a ChainSaveT<true> at every
// MLP -- h1, h2, raw = acc + bias and the chain's input rows go to global memory as the per-layer path keeps them -- in a kernel of
// its own, so that the three kernels above keep their generated code; s2p_posterior_chain_bwd (further down) is the sequential part
// of the backward, per step two head backwards and six input gradients, on the same 16-rows-per-workgroup design.
//
// WHERE THINGS LIVE.  Here: the fp32 layers (chain_load_w, chain_gemm, ChainHidden, ChainHead, ChainAddRegs, chain_action_term), the
// policy layers' epilogues, the five kernels, the whole backward and the five entry points.  In gauss_chain_common.h, shared with the
// bf16 mode of gauss_chain_bf16.hip: the dimensions and knobs, ChainLane, ChainSaveT, chain_mlp / chain_step / chain_load_rows,
// chain_stream_gemm, and the host side (head tables, operand checks, launch frame).
#include "gauss_chain_common.h"

namespace {
constexpr int ch_u(int nt) { return S2P_CHAIN_INFLIGHT / nt > 0 ? S2P_CHAIN_INFLIGHT / nt : 1; }
constexpr int CH_XZ_P = CH_Z + S2P_CHAIN_PAD, CH_H_P = CH_HID + S2P_CHAIN_PAD;

struct ChainArgs {
  const float* feat; const float* ra; const float* rb; const float* eps; float* mean; float* std; float* z;
  int feat_pitch, eps_pitch, mean_pitch, std_pitch, z_pitch, B, T;
  s2p_chain_mlp m[4];                                      // z1_posterior_init, z2_prior_init, z1_posterior, z2_prior
};                                                         // (prior chain: feat = z2(0), ra = rc, T = H, m = z1_prior, z2_prior)

// The weights of NT column tiles for one block of k-chunks; wr: this lane's weight rows, already at k = 4 j.
template <int K, int NT, int U>
__device__ __forceinline__ void chain_load_w(const float* const (&wr)[NT], int blk, f32x4 (&wv)[NT][U]) {
#pragma unroll
  for (int u = 0; u < U; ++u)
    if ((blk * U + u) * 16 < K) {
#pragma unroll
      for (int q = 0; q < NT; ++q) wv[q][u] = *(const f32x4*)(wr[q] + 16 * (blk * U + u));
    }
}

// acc[q] += x[16 rows][K] . w[tile q]^T: the chunk sequence of lin_fwd_kernel.  xr: this lane's activation row in LDS at k = 4 j.
// w0: the first block of weights, asked for before the barrier this layer waited at.  While a block is multiplied the next one
// loads; the scheduling barriers keep hipcc from sinking those loads to their first use (it does, leaving one load in flight).
template <int K, int NT, int U>
__device__ __forceinline__ void chain_gemm(const float* xr, const float* const (&wr)[NT], f32x4 (&w0)[NT][U], f32x4 (&acc)[NT]) {
  static_assert(K % 16 == 0, "whole k-chunks");
  constexpr int NC = K / 16, NB = (NC + U - 1) / U;
  f32x4 xv[2][U], w1[NT][U];
  auto load_x = [&](int buf, int blk) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (blk * U + u < NC) xv[buf][u] = *(const f32x4*)(xr + 16 * (blk * U + u));
  };
  load_x(0, 0);
#pragma unroll
  for (int blk = 0; blk < NB; ++blk) {
    f32x4 (&cur)[NT][U] = (blk & 1) ? w1 : w0;
    f32x4 (&nxt)[NT][U] = (blk & 1) ? w0 : w1;
    if (blk + 1 < NB) { chain_load_w<K, NT, U>(wr, blk + 1, nxt); load_x((blk + 1) & 1, blk + 1); }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (blk * U + u < NC) {
#pragma unroll
        for (int q = 0; q < NT; ++q) acc[q] = lin_mfma_chunk(xv[blk & 1][u], cur[q][u], acc[q]);
      }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// The additive term of a ChainHidden first layer in registers: v[q][r] is the value for column tile q, accumulator register r, of the
// lane that holds it -- the layout of `acc` in ChainHidden::run.
template <int NT>
struct ChainAddRegs { float v[NT][4]; };

// A hidden layer: ys[16][CH_H_P] = lrelu(xs[16][K] . w[256][w_row]^T (+ add) + bias); wave v owns the column tiles v and v + 8.
// ask(): everything that does not depend on the previous layer -- the first weights, the bias, the additive term -- is asked for
// BEFORE the barrier that ends the previous layer; run() after it.
template <int K, bool ADD>
struct ChainHidden {
  static constexpr int NT = CH_HID / 16 / CH_WAVES, U = ch_u(NT);
  const float* wr[NT];
  f32x4 w0[NT][U];
  float av[NT][4], bv[NT];

  __device__ __forceinline__ void ask(const ChainArgs& a, const float* w, int w_row, const float* bias, const float* add, int row0) {
    const int B = a.B;
    const auto [lane, wave, i, j] = ChainLane(threadIdx.x);
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int n = 16 * (wave + q * CH_WAVES) + i;
      wr[q] = w + (size_t)n * w_row + 4 * j;
      bv[q] = bias[n];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gm = row0 + 4 * j + r;
        av[q][r] = (ADD && gm < B) ? add[(size_t)gm * CH_HID + n] : 0.f;
      }
    }
    chain_load_w<K, NT, U>(wr, 0, w0);
  }

  // the same with the additive values handed over in registers (the closed-loop chain's action term)
  __device__ __forceinline__ void ask(const ChainArgs&, const float* w, int w_row, const float* bias, const ChainAddRegs<NT>& add, int) {
    static_assert(ADD, "an additive term for a layer without one");
    const auto [lane, wave, i, j] = ChainLane(threadIdx.x);
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int n = 16 * (wave + q * CH_WAVES) + i;
      wr[q] = w + (size_t)n * w_row + 4 * j;
      bv[q] = bias[n];
#pragma unroll
      for (int r = 0; r < 4; ++r) av[q][r] = add.v[q][r];
    }
    chain_load_w<K, NT, U>(wr, 0, w0);
  }

  __device__ __forceinline__ void forget() {}              // (the bf16 layer drops its operands here; these are refilled block by block)

  // gy (the SAVE variant): the layer's output of the rows < B also to global memory, [B][256]
  template <bool SAVE = false>
  __device__ __forceinline__ void run(const float* xs, int xp, int row0, int B, float* ys, float* gy = nullptr) {
    const auto [lane, wave, i, j] = ChainLane(threadIdx.x);
    f32x4 acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
    chain_gemm<K, NT, U>(xs + i * xp + 4 * j, wr, w0, acc);
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int n = 16 * (wave + q * CH_WAVES) + i;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * j + r;
        float v = acc[q][r];
        if (ADD) v += av[q][r];
        v = act_fwd(v + bv[q], S2P_ACT_LRELU, CH_SLOPE);
        ys[row * CH_H_P + n] = row0 + row < B ? v : 0.f;
        if constexpr (SAVE) { if (row0 + row < B) gy[(size_t)(row0 + row) * CH_HID + n] = v; }
      }
    }
  }
};

// The last layer [mean | raw_std] (2 D wide) and the head, in registers.  A wave owns PAIRS (mean tile p, raw_std tile p + D / 16).
// Writes z(t)[:, off : off + D] to global memory and to xz; with D == 32 also mean and std.
template <int D>
struct ChainHead {
  static constexpr int PAIRS = D / 16, NP = (PAIRS + CH_WAVES - 1) / CH_WAVES, NT = 2 * NP, U = ch_u(NT);
  const float* wr[NT];
  f32x4 w0[NT][U];
  float ev[NP][4], bm[NP], bs[NP];

  static __device__ __forceinline__ bool idle() { return (int)(threadIdx.x >> 6) >= PAIRS; }   // (wave-uniform; the 64-wide head has two pairs)

  __device__ __forceinline__ void ask(const ChainArgs& a, const float* w, const float* bias, int t, int off, int row0) {
    const auto [lane, wave, i, j] = ChainLane(threadIdx.x);
    if (idle()) return;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int d = 16 * (wave + p * CH_WAVES) + i;
      wr[2 * p] = w + (size_t)d * CH_HID + 4 * j;
      wr[2 * p + 1] = w + (size_t)(D + d) * CH_HID + 4 * j;
      bm[p] = bias[d]; bs[p] = bias[D + d];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gm = row0 + 4 * j + r;
        ev[p][r] = gm < a.B ? a.eps[((size_t)gm * a.T + t) * a.eps_pitch + off + d] : 0.f;
      }
    }
    chain_load_w<CH_HID, NT, U>(wr, 0, w0);
  }

  template <typename Save = ChainNoSave>
  __device__ __forceinline__ void run(const ChainArgs& a, const float* hs, int t, int off, int row0, float* xz, const Save sv = Save()) {
    const auto [lane, wave, i, j] = ChainLane(threadIdx.x);
    if (idle()) return;
    f32x4 acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
    chain_gemm<CH_HID, NT, U>(hs + i * CH_H_P + 4 * j, wr, w0, acc);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int d = 16 * (wave + p * CH_WAVES) + i;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * j + r, gm = row0 + row;
        const bool ok = gm < a.B;
        const float mu = acc[2 * p][r] + bm[p], rs = acc[2 * p + 1][r] + bs[p], sd = gauss_head_std(rs);
        const float zv = gauss_head_sample(ev[p][r], sd, mu);
        xz[row * CH_XZ_P + off + d] = ok ? zv : 0.f;
        if (!ok) continue;
        if constexpr (Save::on) {
          sv.raw[(size_t)gm * (2 * D) + d] = mu; sv.raw[(size_t)gm * (2 * D) + D + d] = rs;
          if (sv.xz) sv.xz[(size_t)gm * CH_Z + off + d] = zv;
        }
        const size_t bt = (size_t)gm * a.T + t;
        if (D == CH_Z1) { a.mean[bt * a.mean_pitch + d] = mu; a.std[bt * a.std_pitch + d] = sd; }
        a.z[bt * a.z_pitch + off + d] = zv;
      }
    }
  }
};

// The fp32 mode of the chains (gauss_chain_common.h): the layers above, [16][K + S2P_CHAIN_PAD] fp32 activation tiles, layer 2 asked for
// after layer 1 has run.
struct ChainF32 {
  using Args = ChainArgs; using Mlp = s2p_chain_mlp; using Elem = float;
  template <int K, bool ADD> using Hidden = ChainHidden<K, ADD>;
  template <int D> using Head = ChainHead<D>;
  static constexpr int XZ_P = CH_XZ_P, H_P = CH_H_P, PAD = S2P_CHAIN_PAD;
  static constexpr bool AHEAD = false;
  static __device__ __forceinline__ void put4(float* dst, const f32x4 v) { *(f32x4*)dst = v; }
};

using ImagineArgs = ImagineArgsT<ChainArgs, s2p_policy_mlp>;
constexpr int IM_P_MAX = IM_WMAX + S2P_CHAIN_PAD;

// The operands of chain_stream_gemm: lin_mfma_chunk on 16 k of fp32, a lane holds 4 of them.
struct ChainOpsF32 {
  using Vec = f32x4; using X = float; using W = float;
  static constexpr int KSTEP = 16;
  static __device__ __forceinline__ f32x4 mma(const f32x4 xv, const f32x4 wv, const f32x4 acc) { return lin_mfma_chunk(xv, wv, acc); }
};

// ---- the policy half of the closed-loop imagination chain (SPEC.md N3j) ---------------------------------------------------------------
// A policy hidden layer: ys[16][yp] = relu(xs[16][16 nc] . w[W][w_row]^T + bias); wave v owns the column tiles v, v + 8, ... one at a time
__device__ __forceinline__ void policy_hidden(const float* xs, int xp, int nc, const float* w, int w_row, const float* bias, int W, int row0,
                                              int B, float* ys, int yp) {
  const auto [lane, wave, i, j] = ChainLane(threadIdx.x);
  for (int t = wave; t < W / 16; t += CH_WAVES) {
    const int n = 16 * t + i;
    const float b = bias[n];
    const f32x4 acc = chain_stream_gemm<ChainOpsF32>(xs + i * xp + 4 * j, w + (size_t)n * w_row + 4 * j, nc, true);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * j + r;
      const float v = act_fwd(acc[r] + b, S2P_ACT_RELU, 0.f);
      ys[row * yp + n] = row0 + row < B ? v : 0.f;
    }
  }
}

// a(h) = tanh(last_fc(hs)): one column tile (A <= 8 of its 16 columns), wave 0.  -> act slot h and the LDS tile at[16][IM_AP], whose
// columns >= A and rows >= B are zeros.
__device__ __forceinline__ void policy_last(const ImagineArgs& g, const float* hs, int hp, int h, int row0, float* at) {
  const auto [lane, wave, i, j] = ChainLane(threadIdx.x);
  if (wave != 0) return;
  const bool nok = i < g.A;
  const int W = g.p.width;
  const float b = nok ? g.p.b3[i] : 0.f;
  const f32x4 acc = chain_stream_gemm<ChainOpsF32>(hs + i * hp + 4 * j, g.p.w3 + (size_t)(nok ? i : 0) * W + 4 * j, W / 16, nok);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 4 * j + r, gm = row0 + row;
    const bool ok = nok && gm < g.c.B;
    const float v = ok ? act_fwd(acc[r] + b, S2P_ACT_TANH, 0.f) : 0.f;
    if (i < IM_AP) at[row * IM_AP + i] = v;
    if (ok) g.act[((size_t)gm * g.c.T + h) * g.act_pitch + i] = v;
  }
}

// The action term of a 256-wide first layer for the column tiles this wave owns there: ONE k-chunk of a(h) [16][pad4(A)] x the
// action columns w[256][w_row], zero-filled past pad4(A), from a zero accumulator, then + 0 (s2p_linear_fwd without bias).
template <int NT>
__device__ __forceinline__ void chain_action_term(const float* at, const float* w, int w_row, int kp, ChainAddRegs<NT>& out) {
  const auto [lane, wave, i, j] = ChainLane(threadIdx.x);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const bool kok = 4 * j < kp;
  const f32x4 xv = kok ? *(const f32x4*)(at + i * IM_AP + 4 * j) : zero;
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int n = 16 * (wave + q * CH_WAVES) + i;
    const f32x4 wv = kok ? *(const f32x4*)(w + (size_t)n * w_row + 4 * j) : zero;
    const f32x4 acc = lin_mfma_chunk(xv, wv, zero);
#pragma unroll
    for (int r = 0; r < 4; ++r) out.v[q][r] = acc[r] + 0.f;
  }
}

__global__ __launch_bounds__(CH_THREADS) void posterior_chain_kernel(const ChainArgs a) {
  __shared__ __attribute__((aligned(16))) float xz[CH_ROWS * CH_XZ_P], h1[CH_ROWS * CH_H_P], h2[CH_ROWS * CH_H_P];
  const int row0 = blockIdx.x * CH_ROWS;
  ChainF32::Hidden<CH_FEAT, false> i1;
  ChainF32::Hidden<CH_Z1, false> j1;
  ChainF32::Hidden<CH_Z2, true> a1;
  ChainF32::Hidden<CH_Z, true> b1;
  i1.ask(a, a.m[0].w1, a.m[0].w1_row, a.m[0].b1, nullptr, row0);
  chain_load_rows<ChainF32, CH_Z1, CH_FEAT>(a.feat, a.feat_pitch, row0, a.B, xz);      // feat(0) -> xz[:, 32:]
  auto ask_a1 = [&](int t) {
    if (t < a.T) a1.ask(a, a.m[2].w1, a.m[2].w1_row, a.m[2].b1, a.ra + (size_t)(t - 1) * a.B * CH_HID, row0);
    else a1.forget();
  };
  // t = 0: q(z1(0) | feat(0)), q(z2(0) | z1(0))
  chain_mlp<ChainF32, CH_Z1>(a, a.m[0], i1, xz + CH_Z1, 0, 0, row0, xz, h1, h2, [&] { j1.ask(a, a.m[1].w1, a.m[1].w1_row, a.m[1].b1, nullptr, row0); });
  chain_mlp<ChainF32, CH_Z2>(a, a.m[1], j1, xz, 0, CH_Z1, row0, xz, h1, h2, [&] { ask_a1(1); });
  // q(z1(t) | feat(t), z2(t-1), a(t-1)), q(z2(t) | z1(t), z2(t-1), a(t-1)): the feat / action columns arrive as ra / rb
  for (int t = 1; t < a.T; ++t)
    chain_step<ChainF32>(a, a.m[2], a.m[3], a1, b1, a.rb + (size_t)(t - 1) * a.B * CH_HID, t, row0, xz, h1, h2, [&] { ask_a1(t + 1); });
}

// The training form of the posterior chain (SPEC.md N3k): the kernel above, every MLP with a ChainSaveT<true> that names where its
// h1, h2, raw and sample go in `s` -- everything _PosteriorFn.backward reads.  Written out a second time and not one body with a SAVE
// flag: a body that a kernel only calls is inlined in another order, both kernels get another instruction stream, and this one then
// measured 0.3 % slower at B 256.
__global__ __launch_bounds__(CH_THREADS) void posterior_chain_save_kernel(const ChainArgs a, const s2p_chain_state s) {
  __shared__ __attribute__((aligned(16))) float xz[CH_ROWS * CH_XZ_P], h1[CH_ROWS * CH_H_P], h2[CH_ROWS * CH_H_P];
  using Sv = ChainSaveT<true>;
  const int row0 = blockIdx.x * CH_ROWS;
  const size_t B = a.B;
  ChainF32::Hidden<CH_FEAT, false> i1;
  ChainF32::Hidden<CH_Z1, false> j1;
  ChainF32::Hidden<CH_Z2, true> a1;
  ChainF32::Hidden<CH_Z, true> b1;
  i1.ask(a, a.m[0].w1, a.m[0].w1_row, a.m[0].b1, nullptr, row0);
  chain_load_rows<ChainF32, CH_Z1, CH_FEAT>(a.feat, a.feat_pitch, row0, a.B, xz);
  auto ask_a1 = [&](int t) {
    if (t < a.T) a1.ask(a, a.m[2].w1, a.m[2].w1_row, a.m[2].b1, a.ra + (size_t)(t - 1) * a.B * CH_HID, row0);
  };
  chain_mlp<ChainF32, CH_Z1>(a, a.m[0], i1, xz + CH_Z1, 0, 0, row0, xz, h1, h2, [&] { j1.ask(a, a.m[1].w1, a.m[1].w1_row, a.m[1].b1, nullptr, row0); },
                      Sv(s.a0_h1, s.a0_h2, s.a0_raw, nullptr));
  chain_mlp<ChainF32, CH_Z2>(a, a.m[1], j1, xz, 0, CH_Z1, row0, xz, h1, h2, [&] { ask_a1(1); },
                      Sv(s.b0_h1, s.b0_h2, s.b0_raw, a.T > 1 ? s.xz : nullptr));       // z2(0) -> xz[0][:, 32:]
  for (int t = 1; t < a.T; ++t) {
    const size_t r = (size_t)(t - 1) * B;                  // the first row of slot t - 1 in the time-major state
    chain_step<ChainF32>(a, a.m[2], a.m[3], a1, b1, a.rb + (size_t)(t - 1) * a.B * CH_HID, t, row0, xz, h1, h2, [&] { ask_a1(t + 1); },
                  Sv(s.h1a + r * CH_HID, s.h2a + r * CH_HID, s.rawa + r * 2 * CH_Z1, s.xz + r * CH_Z),      // z1(t) -> xz[t-1][:, :32]
                  Sv(s.h1b + r * CH_HID, s.h2b + r * CH_HID, s.rawb + r * 2 * CH_Z2, t + 1 < a.T ? s.xz + (r + B) * CH_Z : nullptr));
  }
}

__global__ __launch_bounds__(CH_THREADS) void prior_chain_kernel(const ChainArgs a) {
  __shared__ __attribute__((aligned(16))) float xz[CH_ROWS * CH_XZ_P], h1[CH_ROWS * CH_H_P], h2[CH_ROWS * CH_H_P];
  const int row0 = blockIdx.x * CH_ROWS;
  ChainF32::Hidden<CH_Z2, true> a1;
  ChainF32::Hidden<CH_Z, true> b1;
  auto ask_a1 = [&](int s) {
    if (s < a.T) a1.ask(a, a.m[0].w1, a.m[0].w1_row, a.m[0].b1, a.ra + (size_t)s * a.B * CH_HID, row0);
    else a1.forget();
  };
  ask_a1(0);
  chain_load_rows<ChainF32, CH_Z1, CH_Z2>(a.feat, a.feat_pitch, row0, a.B, xz);
  for (int s = 0; s < a.T; ++s)
    chain_step<ChainF32>(a, a.m[0], a.m[1], a1, b1, a.rb + (size_t)s * a.B * CH_HID, s, row0, xz, h1, h2, [&] { ask_a1(s + 1); });
}

__global__ __launch_bounds__(CH_THREADS) void imagine_chain_kernel(const ImagineArgs g) {
  __shared__ __attribute__((aligned(16))) float xz[CH_ROWS * CH_XZ_P], pa[CH_ROWS * IM_P_MAX], pb[CH_ROWS * IM_P_MAX], at[CH_ROWS * IM_AP];
  const ChainArgs& a = g.c;
  const int row0 = blockIdx.x * CH_ROWS, W = g.p.width, pp = W + ChainF32::PAD, kp = (g.A + 3) / 4 * 4;
  ChainF32::Hidden<CH_Z2, true> a1;
  ChainF32::Hidden<CH_Z, true> b1;
  chain_load_rows<ChainF32, 0, CH_Z>(g.z0, g.z0_pitch, row0, a.B, xz);
  for (int s = 0; s < a.T; ++s) {
    __syncthreads();                                       // xz = z(s); the latent half is done with h1 / h2 (= pa / pb)
    policy_hidden(xz, CH_XZ_P, CH_Z / 16, g.p.w1, g.p.w1_row, g.p.b1, W, row0, a.B, pa, pp);
    __syncthreads();
    policy_hidden(pa, pp, W / 16, g.p.w2, W, g.p.b2, W, row0, a.B, pb, pp);
    __syncthreads();
    policy_last(g, pb, pp, s, row0, at);
    __syncthreads();
    ChainAddRegs<ChainHidden<CH_Z2, true>::NT> ta;
    ChainAddRegs<ChainHidden<CH_Z, true>::NT> tb;
    chain_action_term(at, g.wc, g.wc_row, kp, ta);
    chain_action_term(at, g.wb, g.wb_row, kp, tb);
    a1.ask(a, a.m[0].w1, a.m[0].w1_row, a.m[0].b1, ta, row0);
    chain_step<ChainF32>(a, a.m[0], a.m[1], a1, b1, tb, s, row0, xz, pa, pb, [] {});
  }
}
// ---- the backward of the posterior chain's steps (SPEC.md N3k) -----------------------------------------------------------------------
// The loop "for t = S .. 1" of _PosteriorFn.backward as ONE launch: per step the two head backwards and the six input gradients
// that ARE sequential (every weight gradient is a batched launch after the chain and reads what this kernel leaves in global
// memory).  The forward's argument holds: rows never meet, so a workgroup owns 16 rows and every column, workgroup barriers only.
// Bitwise the per-layer path: a dgrad element is lin_fwd_kernel's through lin_dgrad_args -- lin_mfma_chunk over the k-chunks of the
// reduction (512, 256 or 64) in ascending order from 0, operand dy * act_grad_from_out(y) (ONE multiply, done here by the lane that
// stores dy into the LDS tile), epilogue acc + 0 or (acc + dx_old) + 0 -- and a head element is gauss_head_grad (gauss_dev.h).
// Weights: the transposed packs, from L2 straight into the MFMA registers (chain_gemm).  LDS, static, nothing aliased, 84 992 bytes:
//   dr [16][516] draw of the head in flight      ta, tb [16][260] dh2 . act', dh1 . act'      dx [16][292] the gradient at xz
struct ChainBwdArgs {
  const float* eps; const float* dmean; const float* dstd; const float* dz;
  int eps_pitch, dmean_pitch, dstd_pitch, dz_pitch, B, T;
  s2p_chain_mlp_bwd m[2];                                  // z1_posterior, z2_prior
  s2p_chain_state s;
  s2p_chain_grads g;
};
constexpr int CH_DR_P = 2 * CH_Z2 + S2P_CHAIN_PAD;

// One input gradient: o[16][NO] = xs[16][K] . w[NO][w_row]^T, xs = dy . act'(y) already.  Wave v owns the column tiles v, v + 8, ...
// -> global `go` (pitch gp) as it is, and the LDS tile `os` (pitch op): as it is, or with PRE times act'(ya) for the dgrad below
// (ya [B][256]: the saved OUTPUT of the layer this gradient arrives at).  ACC: (acc + os) + 0, the accumulating dgrad.
// ask(): the first weights and ya, before the barrier that ends the previous stage; run() after it.
template <int K, int NO, bool ACC, bool PRE>
struct ChainDgrad {
  static constexpr int TILES = NO / 16, NT = (TILES + CH_WAVES - 1) / CH_WAVES, U = ch_u(NT);
  const float* wr[NT];
  f32x4 w0[NT][U];
  float yv[NT][4];

  static __device__ __forceinline__ bool has(int q) { return (int)(threadIdx.x >> 6) + q * CH_WAVES < TILES; }   // (wave-uniform)

  __device__ __forceinline__ void ask(const float* w, int w_row, const float* ya, int row0, int B) {
    const auto [lane, wave, i, j] = ChainLane(threadIdx.x);
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int n = 16 * (has(q) ? wave + q * CH_WAVES : wave) + i;            // (a wave without tile q multiplies tile 0 again, unused)
      wr[q] = w + (size_t)n * w_row + 4 * j;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gm = row0 + 4 * j + r;
        yv[q][r] = (PRE && gm < B) ? ya[(size_t)gm * CH_HID + n] : 0.f;
      }
    }
    chain_load_w<K, NT, U>(wr, 0, w0);
  }

  __device__ __forceinline__ void run(const float* xs, int xp, int row0, int B, float* go, int gp, float* os, int op) {
    const auto [lane, wave, i, j] = ChainLane(threadIdx.x);
    f32x4 acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
    chain_gemm<K, NT, U>(xs + i * xp + 4 * j, wr, w0, acc);
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      if (!has(q)) continue;
      const int n = 16 * (wave + q * CH_WAVES) + i;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * j + r, gm = row0 + row;
        float v = acc[q][r];
        if (ACC) v += os[row * op + n];
        v = v + 0.f;                                       // (lin_fwd_kernel's "+ bias" without one: -0 becomes +0)
        if (gm < B) go[(size_t)gm * gp + n] = v;
        if (PRE) v *= act_grad_from_out(yv[q][r], S2P_ACT_LRELU, CH_SLOPE);
        os[row * op + n] = gm < B ? v : 0.f;
      }
    }
  }
};

// The head backward of D columns at step t: -> draw [B][2 D] of slot t - 1 in global memory and dr[:, : 2 D].  WIDE (the z2 head):
// no dmean / dstd, and the carried gradient dx[:, 32:] only when `carry`; else (z1): dmean, dstd and dx[:, :32], just written.
template <int D, bool WIDE>
__device__ __forceinline__ void chain_head_bwd(const ChainBwdArgs& a, const float* raw, float* draw, int t, bool carry, int row0,
                                               const float* dx, float* dr) {
  constexpr int off = WIDE ? CH_Z1 : 0;
  for (int e = threadIdx.x; e < CH_ROWS * D; e += CH_THREADS) {
    const int row = e / D, d = e % D, gm = row0 + row;
    GaussHeadGrad g = {0.f, 0.f};
    if (gm < a.B) {
      const size_t bt = (size_t)gm * a.T + t;
      const float dzv = a.dz[bt * a.dz_pitch + off + d], ev = a.eps[bt * a.eps_pitch + off + d], dz2 = dx[row * CH_XZ_P + off + d];
      const float rs = raw[(size_t)gm * (2 * D) + D + d];
      if (WIDE) g = gauss_head_grad(true, dzv, carry, dz2, false, 0.f, false, 0.f, true, ev, rs);
      else g = gauss_head_grad(true, dzv, true, dz2, true, a.dmean[bt * a.dmean_pitch + d], true, a.dstd[bt * a.dstd_pitch + d], true, ev, rs);
      draw[(size_t)gm * (2 * D) + d] = g.dmu;
      draw[(size_t)gm * (2 * D) + D + d] = g.draw_std;
    }
    dr[row * CH_DR_P + d] = g.dmu;
    dr[row * CH_DR_P + D + d] = g.draw_std;
  }
}

__global__ __launch_bounds__(CH_THREADS) void posterior_chain_bwd_kernel(const ChainBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float dr[CH_ROWS * CH_DR_P], ta[CH_ROWS * CH_H_P], tb[CH_ROWS * CH_H_P], dx[CH_ROWS * CH_XZ_P];
  const int row0 = blockIdx.x * CH_ROWS, B = a.B, S = a.T - 1;
  const s2p_chain_mlp_bwd& ma = a.m[0];
  const s2p_chain_mlp_bwd& mb = a.m[1];
  for (int e = threadIdx.x; e < CH_ROWS * CH_XZ_P; e += CH_THREADS) dx[e] = 0.f;   // (read at t = S only as an operand that is not added)
  __syncthreads();
  for (int t = S; t >= 1; --t) {
    const size_t r = (size_t)(t - 1) * B;                  // the first row of slot t - 1
    // the z2 MLP: head, 512 -> 256, 256 -> 256, 256 -> 288
    ChainDgrad<2 * CH_Z2, CH_HID, false, true> b3;
    ChainDgrad<CH_HID, CH_HID, false, true> b2;
    ChainDgrad<CH_HID, CH_Z, false, false> b1;
    chain_head_bwd<CH_Z2, true>(a, a.s.rawb + r * 2 * CH_Z2, a.g.drawb + r * 2 * CH_Z2, t, t < S, row0, dx, dr);
    b3.ask(mb.w3t, 2 * CH_Z2, a.s.h2b + r * CH_HID, row0, B);
    __syncthreads();
    b3.run(dr, CH_DR_P, row0, B, a.g.dh2b + r * CH_HID, CH_HID, ta, CH_H_P);
    b2.ask(mb.w2t, CH_HID, a.s.h1b + r * CH_HID, row0, B);
    __syncthreads();
    b2.run(ta, CH_H_P, row0, B, a.g.dh1b + r * CH_HID, CH_HID, tb, CH_H_P);
    b1.ask(mb.w1t, mb.w1t_row, nullptr, row0, B);
    __syncthreads();
    b1.run(tb, CH_H_P, row0, B, a.g.dxz + r * CH_Z, CH_Z, dx, CH_XZ_P);
    __syncthreads();
    // the z1 MLP: head, 64 -> 256, 256 -> 256, 256 -> 256 added to dxz[:, 32:], the gradient at z2(t-1) that step t - 1 takes up
    ChainDgrad<2 * CH_Z1, CH_HID, false, true> a3;
    ChainDgrad<CH_HID, CH_HID, false, true> a2;
    ChainDgrad<CH_HID, CH_Z2, true, false> a1;
    chain_head_bwd<CH_Z1, false>(a, a.s.rawa + r * 2 * CH_Z1, a.g.drawa + r * 2 * CH_Z1, t, true, row0, dx, dr);
    a3.ask(ma.w3t, 2 * CH_Z1, a.s.h2a + r * CH_HID, row0, B);
    __syncthreads();
    a3.run(dr, CH_DR_P, row0, B, a.g.dh2a + r * CH_HID, CH_HID, ta, CH_H_P);
    a2.ask(ma.w2t, CH_HID, a.s.h1a + r * CH_HID, row0, B);
    __syncthreads();
    a2.run(ta, CH_H_P, row0, B, a.g.dh1a + r * CH_HID, CH_HID, tb, CH_H_P);
    a1.ask(ma.w1t, ma.w1t_row, nullptr, row0, B);
    __syncthreads();
    a1.run(tb, CH_H_P, row0, B, a.g.dxz + r * CH_Z + CH_Z1, CH_Z, dx + CH_Z1, CH_XZ_P);
    __syncthreads();
  }
}
}  // namespace
// ---- host side: the operand checks and the launch frame are gauss_chain_common.h's ----------------------------------------------------

extern "C" int s2p_posterior_chain_fwd_save(const float* feat, int feat_pitch, const float* ra, const float* rb, const float* eps,
                                            int eps_pitch, const s2p_chain_mlp* mlps, float* mean, int mean_pitch, float* std,
                                            int std_pitch, float* z, int z_pitch, const s2p_chain_state* state, int B, int T,
                                            void* stream) {
  const char* who = "s2p_posterior_chain_fwd_save";
  if (int e = chain_sizes(who, B, T); e <= 0) return e;
  ChainArgs a{};
  if (int e = posterior_chain_take(who, feat, feat_pitch, ra, rb, eps, eps_pitch, mlps, mean, mean_pitch, std, std_pitch, z, z_pitch, B, T, a))
    return e;
  if (int e = chain_check_state(who, state, T)) return e;
  return chain_launch("posterior_chain_save_kernel", posterior_chain_save_kernel, B, stream, a, *state);
}

extern "C" int s2p_posterior_chain_bwd(const float* eps, int eps_pitch, const float* dmean, int dmean_pitch, const float* dstd,
                                       int dstd_pitch, const float* dz, int dz_pitch, const s2p_chain_mlp_bwd* mlps,
                                       const s2p_chain_state* state, const s2p_chain_grads* grads, int B, int T, void* stream) {
  const char* who = "s2p_posterior_chain_bwd";
  if (int e = chain_sizes(who, B, T, 2); e <= 0) return e;    // (T == 1: the chain has no step)
  ChainBwdArgs a{};
  if (int e = posterior_bwd_take(who, eps, eps_pitch, dmean, dmean_pitch, dstd, dstd_pitch, dz, dz_pitch, mlps, state, grads, B, T, a))
    return e;
  return chain_launch("posterior_chain_bwd_kernel", posterior_chain_bwd_kernel, B, stream, a);
}

extern "C" int s2p_posterior_chain_fwd(const float* feat, int feat_pitch, const float* ra, const float* rb, const float* eps,
                                       int eps_pitch, const s2p_chain_mlp* mlps, float* mean, int mean_pitch, float* std,
                                       int std_pitch, float* z, int z_pitch, int B, int T, void* stream) {
  const char* who = "s2p_posterior_chain_fwd";
  if (int e = chain_sizes(who, B, T); e <= 0) return e;
  ChainArgs a{};
  if (int e = posterior_chain_take(who, feat, feat_pitch, ra, rb, eps, eps_pitch, mlps, mean, mean_pitch, std, std_pitch, z, z_pitch, B, T, a))
    return e;
  return chain_launch("posterior_chain_kernel", posterior_chain_kernel, B, stream, a);
}

extern "C" int s2p_prior_chain_fwd(const float* z2_0, int z2_0_pitch, const float* rc, const float* rb, const float* eps, int eps_pitch,
                                   const s2p_chain_mlp* mlps, float* mean, int mean_pitch, float* std, int std_pitch, float* z,
                                   int z_pitch, int B, int H, void* stream) {
  const char* who = "s2p_prior_chain_fwd";
  if (int e = chain_sizes(who, B, H); e <= 0) return e;
  ChainArgs a{};
  if (int e = prior_chain_take(who, z2_0, z2_0_pitch, rc, rb, eps, eps_pitch, mlps, mean, mean_pitch, std, std_pitch, z, z_pitch, B, H, a))
    return e;
  return chain_launch("prior_chain_kernel", prior_chain_kernel, B, stream, a);
}

extern "C" int s2p_imagine_chain_fwd(const float* z0, int z0_pitch, const float* eps, int eps_pitch, const s2p_chain_mlp* mlps,
                                     const float* wc, int wc_row, const float* wb, int wb_row, int A, const s2p_policy_mlp* policy,
                                     float* act, int act_pitch, float* mean, int mean_pitch, float* std, int std_pitch, float* z,
                                     int z_pitch, int B, int H, void* stream) {
  const char* who = "s2p_imagine_chain_fwd";
  if (int e = chain_sizes(who, B, H); e <= 0) return e;
  ImagineArgs g{};
  if (int e = imagine_chain_take(who, z0, z0_pitch, eps, eps_pitch, mlps, wc, wc_row, wb, wb_row, A, policy, act, act_pitch, mean, mean_pitch,
                                 std, std_pitch, z, z_pitch, B, H, g))
    return e;
  return chain_launch("imagine_chain_kernel", imagine_chain_kernel, B, stream, g);
}
