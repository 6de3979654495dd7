// The two fused no-grad latent chains of gauss_chain.hip -- the posterior chain (SPEC.md N3h) and the open-loop prior chain (N3i) -- in
// bf16 compute (SPEC.md N3m): s2p_posterior_chain_fwd_bf16, s2p_prior_chain_fwd_bf16; further down the closed-loop imagination chain
// (N3j) in the same mode (N3n): s2p_imagine_chain_fwd_bf16.  Ordinary mixed precision: every tensor the
// caller sees stays fp32; the WEIGHT operand of each layer is a bf16 pack the host made once (round to nearest even), the ACTIVATION
// operand is rounded to bf16 where it is written to LDS (feat(0), z1(t), z2(t-1), h1, h2), the products are summed in fp32 on
// v_mfma_f32_16x16x32_bf16 with k ascending in steps of 32 and K never split, and everything after the sum -- (acc + add) + bias or
// acc + bias, LeakyReLU 0.2, the head of gauss_dev.h -- is the fp32 code of the fp32 chain.  z goes to global memory unrounded.
//
// The design is that of gauss_chain.hip: a workgroup owns 16 batch rows and every output column of every layer, workgroup barriers only,
// grid = ceil(B / 16), 512 threads = 8 waves; the waves split the 16-column tiles of a layer (2 each in a 256-wide layer, PAIRS (mean
// tile p, raw_std tile p + D / 16) in a head layer, so the head is evaluated in registers); cb_step() is shared by both kernels.
// What the eightfold shorter MFMA sequence changes:
//   * Operands.  Lane 16 j + i holds k = 32 c + 8 j .. + 7 of its row: ONE 16-byte read per operand and MFMA.  The weights are the A
//     operand and the activations the B operand, so a lane's four results are four CONSECUTIVE output columns (16 tile + 4 j .. + 3) of
//     batch row i: an epilogue rounds them pairwise and writes them to LDS as one 8-byte store, once.
//   * Weights.  A layer's whole weight operand of a wave is 64 (K 256), 72 (K 288) or, in the 512-wide head, 128 VGPRs, so ask() requests
//     ALL of it, from L2 straight into the MFMA registers, and run() is a bare loop of one LDS read and NT MFMAs per k-step.  A layer is
//     asked for, as in the fp32 file, before the barrier that ends the layer in front of it; layer 2 of an MLP one layer earlier
//     (S2P_CHAIN_BF16_AHEAD, cb_mlp).  Zero scratch: DESIGN.md section 6b.21 has the resource table and the measurements.
//   * LDS (26 368 bytes, static, nothing aliased): xz [16][296], h1, h2 [16][264] bf16.  Row pitches are K + 8 elements = 592 and 528
//     bytes: row i starts 80 i resp. 16 i bytes into the 256-byte bank row, sixteen different 16-byte slots (the reasoning of the fp32
//     file with halved pitches; as there, the 16-lane groups a ds_read_b128 is served in still leave one lane pair per group colliding).
// A row of a tile depends on that row's operands alone, so a row's values do not depend on B or on which rows share its tile; rows >= B
// are zero operands and are never stored.
//
// The closed-loop IMAGINATION chain (SPEC.md N3j) in the same mode (SPEC.md N3n; s2p_imagine_chain_fwd_bf16) puts the deterministic tanh
// policy in front of cb_step(): the policy's three layers multiply in bf16 as every layer here does (weights: a bf16 pack; first layer:
// xz as it stands; hidden activations: rounded where they are written to two [16][W + 8] bf16 tiles, whose heads h1 / h2 of the latent
// half alias -- the halves never overlap in time), a(h) stays fp32 (global memory and a 16 x 8 fp32 LDS tile), and the two action terms
// are the fp32 MFMA chunk of the hoisted GEMM with its operands exchanged, so that a lane's four results are the four additive values of
// CbHidden (CbActionTerm): they never leave the registers and are bitwise the hoisted GEMM's.  A policy layer is up to 64 column tiles,
// so a wave takes its tiles one at a time and streams the weights in k-blocks with the next block in flight (ib_gemm).
// LDS: xz 9 472 + 2 x 33 024 + action tile 512 = 76 032 bytes, static.
#include "gauss_dev.h"

namespace {
constexpr int CB_Z1 = 32, CB_Z2 = 256, CB_Z = CB_Z1 + CB_Z2, CB_HID = 256, CB_FEAT = 256;
#ifndef S2P_CHAIN_BF16_AHEAD
#define S2P_CHAIN_BF16_AHEAD 1                             // 1: an MLP's layer 2 is asked for before its layer 1 runs; 0: after
#endif
constexpr int CB_THREADS = 512, CB_WAVES = CB_THREADS / 64, CB_ROWS = 16;
constexpr int CB_PAD = 8;                                  // bf16 elements added to the LDS row pitch of the activation tiles
constexpr int CB_XZ_P = CB_Z + CB_PAD, CB_H_P = CB_HID + CB_PAD;
constexpr float CB_SLOPE = 0.2f;
constexpr bool CB_AHEAD = S2P_CHAIN_BF16_AHEAD != 0;

struct ChainArgsB {
  const float* feat; const float* ra; const float* rb; const float* eps; float* mean; float* std; float* z;
  int feat_pitch, eps_pitch, mean_pitch, std_pitch, z_pitch, B, T;
  int vec_in, vec_out;                                     // bias / add / eps resp. mean / std / z allow 16-byte accesses (cb_load4, cb_store4f)
  s2p_chain_mlp_bf16 m[4];                                 // z1_posterior_init, z2_prior_init, z1_posterior, z2_prior
};                                                         // (prior chain: feat = z2(0), ra = rc, T = H, m = z1_prior, z2_prior)

// four fp32 values -> four bf16 (round to nearest even, pairwise), one 8-byte LDS store
__device__ __forceinline__ void cb_store4(__bf16* dst, const float (&v)[4]) {
  bf16x4 h;
#pragma unroll
  for (int r = 0; r < 4; ++r) h[r] = (__bf16)v[r];
  *(bf16x4*)dst = h;
}

// Four consecutive fp32 values a lane owns (its four output columns) from / to global memory: ONE 16-byte access where the host found
// the tensors aligned for it (`vec`, uniform for the launch), else four 4-byte ones.  A wave's memory instruction costs about the same
// whichever its width, and a phase of this kernel is bound by their number.
__device__ __forceinline__ void cb_load4(const float* p, bool vec, float (&v)[4]) {
  if (vec) {
    const f32x4 t = *(const f32x4*)p;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = t[r];
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = p[r];
  }
}
__device__ __forceinline__ void cb_store4f(float* p, bool vec, const float (&v)[4]) {
  if (vec) {
    *(f32x4*)p = (f32x4){v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r] = v[r];
  }
}

// The whole weight operand of NT column tiles: wv[q][c] = this lane's weight row of tile q at k = 32 c + 8 j .. + 7.
template <int K, int NT>
__device__ __forceinline__ void cb_load_w(const uint16_t* const (&wr)[NT], bf16x8 (&wv)[NT][K / 32]) {
#pragma unroll
  for (int c = 0; c < K / 32; ++c)
#pragma unroll
    for (int q = 0; q < NT; ++q) wv[q][c] = *(const bf16x8*)(wr[q] + 32 * c);
}

// acc[q] += w[tile q] . x[16 rows][K]^T, k ascending in steps of 32.  xr: this lane's activation row in LDS at k = 8 j.
template <int K, int NT>
__device__ __forceinline__ void cb_gemm(const __bf16* xr, const bf16x8 (&wv)[NT][K / 32], f32x4 (&acc)[NT]) {
  static_assert(K % 32 == 0, "whole k-steps");
#pragma unroll
  for (int c = 0; c < K / 32; ++c) {
    const bf16x8 xv = *(const bf16x8*)(xr + 32 * c);
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv[q][c], xv, acc[q], 0, 0, 0);
  }
}

// The additive term of a CbHidden first layer that the closed-loop chain makes itself (SPEC.md N3n): ONE k-chunk of a(h) [16][pad4(A)]
// x the action columns w[256][w_row], zero-filled past kp = pad4(A), from a zero accumulator, then + 0 -- s2p_linear_fwd without bias.
// `at`: the fp32 LDS tile [16][CB_AT_P] of a(h), columns >= A and rows >= B zeros.  CbHidden::ask evaluates it where it takes its operands.
// `tid`: threadIdx.x as the step's own value (ib_tid), so that the term's addresses are made where they are used.
constexpr int CB_AT_P = 8;
struct CbActionTerm { const float* at; const float* w; int w_row, kp, tid; };

// A hidden layer: ys[16][CB_H_P] = bf16(lrelu(xs[16][K] . w[256][w_row]^T (+ add) + bias)); wave v owns the column tiles v and v + 8.
// ask(): everything that does not depend on the previous layer -- the weights, the bias, the additive term; run() after the barrier.
template <int K, bool ADD>
struct CbHidden {
  static constexpr int NT = CB_HID / 16 / CB_WAVES;
  bf16x8 wv[NT][K / 32];
  float av[NT][4], bv[NT][4];

  __device__ __forceinline__ void ask(const uint16_t* w, int w_row, const float* bias, const float* add, int row0, int B, bool vec) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, j = lane >> 4;
    const uint16_t* wr[NT];
    __builtin_amdgcn_sched_barrier(0);                     // (nor do they rise into the layer in front)
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int t0 = 16 * (wave + q * CB_WAVES);
      wr[q] = w + (size_t)(t0 + i) * w_row + 8 * j;
      cb_load4(bias + t0 + 4 * j, vec, bv[q]);
#pragma unroll
      for (int r = 0; r < 4; ++r) av[q][r] = 0.f;
      if (ADD && row0 + i < B) cb_load4(add + (size_t)(row0 + i) * CB_HID + t0 + 4 * j, vec, av[q]);
    }
    cb_load_w<K, NT>(wr, wv);
    __builtin_amdgcn_sched_barrier(0);                     // (the loads stay here: hipcc would sink them to their first use)
  }

  // The same with the action term of the closed-loop chain as the additive values.  The chunk is lin_mfma_chunk with its operands
  // exchanged -- the same four products per element and MFMA -- so that a lane's four results are the columns 16 tile + 4 j .. + 3 of
  // row i: they are `av` and never leave the registers.
  __device__ __forceinline__ void ask(const uint16_t* w, int w_row, const float* bias, const CbActionTerm& add, int, int, bool vec) {
    static_assert(ADD, "an additive term for a layer without one");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, j = lane >> 4;
    const uint16_t* wr[NT];
    const int ti = add.tid & 15, tj = (add.tid >> 4) & 3, tw = add.tid >> 6;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const bool kok = 4 * tj < add.kp;
    const f32x4 xv = kok ? *(const f32x4*)(add.at + ti * CB_AT_P + 4 * tj) : zero;
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int t0 = 16 * (wave + q * CB_WAVES);
      wr[q] = w + (size_t)(t0 + i) * w_row + 8 * j;
      cb_load4(bias + t0 + 4 * j, vec, bv[q]);
      const f32x4 tv = kok ? *(const f32x4*)(add.w + (size_t)(16 * (tw + q * CB_WAVES) + ti) * add.w_row + 4 * tj) : zero;
      const f32x4 acc = lin_mfma_chunk(tv, xv, zero);
#pragma unroll
      for (int r = 0; r < 4; ++r) av[q][r] = acc[r] + 0.f;
    }
    cb_load_w<K, NT>(wr, wv);
    __builtin_amdgcn_sched_barrier(0);
  }

  // Where a step does NOT ask for the next one (the last step): the operands hold nothing.  Without this the old ones stay live
  // through the whole step on that path -- 80 VGPRs that hipcc then keeps in scratch.
  __device__ __forceinline__ void forget() {
#pragma unroll
    for (int q = 0; q < NT; ++q) {
#pragma unroll
      for (int c = 0; c < K / 32; ++c) wv[q][c] = (bf16x8){};
#pragma unroll
      for (int r = 0; r < 4; ++r) av[q][r] = bv[q][r] = 0.f;
    }
  }

  __device__ __forceinline__ void run(const __bf16* xs, int xp, int row0, int B, __bf16* ys) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, j = lane >> 4;
    f32x4 acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
    cb_gemm<K, NT>(xs + i * xp + 8 * j, wv, acc);
    const bool ok = row0 + i < B;
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float s = acc[q][r];
        if (ADD) s += av[q][r];
        s = act_fwd(s + bv[q][r], S2P_ACT_LRELU, CB_SLOPE);
        v[r] = ok ? s : 0.f;
      }
      cb_store4(ys + i * CB_H_P + 16 * (wave + q * CB_WAVES) + 4 * j, v);
    }
  }
};

// The last layer [mean | raw_std] (2 D wide) and the head, in registers.  A wave owns PAIRS (mean tile p, raw_std tile p + D / 16).
// Writes z(t)[:, off : off + D] unrounded to global memory and rounded to xz; with D == 32 also mean and std.
template <int D>
struct CbHead {
  static constexpr int PAIRS = D / 16, NP = (PAIRS + CB_WAVES - 1) / CB_WAVES, NT = 2 * NP;
  bf16x8 wv[NT][CB_HID / 32];
  float ev[NP][4], bm[NP][4], bs[NP][4];

  static __device__ __forceinline__ bool idle() { return (int)(threadIdx.x >> 6) >= PAIRS; }   // (wave-uniform; the 64-wide head has two pairs)

  __device__ __forceinline__ void ask(const ChainArgsB& a, const uint16_t* w, const float* bias, int t, int off, int row0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, j = lane >> 4;
    if (idle()) return;
    const uint16_t* wr[NT];
    const int gm = row0 + i;
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int t0 = 16 * (wave + p * CB_WAVES);
      wr[2 * p] = w + (size_t)(t0 + i) * CB_HID + 8 * j;
      wr[2 * p + 1] = w + (size_t)(D + t0 + i) * CB_HID + 8 * j;
      const int d0 = t0 + 4 * j;
      cb_load4(bias + d0, a.vec_in, bm[p]);
      cb_load4(bias + D + d0, a.vec_in, bs[p]);
#pragma unroll
      for (int r = 0; r < 4; ++r) ev[p][r] = 0.f;
      if (gm < a.B) cb_load4(a.eps + ((size_t)gm * a.T + t) * a.eps_pitch + off + d0, a.vec_in, ev[p]);
    }
    cb_load_w<CB_HID, NT>(wr, wv);
    __builtin_amdgcn_sched_barrier(0);
  }

  __device__ __forceinline__ void run(const ChainArgsB& a, const __bf16* hs, int t, int off, int row0, __bf16* xz) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, j = lane >> 4;
    if (idle()) return;
    f32x4 acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
    cb_gemm<CB_HID, NT>(hs + i * CB_H_P + 8 * j, wv, acc);
    const int gm = row0 + i;
    const bool ok = gm < a.B;
    const size_t bt = (size_t)gm * a.T + t;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int d0 = 16 * (wave + p * CB_WAVES) + 4 * j;
      float mu[4], sd[4], zv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        mu[r] = acc[2 * p][r] + bm[p][r];
        sd[r] = gauss_head_std(acc[2 * p + 1][r] + bs[p][r]);
        zv[r] = gauss_head_sample(ev[p][r], sd[r], mu[r]);
      }
      if (ok) {
        if (D == CB_Z1) { cb_store4f(a.mean + bt * a.mean_pitch + d0, a.vec_out, mu); cb_store4f(a.std + bt * a.std_pitch + d0, a.vec_out, sd); }
        cb_store4f(a.z + bt * a.z_pitch + off + d0, a.vec_out, zv);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) zv[r] = 0.f;
      }
      cb_store4(xz + i * CB_XZ_P + off + d0, zv);
    }
  }
};

// Layers 2 and 3 of a Gaussian MLP whose first layer `l1` has been asked for: input xs, output z(t)[:, off : off + D].  After the head it
// asks for the first layer of the NEXT MLP through `next()`, before that MLP's first barrier.  CB_AHEAD: layer 2, which depends on
// nothing, is asked for before layer 1 runs instead of after it (136 VGPRs of weights live).  The same for the head or for next() would
// put 192 to 216 VGPRs of weights beside the epilogue's operands: hipcc then spills (112 to 316 bytes of scratch per lane).
template <int D, typename L1, typename Next>
__device__ __forceinline__ void cb_mlp(const ChainArgsB& a, const s2p_chain_mlp_bf16& m, L1& l1, const __bf16* xs, int t, int off, int row0,
                                       __bf16* xz, __bf16* h1, __bf16* h2, Next next) {
  CbHidden<CB_HID, false> l2;
  CbHead<D> l3;
  __syncthreads();
  if (CB_AHEAD) l2.ask(m.w2, CB_HID, m.b2, nullptr, row0, a.B, a.vec_in);
  l1.run(xs, CB_XZ_P, row0, a.B, h1);
  if (!CB_AHEAD) l2.ask(m.w2, CB_HID, m.b2, nullptr, row0, a.B, a.vec_in);
  __syncthreads();
  l2.run(h1, CB_H_P, row0, a.B, h2);
  l3.ask(a, m.w3, m.b3, t, off, row0);
  __syncthreads();
  l3.run(a, h2, t, off, row0, xz);
  next();
}

// One chain step, shared by the posterior chain (t >= 1) and the prior chain (every step): the z1 MLP `ma` on xz[:, 32:288] =
// z2(t-1) with its first layer `a1` already asked for, then the z2 MLP `mb` on xz = z1(t) | z2(t-1) with the additive term `add_b`.
// (a pointer to the hoisted term [B][256] of this step, or a CbActionTerm).  Results go to slot t of eps / mean / std / z.  `next()` asks
// for whatever follows the step.
template <typename AddB, typename Next>
__device__ __forceinline__ void cb_step(const ChainArgsB& a, const s2p_chain_mlp_bf16& ma, const s2p_chain_mlp_bf16& mb,
                                        CbHidden<CB_Z2, true>& a1, CbHidden<CB_Z, true>& b1, const AddB add_b, int t, int row0, __bf16* xz,
                                        __bf16* h1, __bf16* h2, Next next) {
  cb_mlp<CB_Z1>(a, ma, a1, xz + CB_Z1, t, 0, row0, xz, h1, h2, [&] { b1.ask(mb.w1, mb.w1_row, mb.b1, add_b, row0, a.B, a.vec_in); });
  cb_mlp<CB_Z2>(a, mb, b1, xz, t, CB_Z1, row0, xz, h1, h2, next);
}

// src[16 rows][W] fp32 -> xz[:, C0 : C0 + W] rounded; rows >= B are zeros, and so is every activation row derived from them
template <int C0, int W>
__device__ __forceinline__ void cb_load_rows(const float* src, int pitch, int row0, int B, __bf16* xz) {
  for (int idx = threadIdx.x; idx < CB_ROWS * (W / 4); idx += CB_THREADS) {
    const int row = idx / (W / 4), c4 = idx % (W / 4), gm = row0 + row;
    const f32x4 v = gm < B ? *(const f32x4*)(src + (size_t)gm * pitch + 4 * c4) : (f32x4){0.f, 0.f, 0.f, 0.f};
    const float f[4] = {v[0], v[1], v[2], v[3]};
    cb_store4(xz + row * CB_XZ_P + C0 + 4 * c4, f);
  }
}

__global__ __launch_bounds__(CB_THREADS) void posterior_chain_bf16_kernel(const ChainArgsB a) {
  __shared__ __attribute__((aligned(16))) __bf16 xz[CB_ROWS * CB_XZ_P], h1[CB_ROWS * CB_H_P], h2[CB_ROWS * CB_H_P];
  const int row0 = blockIdx.x * CB_ROWS;
  CbHidden<CB_FEAT, false> i1;
  CbHidden<CB_Z1, false> j1;
  CbHidden<CB_Z2, true> a1;
  CbHidden<CB_Z, true> b1;
  i1.ask(a.m[0].w1, a.m[0].w1_row, a.m[0].b1, nullptr, row0, a.B, a.vec_in);
  cb_load_rows<CB_Z1, CB_FEAT>(a.feat, a.feat_pitch, row0, a.B, xz);        // feat(0) -> xz[:, 32:]
  auto ask_a1 = [&](int t) {
    if (t < a.T) a1.ask(a.m[2].w1, a.m[2].w1_row, a.m[2].b1, a.ra + (size_t)(t - 1) * a.B * CB_HID, row0, a.B, a.vec_in);
    else a1.forget();
  };
  // t = 0: q(z1(0) | feat(0)), q(z2(0) | z1(0))
  cb_mlp<CB_Z1>(a, a.m[0], i1, xz + CB_Z1, 0, 0, row0, xz, h1, h2, [&] { j1.ask(a.m[1].w1, a.m[1].w1_row, a.m[1].b1, nullptr, row0, a.B, a.vec_in); });
  cb_mlp<CB_Z2>(a, a.m[1], j1, xz, 0, CB_Z1, row0, xz, h1, h2, [&] { ask_a1(1); });
  // q(z1(t) | feat(t), z2(t-1), a(t-1)), q(z2(t) | z1(t), z2(t-1), a(t-1)): the feat / action columns arrive as ra / rb
  for (int t = 1; t < a.T; ++t)
    cb_step(a, a.m[2], a.m[3], a1, b1, a.rb + (size_t)(t - 1) * a.B * CB_HID, t, row0, xz, h1, h2, [&] { ask_a1(t + 1); });
}

// The open-loop prior chain: z2(0) -> xz[:, 32:], then H steps on the model's own samples.  a.feat is z2(0), a.ra / a.rb the action terms
// of the two first layers, a.T the horizon H, a.m[0] / a.m[1] z1_prior / z2_prior; step h writes slot h - 1.
__global__ __launch_bounds__(CB_THREADS) void prior_chain_bf16_kernel(const ChainArgsB a) {
  __shared__ __attribute__((aligned(16))) __bf16 xz[CB_ROWS * CB_XZ_P], h1[CB_ROWS * CB_H_P], h2[CB_ROWS * CB_H_P];
  const int row0 = blockIdx.x * CB_ROWS;
  CbHidden<CB_Z2, true> a1;
  CbHidden<CB_Z, true> b1;
  auto ask_a1 = [&](int s) {
    if (s < a.T) a1.ask(a.m[0].w1, a.m[0].w1_row, a.m[0].b1, a.ra + (size_t)s * a.B * CB_HID, row0, a.B, a.vec_in);
    else a1.forget();
  };
  ask_a1(0);
  cb_load_rows<CB_Z1, CB_Z2>(a.feat, a.feat_pitch, row0, a.B, xz);
  for (int s = 0; s < a.T; ++s)
    cb_step(a, a.m[0], a.m[1], a1, b1, a.rb + (size_t)s * a.B * CB_HID, s, row0, xz, h1, h2, [&] { ask_a1(s + 1); });
}

// ---- the closed-loop imagination chain in bf16 compute (SPEC.md N3n) -----------------------------------------------------------------
constexpr int IB_WMAX = 1024, IB_AP = CB_AT_P;             // widest policy hidden layer; columns of the fp32 LDS action tile (A <= 8)
constexpr int IB_P_MAX = IB_WMAX + CB_PAD;

struct ImagineArgsB {
  ChainArgsB c;                                            // feat / ra / rb unused; m[0] / m[1] = z1_prior / z2_prior; T = H
  const float* z0; const float* wc; const float* wb; float* act;
  int z0_pitch, wc_row, wb_row, act_pitch, A;
  s2p_policy_mlp_bf16 p;
};

// One 16 x 16 tile of w[16 columns][32 nc] . x[16 rows][32 nc]^T: the MFMA over the k-steps 0 .. nc - 1 in ascending order from a zero
// accumulator.  nc is a run-time value (the policy's width): blocks of 8 k-steps, the next block's operands load while this one is
// multiplied (policy_gemm of the fp32 file).  xr / wr: this lane's LDS activation row and weight row at k = 8 j; wok false (a column
// past N): zero weights.
__device__ __forceinline__ f32x4 ib_gemm(const __bf16* xr, const uint16_t* wr, int nc, bool wok) {
  constexpr int U = 8;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  bf16x8 xa[U], wa[U], xb[U], wb[U];
  auto load = [&](bf16x8 (&xv)[U], bf16x8 (&wv)[U], int c0) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (c0 + u < nc) {
        xv[u] = *(const bf16x8*)(xr + 32 * (c0 + u));
        wv[u] = wok ? *(const bf16x8*)(wr + 32 * (c0 + u)) : (bf16x8){};
      }
  };
  auto mul = [&](const bf16x8 (&xv)[U], const bf16x8 (&wv)[U], int c0) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (c0 + u < nc) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv[u], xv[u], acc, 0, 0, 0);
  };
  load(xa, wa, 0);
  for (int c0 = 0; c0 < nc; c0 += 2 * U) {
    load(xb, wb, c0 + U);
    __builtin_amdgcn_sched_barrier(0);
    mul(xa, wa, c0);
    __builtin_amdgcn_sched_barrier(0);
    load(xa, wa, c0 + 2 * U);
    __builtin_amdgcn_sched_barrier(0);
    mul(xb, wb, c0 + U);
    __builtin_amdgcn_sched_barrier(0);
  }
  return acc;
}

// threadIdx.x as a value of the step it is asked in.  The policy half's per-lane addresses (weight rows, biases, act, the action columns)
// are launch constants; hipcc computes them before the step loop and, at the register ceiling of the latent half, keeps them in scratch
// that every step reloads.  Made from this value they are a few VALU instructions per step instead.
__device__ __forceinline__ int ib_tid() {
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  return tid;
}

// A policy hidden layer: ys[16][yp] = bf16(relu(xs[16][32 nc] . w[W][w_row]^T + bias)); wave v owns the column tiles v, v + 8, ... one at a time
__device__ __forceinline__ void ib_hidden(const __bf16* xs, int xp, int nc, const uint16_t* w, int w_row, const float* bias, int W, int row0,
                                          int B, bool vec, int tid, __bf16* ys, int yp) {
  const int lane = tid & 63, wave = tid >> 6, i = lane & 15, j = lane >> 4;
  const bool ok = row0 + i < B;
  for (int t = wave; t < W / 16; t += CB_WAVES) {
    float bv[4], v[4];
    cb_load4(bias + 16 * t + 4 * j, vec, bv);
    const f32x4 acc = ib_gemm(xs + i * xp + 8 * j, w + (size_t)(16 * t + i) * w_row + 8 * j, nc, true);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float s = act_fwd(acc[r] + bv[r], S2P_ACT_RELU, 0.f);
      v[r] = ok ? s : 0.f;
    }
    cb_store4(ys + i * yp + 16 * t + 4 * j, v);
  }
}

// a(h) = tanh(last_fc(hs)): one column tile (A <= 8 of its 16 columns), wave 0; a lane holds the columns 4 j .. + 3 of row i.  -> act
// slot h, unrounded, and the fp32 LDS tile at[16][IB_AP], whose columns >= A and rows >= B are zeros.
__device__ __forceinline__ void ib_last(const ImagineArgsB& g, const __bf16* hs, int hp, int h, int row0, int tid, float* at) {
  const int lane = tid & 63, wave = tid >> 6, i = lane & 15, j = lane >> 4;
  if (wave != 0) return;
  const bool nok = i < g.A;
  const int W = g.p.width, gm = row0 + i;
  const f32x4 acc = ib_gemm(hs + i * hp + 8 * j, g.p.w3 + (size_t)(nok ? i : 0) * W + 8 * j, W / 32, nok);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = 4 * j + r;
    const bool ok = n < g.A && gm < g.c.B;
    const float v = ok ? act_fwd(acc[r] + g.p.b3[n < g.A ? n : 0], S2P_ACT_TANH, 0.f) : 0.f;
    if (n < IB_AP) at[i * IB_AP + n] = v;
    if (ok) g.act[((size_t)gm * g.c.T + h) * g.act_pitch + n] = v;
  }
}

// z(0) -> xz, then H times: a(h) = policy(z(h)), the two action terms, cb_step.  Slot h holds a(h) and z(h+1).
__global__ __launch_bounds__(CB_THREADS) void imagine_chain_bf16_kernel(const ImagineArgsB g) {
  __shared__ __attribute__((aligned(16))) __bf16 xz[CB_ROWS * CB_XZ_P], pa[CB_ROWS * IB_P_MAX], pb[CB_ROWS * IB_P_MAX];
  __shared__ __attribute__((aligned(16))) float at[CB_ROWS * IB_AP];
  const ChainArgsB& a = g.c;
  const int row0 = blockIdx.x * CB_ROWS, W = g.p.width, pp = W + CB_PAD, kp = (g.A + 3) / 4 * 4;
  CbHidden<CB_Z2, true> a1;
  CbHidden<CB_Z, true> b1;
  cb_load_rows<0, CB_Z>(g.z0, g.z0_pitch, row0, a.B, xz);
  for (int s = 0; s < a.T; ++s) {
    const int tid = ib_tid();
    __syncthreads();                                       // xz = z(s); the latent half is done with h1 / h2 (= pa / pb)
    ib_hidden(xz, CB_XZ_P, CB_Z / 32, g.p.w1, g.p.w1_row, g.p.b1, W, row0, a.B, a.vec_in, tid, pa, pp);
    __syncthreads();
    ib_hidden(pa, pp, W / 32, g.p.w2, W, g.p.b2, W, row0, a.B, a.vec_in, tid, pb, pp);
    __syncthreads();
    ib_last(g, pb, pp, s, row0, tid, at);
    __syncthreads();
    a1.ask(a.m[0].w1, a.m[0].w1_row, a.m[0].b1, CbActionTerm{at, g.wc, g.wc_row, kp, tid}, row0, a.B, a.vec_in);
    cb_step(a, a.m[0], a.m[1], a1, b1, CbActionTerm{at, g.wb, g.wb_row, kp, tid}, s, row0, xz, pa, pb, [] {});
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
struct CbHeadSpec { int k1; const char* name; };           // the chain columns of a head's first layer, and the head's name in messages
const CbHeadSpec CB_POSTERIOR_HEADS[4] = {{CB_FEAT, "z1_posterior_init"}, {CB_Z1, "z2_prior_init"}, {CB_Z2, "z1_posterior"}, {CB_Z, "z2_prior"}};
const CbHeadSpec CB_PRIOR_HEADS[2] = {{CB_Z2, "z1_prior"}, {CB_Z, "z2_prior"}};

// Checks `n` s2p_chain_mlp_bf16s against `spec` and copies them into a.m.  0, or S2P_REQUIRE's value with the error text set.
int cb_take_mlps(const char* who, const s2p_chain_mlp_bf16* mlps, const CbHeadSpec* spec, int n, ChainArgsB& a) {
  for (int g = 0; g < n; ++g) {
    const s2p_chain_mlp_bf16& m = mlps[g];
    const char* name = spec[g].name;
    S2P_REQUIRE(m.w1 && m.b1 && m.w2 && m.b2 && m.w3 && m.b3, "%s: %s: null operand", who, name);
    S2P_REQUIRE(m.k1 == spec[g].k1, "%s: %s: the first layer's K is %d, %d is built", who, name, (int)m.k1, spec[g].k1);
    S2P_REQUIRE(m.w1_row >= m.k1 && m.w1_row % 8 == 0, "%s: %s: w1_row must be a multiple of 8 bf16 elements and at least K", who, name);
    S2P_REQUIRE(s2p_al16(m.w1) && s2p_al16(m.w2) && s2p_al16(m.w3), "%s: %s: the weights must be 16-byte aligned", who, name);
    a.vec_in &= s2p_al16(m.b1) && s2p_al16(m.b2) && s2p_al16(m.b3);
    a.m[g] = m;
  }
  return 0;
}

// Checks the [B, T, C] views a chain reads (eps) and writes (mean, std, z) and the [B][256] source rows, and fills them into `a`.
int cb_take_views(const char* who, const char* src_name, const float* src, int src_pitch, const float* eps, int eps_pitch, float* mean,
                  int mean_pitch, float* std, int std_pitch, float* z, int z_pitch, int B, int T, ChainArgsB& a) {
  S2P_REQUIRE(eps && mean && std && z, "%s: null pointer (eps, mean, std and z are required)", who);
  S2P_REQUIRE(eps_pitch >= CB_Z && mean_pitch >= CB_Z1 && std_pitch >= CB_Z1 && z_pitch >= CB_Z,
              "%s: a pitch is below its row (eps 288, mean 32, std 32, z 288)", who);
  S2P_REQUIRE(src_pitch >= 256, "%s: the pitch of %s is below its row of 256", who, src_name);
  S2P_REQUIRE(s2p_al16(src) && src_pitch % 4 == 0, "%s: %s must be 16-byte aligned, its pitch a multiple of 4 floats", who, src_name);
  a.feat = src; a.feat_pitch = src_pitch; a.eps = eps; a.eps_pitch = eps_pitch; a.mean = mean; a.mean_pitch = mean_pitch; a.std = std;
  a.std_pitch = std_pitch; a.z = z; a.z_pitch = z_pitch; a.B = B; a.T = T;
  a.vec_in = s2p_al16(eps) && eps_pitch % 4 == 0;          // (the callers add the hoisted terms, cb_take_mlps the biases)
  a.vec_out = s2p_al16(mean) && s2p_al16(std) && s2p_al16(z) && mean_pitch % 4 == 0 && std_pitch % 4 == 0 && z_pitch % 4 == 0;
  return 0;
}
}  // namespace

extern "C" int s2p_posterior_chain_fwd_bf16(const float* feat, int feat_pitch, const float* ra, const float* rb, const float* eps,
                                            int eps_pitch, const s2p_chain_mlp_bf16* mlps, float* mean, int mean_pitch, float* std,
                                            int std_pitch, float* z, int z_pitch, int B, int T, void* stream) {
  const char* who = "s2p_posterior_chain_fwd_bf16";
  S2P_REQUIRE(B >= 0 && T >= 0, "%s: negative size", who);
  if (B == 0 || T == 0) return 0;
  S2P_REQUIRE(feat && mlps, "%s: null pointer (feat and mlps are required)", who);
  S2P_REQUIRE(T == 1 || (ra && rb), "%s: ra and rb are required when T > 1", who);
  ChainArgsB a{};
  if (int e = cb_take_views(who, "feat", feat, feat_pitch, eps, eps_pitch, mean, mean_pitch, std, std_pitch, z, z_pitch, B, T, a)) return e;
  if (int e = cb_take_mlps(who, mlps, CB_POSTERIOR_HEADS, T > 1 ? 4 : 2, a)) return e;
  a.ra = ra; a.rb = rb; a.vec_in &= s2p_al16(ra) && s2p_al16(rb);
  hipLaunchKernelGGL(posterior_chain_bf16_kernel, dim3(cdiv(B, CB_ROWS)), dim3(CB_THREADS), 0, (hipStream_t)stream, a);
  S2P_CHECK_LAUNCH("posterior_chain_bf16_kernel");
  return 0;
}

extern "C" int s2p_prior_chain_fwd_bf16(const float* z2_0, int z2_0_pitch, const float* rc, const float* rb, const float* eps,
                                        int eps_pitch, const s2p_chain_mlp_bf16* mlps, float* mean, int mean_pitch, float* std,
                                        int std_pitch, float* z, int z_pitch, int B, int H, void* stream) {
  const char* who = "s2p_prior_chain_fwd_bf16";
  S2P_REQUIRE(B >= 0 && H >= 0, "%s: negative size", who);
  if (B == 0 || H == 0) return 0;
  S2P_REQUIRE(z2_0 && rc && rb && mlps, "%s: null pointer (z2_0, rc, rb and mlps are required)", who);
  ChainArgsB a{};
  if (int e = cb_take_views(who, "z2_0", z2_0, z2_0_pitch, eps, eps_pitch, mean, mean_pitch, std, std_pitch, z, z_pitch, B, H, a)) return e;
  if (int e = cb_take_mlps(who, mlps, CB_PRIOR_HEADS, 2, a)) return e;
  a.ra = rc; a.rb = rb; a.vec_in &= s2p_al16(rc) && s2p_al16(rb);
  hipLaunchKernelGGL(prior_chain_bf16_kernel, dim3(cdiv(B, CB_ROWS)), dim3(CB_THREADS), 0, (hipStream_t)stream, a);
  S2P_CHECK_LAUNCH("prior_chain_bf16_kernel");
  return 0;
}

extern "C" int s2p_imagine_chain_fwd_bf16(const float* z0, int z0_pitch, const float* eps, int eps_pitch, const s2p_chain_mlp_bf16* mlps,
                                          const float* wc, int wc_row, const float* wb, int wb_row, int A,
                                          const s2p_policy_mlp_bf16* policy, float* act, int act_pitch, float* mean, int mean_pitch,
                                          float* std, int std_pitch, float* z, int z_pitch, int B, int H, void* stream) {
  const char* who = "s2p_imagine_chain_fwd_bf16";
  S2P_REQUIRE(B >= 0 && H >= 0, "%s: negative size", who);
  if (B == 0 || H == 0) return 0;
  S2P_REQUIRE(z0 && mlps && wc && wb && policy && act, "%s: null pointer (z0, mlps, wc, wb, policy and act are required)", who);
  S2P_REQUIRE(A >= 1 && A <= IB_AP, "%s: action width %d, 1 .. 8 is built", who, A);
  const int kp = (A + 3) / 4 * 4;
  S2P_REQUIRE(z0_pitch >= CB_Z && act_pitch >= A, "%s: a pitch is below its row (z0 288, act A)", who);
  ImagineArgsB g{};
  if (int e = cb_take_views(who, "z0", z0, z0_pitch, eps, eps_pitch, mean, mean_pitch, std, std_pitch, z, z_pitch, B, H, g.c)) return e;
  S2P_REQUIRE(wc_row >= kp && wc_row % 4 == 0 && wb_row >= kp && wb_row % 4 == 0,
              "%s: wc_row and wb_row must be multiples of 4 floats and at least A padded to 4", who);
  S2P_REQUIRE(s2p_al16(wc) && s2p_al16(wb), "%s: wc and wb must be 16-byte aligned", who);
  if (int e = cb_take_mlps(who, mlps, CB_PRIOR_HEADS, 2, g.c)) return e;
  const s2p_policy_mlp_bf16& p = *policy;
  S2P_REQUIRE(p.w1 && p.b1 && p.w2 && p.b2 && p.w3 && p.b3, "%s: policy: null operand", who);
  S2P_REQUIRE(p.width >= 128 && p.width <= IB_WMAX && p.width % 128 == 0,
              "%s: policy: hidden width %d, multiples of 128 from 128 to 1024 are built", who, (int)p.width);
  S2P_REQUIRE(p.w1_row >= CB_Z && p.w1_row % 8 == 0, "%s: policy: w1_row must be a multiple of 8 bf16 elements and at least K", who);
  S2P_REQUIRE(s2p_al16(p.w1) && s2p_al16(p.w2) && s2p_al16(p.w3), "%s: policy: the weights must be 16-byte aligned", who);
  g.c.vec_in &= s2p_al16(p.b1) && s2p_al16(p.b2);
  g.p = p; g.z0 = z0; g.z0_pitch = z0_pitch; g.wc = wc; g.wc_row = wc_row; g.wb = wb; g.wb_row = wb_row; g.A = A; g.act = act;
  g.act_pitch = act_pitch;
  hipLaunchKernelGGL(imagine_chain_bf16_kernel, dim3(cdiv(B, CB_ROWS)), dim3(CB_THREADS), 0, (hipStream_t)stream, g);
  S2P_CHECK_LAUNCH("imagine_chain_bf16_kernel");
  return 0;
}
