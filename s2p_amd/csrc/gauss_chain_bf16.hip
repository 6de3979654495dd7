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
// tile p, raw_std tile p + D / 16) in a head layer, so the head is evaluated in registers); the control skeleton around a layer, the
// dimensions and the host-side checks ARE the fp32 file's: gauss_chain_common.h, which this file gives its layers as the mode ChainBf16.
// What the eightfold shorter MFMA sequence changes:
//   * Operands.  Lane 16 j + i holds k = 32 c + 8 j .. + 7 of its row: ONE 16-byte read per operand and MFMA.  The weights are the A
//     operand and the activations the B operand, so a lane's four results are four CONSECUTIVE output columns (16 tile + 4 j .. + 3) of
//     batch row i: an epilogue rounds them pairwise and writes them to LDS as one 8-byte store, once.
//   * Weights.  A layer's whole weight operand of a wave is 64 (K 256), 72 (K 288) or, in the 512-wide head, 128 VGPRs, so ask() requests
//     ALL of it, from L2 straight into the MFMA registers, and run() is a bare loop of one LDS read and NT MFMAs per k-step.  A layer is
//     asked for, as in the fp32 file, before the barrier that ends the layer in front of it; layer 2 of an MLP one layer earlier
//     (S2P_CHAIN_BF16_AHEAD, chain_mlp).  Zero scratch: DESIGN.md section 6b.21 has the resource table and the measurements.
//   * LDS (26 368 bytes, static, nothing aliased): xz [16][296], h1, h2 [16][264] bf16.  Row pitches are K + 8 elements = 592 and 528
//     bytes: row i starts 80 i resp. 16 i bytes into the 256-byte bank row, sixteen different 16-byte slots (the reasoning of the fp32
//     file with halved pitches; as there, the 16-lane groups a ds_read_b128 is served in still leave one lane pair per group colliding).
// A row of a tile depends on that row's operands alone, so a row's values do not depend on B or on which rows share its tile; rows >= B
// are zero operands and are never stored.
//
// The closed-loop IMAGINATION chain (SPEC.md N3j) in the same mode (SPEC.md N3n; s2p_imagine_chain_fwd_bf16) puts the deterministic tanh
// policy in front of chain_step(): the policy's three layers multiply in bf16 as every layer here does (weights: a bf16 pack; first layer:
// xz as it stands; hidden activations: rounded where they are written to two [16][W + 8] bf16 tiles, whose heads h1 / h2 of the latent
// half alias -- the halves never overlap in time), a(h) stays fp32 (global memory and a 16 x 8 fp32 LDS tile), and the two action terms
// are the fp32 MFMA chunk of the hoisted GEMM with its operands exchanged, so that a lane's four results are the four additive values of
// CbHidden (CbActionTerm): they never leave the registers and are bitwise the hoisted GEMM's.  A policy layer is up to 64 column tiles,
// so a wave takes its tiles one at a time and streams the weights in k-blocks with the next block in flight (chain_stream_gemm).
// LDS: xz 9 472 + 2 x 33 024 + action tile 512 = 76 032 bytes, static.
//
// The posterior chain UNDER GRAD in the same mode (SPEC.md N3p; further down): s2p_posterior_chain_fwd_save_bf16 is the posterior kernel
// with a ChainSaveT<true> at every MLP, in a kernel of its own -- the state gets the fp32 values the epilogues hold before they round;
// s2p_posterior_chain_bwd_bf16 is the sequential part of the backward with its six input gradients per step on the bf16 matrix cores
// (CbDgrad), heads and the carried gradient in fp32; s2p_chain_pack_bf16 makes the rounded packs and their transposes, one launch
// for several matrices.  DESIGN.md section 6b.25 has the LDS map, the resource table and the measurements.
#include "gauss_chain_common.h"

namespace {
constexpr int CB_PAD = 8;                                  // bf16 elements added to the LDS row pitch of the activation tiles
constexpr int CB_XZ_P = CH_Z + CB_PAD, CB_H_P = CH_HID + CB_PAD;

struct ChainArgsB {
  const float* feat; const float* ra; const float* rb; const float* eps; float* mean; float* std; float* z;
  int feat_pitch, eps_pitch, mean_pitch, std_pitch, z_pitch, B, T;
  int vec_in, vec_out;                                     // bias / add / eps resp. mean / std / z allow 16-byte accesses (cb_load4, cb_store4f)
  s2p_chain_mlp_bf16 m[4];                                 // z1_posterior_init, z2_prior_init, z1_posterior, z2_prior
                                                           // (prior chain: feat = z2(0), ra = rc, T = H, m = z1_prior, z2_prior)
  // Host: vec_in / vec_out from the operands in place, `n` of m among them (a null ra / rb counts as aligned: no step reads it).
  void set_vec(int n) {
    vec_in = s2p_al16(eps) && eps_pitch % 4 == 0 && s2p_al16(ra) && s2p_al16(rb);
    for (int g = 0; g < n; ++g) vec_in &= s2p_al16(m[g].b1) && s2p_al16(m[g].b2) && s2p_al16(m[g].b3);
    vec_out = s2p_al16(mean) && s2p_al16(std) && s2p_al16(z) && mean_pitch % 4 == 0 && std_pitch % 4 == 0 && z_pitch % 4 == 0;
  }
};

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
// `at`: the fp32 LDS tile [16][IM_AP] of a(h), columns >= A and rows >= B zeros.  CbHidden::ask evaluates it where it takes its operands.
// `tid`: threadIdx.x as the step's own value (ib_tid), so that the term's addresses are made where they are used.
struct CbActionTerm { const float* at; const float* w; int w_row, kp, tid; };

// A hidden layer: ys[16][CB_H_P] = bf16(lrelu(xs[16][K] . w[256][w_row]^T (+ add) + bias)); wave v owns the column tiles v and v + 8.
// ask(): everything that does not depend on the previous layer -- the weights, the bias, the additive term; run() after the barrier.
template <int K, bool ADD>
struct CbHidden {
  static constexpr int NT = CH_HID / 16 / CH_WAVES;
  bf16x8 wv[NT][K / 32];
  float av[NT][4], bv[NT][4];

  // The form the shared skeleton calls.  It only forwards: B and the `vec` flag are read from `a` HERE, in front of the layer's own
  // code -- read inside it, hipcc schedules all three kernels differently.
  template <typename Add>
  __device__ __forceinline__ void ask(const ChainArgsB& a, const uint16_t* w, int w_row, const float* bias, const Add& add, int row0) {
    ask(w, w_row, bias, add, row0, a.B, a.vec_in);
  }

  __device__ __forceinline__ void ask(const uint16_t* w, int w_row, const float* bias, const float* add, int row0, int B, bool vec) {
    const auto [lane, wave, i, j] = ChainLane(threadIdx.x);
    const uint16_t* wr[NT];
    __builtin_amdgcn_sched_barrier(0);                     // (nor do they rise into the layer in front)
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int t0 = 16 * (wave + q * CH_WAVES);
      wr[q] = w + (size_t)(t0 + i) * w_row + 8 * j;
      cb_load4(bias + t0 + 4 * j, vec, bv[q]);
#pragma unroll
      for (int r = 0; r < 4; ++r) av[q][r] = 0.f;
      if (ADD && row0 + i < B) cb_load4(add + (size_t)(row0 + i) * CH_HID + t0 + 4 * j, vec, av[q]);
    }
    cb_load_w<K, NT>(wr, wv);
    __builtin_amdgcn_sched_barrier(0);                     // (the loads stay here: hipcc would sink them to their first use)
  }

  // The same with the action term of the closed-loop chain as the additive values.  The chunk is lin_mfma_chunk with its operands
  // exchanged -- the same four products per element and MFMA -- so that a lane's four results are the columns 16 tile + 4 j .. + 3 of
  // row i: they are `av` and never leave the registers.
  __device__ __forceinline__ void ask(const uint16_t* w, int w_row, const float* bias, const CbActionTerm& add, int, int, bool vec) {
    static_assert(ADD, "an additive term for a layer without one");
    const auto [lane, wave, i, j] = ChainLane(threadIdx.x);
    const uint16_t* wr[NT];
    const int ti = add.tid & 15, tj = (add.tid >> 4) & 3, tw = add.tid >> 6;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const bool kok = 4 * tj < add.kp;
    const f32x4 xv = kok ? *(const f32x4*)(add.at + ti * IM_AP + 4 * tj) : zero;
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int t0 = 16 * (wave + q * CH_WAVES);
      wr[q] = w + (size_t)(t0 + i) * w_row + 8 * j;
      cb_load4(bias + t0 + 4 * j, vec, bv[q]);
      const f32x4 tv = kok ? *(const f32x4*)(add.w + (size_t)(16 * (tw + q * CH_WAVES) + ti) * add.w_row + 4 * tj) : zero;
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

  // gy (the SAVE variant, SPEC.md N3p): the layer's UNROUNDED output of the rows < B also to global memory, [B][256], 16-byte aligned
  template <bool SAVE = false>
  __device__ __forceinline__ void run(const __bf16* xs, int xp, int row0, int B, __bf16* ys, float* gy = nullptr) {
    const auto [lane, wave, i, j] = ChainLane(threadIdx.x);
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
        s = act_fwd(s + bv[q][r], S2P_ACT_LRELU, CH_SLOPE);
        v[r] = ok ? s : 0.f;
      }
      if constexpr (SAVE) { if (ok) cb_store4f(gy + (size_t)(row0 + i) * CH_HID + 16 * (wave + q * CH_WAVES) + 4 * j, true, v); }
      cb_store4(ys + i * CB_H_P + 16 * (wave + q * CH_WAVES) + 4 * j, v);
    }
  }
};

// The last layer [mean | raw_std] (2 D wide) and the head, in registers.  A wave owns PAIRS (mean tile p, raw_std tile p + D / 16).
// Writes z(t)[:, off : off + D] unrounded to global memory and rounded to xz; with D == 32 also mean and std.
template <int D>
struct CbHead {
  static constexpr int PAIRS = D / 16, NP = (PAIRS + CH_WAVES - 1) / CH_WAVES, NT = 2 * NP;
  bf16x8 wv[NT][CH_HID / 32];
  float ev[NP][4], bm[NP][4], bs[NP][4];

  static __device__ __forceinline__ bool idle() { return (int)(threadIdx.x >> 6) >= PAIRS; }   // (wave-uniform; the 64-wide head has two pairs)

  __device__ __forceinline__ void ask(const ChainArgsB& a, const uint16_t* w, const float* bias, int t, int off, int row0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, j = lane >> 4;   // (spelled out: from a ChainLane hipcc allocates posterior_chain_bf16_kernel differently)
    if (idle()) return;
    const uint16_t* wr[NT];
    const int gm = row0 + i;
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int t0 = 16 * (wave + p * CH_WAVES);
      wr[2 * p] = w + (size_t)(t0 + i) * CH_HID + 8 * j;
      wr[2 * p + 1] = w + (size_t)(D + t0 + i) * CH_HID + 8 * j;
      const int d0 = t0 + 4 * j;
      cb_load4(bias + d0, a.vec_in, bm[p]);
      cb_load4(bias + D + d0, a.vec_in, bs[p]);
#pragma unroll
      for (int r = 0; r < 4; ++r) ev[p][r] = 0.f;
      if (gm < a.B) cb_load4(a.eps + ((size_t)gm * a.T + t) * a.eps_pitch + off + d0, a.vec_in, ev[p]);
    }
    cb_load_w<CH_HID, NT>(wr, wv);
    __builtin_amdgcn_sched_barrier(0);
  }

  // sv (the SAVE variant, SPEC.md N3p): raw = [acc + bias] of both halves and the sample, unrounded, to the state; 16-byte stores
  template <typename Save = ChainNoSave>
  __device__ __forceinline__ void run(const ChainArgsB& a, const __bf16* hs, int t, int off, int row0, __bf16* xz, const Save sv = Save()) {
    const auto [lane, wave, i, j] = ChainLane(threadIdx.x);
    if (idle()) return;
    f32x4 acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
    cb_gemm<CH_HID, NT>(hs + i * CB_H_P + 8 * j, wv, acc);
    const int gm = row0 + i;
    const bool ok = gm < a.B;
    const size_t bt = (size_t)gm * a.T + t;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int d0 = 16 * (wave + p * CH_WAVES) + 4 * j;
      float mu[4], rs[4], sd[4], zv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        mu[r] = acc[2 * p][r] + bm[p][r];
        rs[r] = acc[2 * p + 1][r] + bs[p][r];
        sd[r] = gauss_head_std(rs[r]);
        zv[r] = gauss_head_sample(ev[p][r], sd[r], mu[r]);
      }
      if constexpr (Save::on) {
        if (ok) {
          cb_store4f(sv.raw + (size_t)gm * (2 * D) + d0, true, mu);
          cb_store4f(sv.raw + (size_t)gm * (2 * D) + D + d0, true, rs);
          if (sv.xz) cb_store4f(sv.xz + (size_t)gm * CH_Z + off + d0, true, zv);
        }
      }
      if (ok) {
        if (D == CH_Z1) { cb_store4f(a.mean + bt * a.mean_pitch + d0, a.vec_out, mu); cb_store4f(a.std + bt * a.std_pitch + d0, a.vec_out, sd); }
        cb_store4f(a.z + bt * a.z_pitch + off + d0, a.vec_out, zv);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) zv[r] = 0.f;
      }
      cb_store4(xz + i * CB_XZ_P + off + d0, zv);
    }
  }
};

// threadIdx.x as a value of the step it is asked in.  The policy half's per-lane addresses (weight rows, biases, act, the action columns)
// are launch constants; hipcc computes them before the step loop and, at the register ceiling of the latent half, keeps them in scratch
// that every step reloads.  Made from this value they are a few VALU instructions per step instead.
__device__ __forceinline__ int ib_tid() {
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  return tid;
}

// The bf16 mode of the chains (gauss_chain_common.h): the layers above, [16][K + 8] bf16 activation tiles, layer 2 asked for before layer
// 1 runs.
struct ChainBf16 {
  using Args = ChainArgsB; using Mlp = s2p_chain_mlp_bf16; using Elem = __bf16;
  template <int K, bool ADD> using Hidden = CbHidden<K, ADD>;
  template <int D> using Head = CbHead<D>;
  static constexpr int XZ_P = CB_XZ_P, H_P = CB_H_P, PAD = CB_PAD;
  static constexpr bool AHEAD = CB_AHEAD;
  static __device__ __forceinline__ void put4(__bf16* dst, const f32x4 v) {
    const float f[4] = {v[0], v[1], v[2], v[3]};
    cb_store4(dst, f);
  }
};

using ImagineArgsB = ImagineArgsT<ChainArgsB, s2p_policy_mlp_bf16>;
constexpr int IB_P_MAX = IM_WMAX + CB_PAD;

// The operands of chain_stream_gemm: one MFMA on 32 k of bf16, a lane holds 8 of them; the weights are the A operand.
struct ChainOpsBf16 {
  using Vec = bf16x8; using X = __bf16; using W = uint16_t;
  static constexpr int KSTEP = 32;
  static __device__ __forceinline__ f32x4 mma(const bf16x8 xv, const bf16x8 wv, const f32x4 acc) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv, xv, acc, 0, 0, 0);
  }
};

// ---- the policy half of the closed-loop imagination chain in bf16 compute (SPEC.md N3n) ----------------------------------------------
// A policy hidden layer: ys[16][yp] = bf16(relu(xs[16][32 nc] . w[W][w_row]^T + bias)); wave v owns the column tiles v, v + 8, ... one at a time
__device__ __forceinline__ void ib_hidden(const __bf16* xs, int xp, int nc, const uint16_t* w, int w_row, const float* bias, int W, int row0,
                                          int B, bool vec, int tid, __bf16* ys, int yp) {
  const auto [lane, wave, i, j] = ChainLane(tid);
  const bool ok = row0 + i < B;
  for (int t = wave; t < W / 16; t += CH_WAVES) {
    float bv[4], v[4];
    cb_load4(bias + 16 * t + 4 * j, vec, bv);
    const f32x4 acc = chain_stream_gemm<ChainOpsBf16>(xs + i * xp + 8 * j, w + (size_t)(16 * t + i) * w_row + 8 * j, nc, true);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float s = act_fwd(acc[r] + bv[r], S2P_ACT_RELU, 0.f);
      v[r] = ok ? s : 0.f;
    }
    cb_store4(ys + i * yp + 16 * t + 4 * j, v);
  }
}

// a(h) = tanh(last_fc(hs)): one column tile (A <= 8 of its 16 columns), wave 0; a lane holds the columns 4 j .. + 3 of row i.  -> act
// slot h, unrounded, and the fp32 LDS tile at[16][IM_AP], whose columns >= A and rows >= B are zeros.
__device__ __forceinline__ void ib_last(const ImagineArgsB& g, const __bf16* hs, int hp, int h, int row0, int tid, float* at) {
  const auto [lane, wave, i, j] = ChainLane(tid);
  if (wave != 0) return;
  const bool nok = i < g.A;
  const int W = g.p.width, gm = row0 + i;
  const f32x4 acc = chain_stream_gemm<ChainOpsBf16>(hs + i * hp + 8 * j, g.p.w3 + (size_t)(nok ? i : 0) * W + 8 * j, W / 32, nok);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = 4 * j + r;
    const bool ok = n < g.A && gm < g.c.B;
    const float v = ok ? act_fwd(acc[r] + g.p.b3[n < g.A ? n : 0], S2P_ACT_TANH, 0.f) : 0.f;
    if (n < IM_AP) at[i * IM_AP + n] = v;
    if (ok) g.act[((size_t)gm * g.c.T + h) * g.act_pitch + n] = v;
  }
}

__global__ __launch_bounds__(CH_THREADS) void posterior_chain_bf16_kernel(const ChainArgsB a) {
  __shared__ __attribute__((aligned(16))) __bf16 xz[CH_ROWS * CB_XZ_P], h1[CH_ROWS * CB_H_P], h2[CH_ROWS * CB_H_P];
  const int row0 = blockIdx.x * CH_ROWS;
  ChainBf16::Hidden<CH_FEAT, false> i1;
  ChainBf16::Hidden<CH_Z1, false> j1;
  ChainBf16::Hidden<CH_Z2, true> a1;
  ChainBf16::Hidden<CH_Z, true> b1;
  i1.ask(a, a.m[0].w1, a.m[0].w1_row, a.m[0].b1, nullptr, row0);
  chain_load_rows<ChainBf16, CH_Z1, CH_FEAT>(a.feat, a.feat_pitch, row0, a.B, xz);      // feat(0) -> xz[:, 32:]
  auto ask_a1 = [&](int t) {
    if (t < a.T) a1.ask(a, a.m[2].w1, a.m[2].w1_row, a.m[2].b1, a.ra + (size_t)(t - 1) * a.B * CH_HID, row0);
    else a1.forget();
  };
  // t = 0: q(z1(0) | feat(0)), q(z2(0) | z1(0))
  chain_mlp<ChainBf16, CH_Z1>(a, a.m[0], i1, xz + CH_Z1, 0, 0, row0, xz, h1, h2, [&] { j1.ask(a, a.m[1].w1, a.m[1].w1_row, a.m[1].b1, nullptr, row0); });
  chain_mlp<ChainBf16, CH_Z2>(a, a.m[1], j1, xz, 0, CH_Z1, row0, xz, h1, h2, [&] { ask_a1(1); });
  // q(z1(t) | feat(t), z2(t-1), a(t-1)), q(z2(t) | z1(t), z2(t-1), a(t-1)): the feat / action columns arrive as ra / rb
  for (int t = 1; t < a.T; ++t)
    chain_step<ChainBf16>(a, a.m[2], a.m[3], a1, b1, a.rb + (size_t)(t - 1) * a.B * CH_HID, t, row0, xz, h1, h2, [&] { ask_a1(t + 1); });
}

__global__ __launch_bounds__(CH_THREADS) void prior_chain_bf16_kernel(const ChainArgsB a) {
  __shared__ __attribute__((aligned(16))) __bf16 xz[CH_ROWS * CB_XZ_P], h1[CH_ROWS * CB_H_P], h2[CH_ROWS * CB_H_P];
  const int row0 = blockIdx.x * CH_ROWS;
  ChainBf16::Hidden<CH_Z2, true> a1;
  ChainBf16::Hidden<CH_Z, true> b1;
  auto ask_a1 = [&](int s) {
    if (s < a.T) a1.ask(a, a.m[0].w1, a.m[0].w1_row, a.m[0].b1, a.ra + (size_t)s * a.B * CH_HID, row0);
    else a1.forget();
  };
  ask_a1(0);
  chain_load_rows<ChainBf16, CH_Z1, CH_Z2>(a.feat, a.feat_pitch, row0, a.B, xz);
  for (int s = 0; s < a.T; ++s)
    chain_step<ChainBf16>(a, a.m[0], a.m[1], a1, b1, a.rb + (size_t)s * a.B * CH_HID, s, row0, xz, h1, h2, [&] { ask_a1(s + 1); });
}

__global__ __launch_bounds__(CH_THREADS) void imagine_chain_bf16_kernel(const ImagineArgsB g) {
  __shared__ __attribute__((aligned(16))) __bf16 xz[CH_ROWS * CB_XZ_P], pa[CH_ROWS * IB_P_MAX], pb[CH_ROWS * IB_P_MAX];
  __shared__ __attribute__((aligned(16))) float at[CH_ROWS * IM_AP];
  const ChainArgsB& a = g.c;
  const int row0 = blockIdx.x * CH_ROWS, W = g.p.width, pp = W + ChainBf16::PAD, kp = (g.A + 3) / 4 * 4;
  ChainBf16::Hidden<CH_Z2, true> a1;
  ChainBf16::Hidden<CH_Z, true> b1;
  chain_load_rows<ChainBf16, 0, CH_Z>(g.z0, g.z0_pitch, row0, a.B, xz);
  for (int s = 0; s < a.T; ++s) {
    const int tid = ib_tid();
    __syncthreads();                                       // xz = z(s); the latent half is done with h1 / h2 (= pa / pb)
    ib_hidden(xz, CB_XZ_P, CH_Z / 32, g.p.w1, g.p.w1_row, g.p.b1, W, row0, a.B, a.vec_in, tid, pa, pp);
    __syncthreads();
    ib_hidden(pa, pp, W / 32, g.p.w2, W, g.p.b2, W, row0, a.B, a.vec_in, tid, pb, pp);
    __syncthreads();
    ib_last(g, pb, pp, s, row0, tid, at);
    __syncthreads();
    a1.ask(a, a.m[0].w1, a.m[0].w1_row, a.m[0].b1, CbActionTerm{at, g.wc, g.wc_row, kp, tid}, row0);
    chain_step<ChainBf16>(a, a.m[0], a.m[1], a1, b1, CbActionTerm{at, g.wb, g.wb_row, kp, tid}, s, row0, xz, pa, pb, [] {});
  }
}

// ---- the posterior chain under grad in bf16 compute (SPEC.md N3p) ----------------------------------------------------------------------
// The training form of posterior_chain_bf16_kernel: every MLP with a ChainSaveT<true> that names where its h1, h2, raw and sample go in
// `s`, UNROUNDED (the values the epilogues hold before they round for LDS), so mean / std / z are bitwise the kernel above and the fp32
// launches after the chain (t = 0 backward, weight gradients) read what the fp32 form would have left them.  A kernel of its own, as
// posterior_chain_save_kernel is, so that the three kernels above keep their generated code.
__global__ __launch_bounds__(CH_THREADS) void posterior_chain_save_bf16_kernel(const ChainArgsB a, const s2p_chain_state s) {
  __shared__ __attribute__((aligned(16))) __bf16 xz[CH_ROWS * CB_XZ_P], h1[CH_ROWS * CB_H_P], h2[CH_ROWS * CB_H_P];
  using Sv = ChainSaveT<true>;
  const int row0 = blockIdx.x * CH_ROWS;
  const size_t B = a.B;
  ChainBf16::Hidden<CH_FEAT, false> i1;
  ChainBf16::Hidden<CH_Z1, false> j1;
  ChainBf16::Hidden<CH_Z2, true> a1;
  ChainBf16::Hidden<CH_Z, true> b1;
  i1.ask(a, a.m[0].w1, a.m[0].w1_row, a.m[0].b1, nullptr, row0);
  chain_load_rows<ChainBf16, CH_Z1, CH_FEAT>(a.feat, a.feat_pitch, row0, a.B, xz);
  auto ask_a1 = [&](int t) {
    if (t < a.T) a1.ask(a, a.m[2].w1, a.m[2].w1_row, a.m[2].b1, a.ra + (size_t)(t - 1) * a.B * CH_HID, row0);
    else a1.forget();
  };
  chain_mlp<ChainBf16, CH_Z1>(a, a.m[0], i1, xz + CH_Z1, 0, 0, row0, xz, h1, h2, [&] { j1.ask(a, a.m[1].w1, a.m[1].w1_row, a.m[1].b1, nullptr, row0); },
                       Sv(s.a0_h1, s.a0_h2, s.a0_raw, nullptr));
  chain_mlp<ChainBf16, CH_Z2>(a, a.m[1], j1, xz, 0, CH_Z1, row0, xz, h1, h2, [&] { ask_a1(1); },
                       Sv(s.b0_h1, s.b0_h2, s.b0_raw, a.T > 1 ? s.xz : nullptr));      // z2(0) -> xz[0][:, 32:]
  for (int t = 1; t < a.T; ++t) {
    const size_t r = (size_t)(t - 1) * B;                  // the first row of slot t - 1 in the time-major state
    chain_step<ChainBf16>(a, a.m[2], a.m[3], a1, b1, a.rb + (size_t)(t - 1) * a.B * CH_HID, t, row0, xz, h1, h2, [&] { ask_a1(t + 1); },
                   Sv(s.h1a + r * CH_HID, s.h2a + r * CH_HID, s.rawa + r * 2 * CH_Z1, s.xz + r * CH_Z),     // z1(t) -> xz[t-1][:, :32]
                   Sv(s.h1b + r * CH_HID, s.h2b + r * CH_HID, s.rawb + r * 2 * CH_Z2, t + 1 < a.T ? s.xz + (r + B) * CH_Z : nullptr));
  }
}

// The loop "for t = S .. 1" of the backward (posterior_chain_bwd_kernel of gauss_chain.hip) with its six input gradients per step in
// bf16 compute.  The head backwards are gauss_head_grad on fp32 inputs; draw goes to global memory in fp32 and, rounded, to `dr`.  An
// input gradient multiplies the transposed bf16 pack (the A operand, all of it asked for at once, as the forward layers do) with a
// bf16 LDS tile of g = draw or dh . act'(h); the multiply by act' is ONE fp32 multiply in the epilogue of the gradient in front, which
// also writes dh to global memory unrounded.  The gradient at xz is an fp32 tile: it is an addend and a head input, never an operand.
// LDS, static, nothing aliased, 52 224 bytes:
//   dr [16][520] bf16 draw of the head in flight    ta, tb [16][264] bf16 dh2 . act', dh1 . act'    dx [16][292] fp32 the gradient at xz
struct ChainBwdArgsB {
  const float* eps; const float* dmean; const float* dstd; const float* dz;
  int eps_pitch, dmean_pitch, dstd_pitch, dz_pitch, B, T;
  s2p_chain_mlp_bwd_bf16 m[2];                             // z1_posterior, z2_prior
  s2p_chain_state s;
  s2p_chain_grads g;
};
constexpr int CB_DR_P = 2 * CH_Z2 + CB_PAD, CB_DX_P = CH_Z + 4;

// One input gradient: o[16][NO] = xs[16][K] . w[NO][w_row]^T, xs = bf16(dy . act'(y)) already.  Wave v owns the column tiles v, v + 8,
// ...; a lane's four results are the columns 16 tile + 4 j .. + 3 of row i -> global `go` (pitch gp, 16-byte aligned) as they are, and
// the LDS tile `os`: PRE: times act'(ya), rounded, bf16 (ya [B][256]: the saved OUTPUT of the layer this gradient arrives at); else
// fp32 as they are.  ACC: (acc + os) + 0, the accumulating dgrad.  ask(): the weights and ya; it depends on nothing the chain computes.
// Only the waves that own the tile past the last full round (NO 288: waves 0 and 1) load and multiply it.
template <int K, int NO, bool ACC, bool PRE>
struct CbDgrad {
  static_assert(!(ACC && PRE), "the accumulating gradient arrives at xz");
  static constexpr int TILES = NO / 16, NF = TILES / CH_WAVES, NT = (TILES + CH_WAVES - 1) / CH_WAVES;
  using Out = std::conditional_t<PRE, __bf16, float>;
  bf16x8 wv[NT][K / 32];
  float yv[NT][4];

  int tid;                                                 // threadIdx.x as a value of the step (ib_tid): the addresses are made where they are used

  __device__ __forceinline__ explicit CbDgrad(int tid_) : tid(tid_) {}
  __device__ __forceinline__ bool has(int q) const { return q < NF || (tid >> 6) + q * CH_WAVES < TILES; }   // (wave-uniform)

  template <int Q0, int Q1>
  __device__ __forceinline__ void ask_part(const uint16_t* w, int w_row, const float* ya, int row0, int B) {
    const auto [lane, wave, i, j] = ChainLane(tid);
#pragma unroll
    for (int q = Q0; q < Q1; ++q) {
      const int t0 = 16 * (wave + q * CH_WAVES);
      const uint16_t* wr = w + (size_t)(t0 + i) * w_row + 8 * j;
#pragma unroll
      for (int r = 0; r < 4; ++r) yv[q][r] = 0.f;
      if (PRE && row0 + i < B) cb_load4(ya + (size_t)(row0 + i) * CH_HID + t0 + 4 * j, true, yv[q]);
#pragma unroll
      for (int c = 0; c < K / 32; ++c) wv[q][c] = *(const bf16x8*)(wr + 32 * c);
    }
  }

  __device__ __forceinline__ void ask(const uint16_t* w, int w_row, const float* ya, int row0, int B) {
    __builtin_amdgcn_sched_barrier(0);
    ask_part<0, NF>(w, w_row, ya, row0, B);
    if (NF < NT && has(NF)) ask_part<NF, NT>(w, w_row, ya, row0, B);
    __builtin_amdgcn_sched_barrier(0);                     // (the loads stay here: hipcc would sink them to their first use)
  }

  template <int Q0, int Q1>
  __device__ __forceinline__ void run_part(const __bf16* xs, int xp, int row0, int B, float* go, int gp, Out* os, int op) {
    const auto [lane, wave, i, j] = ChainLane(tid);
    f32x4 acc[NT];
#pragma unroll
    for (int q = Q0; q < Q1; ++q) acc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const __bf16* xr = xs + i * xp + 8 * j;
#pragma unroll
    for (int c = 0; c < K / 32; ++c) {
      const bf16x8 xv = *(const bf16x8*)(xr + 32 * c);
#pragma unroll
      for (int q = Q0; q < Q1; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv[q][c], xv, acc[q], 0, 0, 0);
    }
    const int gm = row0 + i;
    const bool ok = gm < B;
#pragma unroll
    for (int q = Q0; q < Q1; ++q) {
      const int c0 = 16 * (wave + q * CH_WAVES) + 4 * j;
      float v[4];
      f32x4 old = {0.f, 0.f, 0.f, 0.f};
      if constexpr (ACC) old = *(const f32x4*)(os + i * op + c0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float s = acc[q][r];
        if (ACC) s += old[r];
        v[r] = s + 0.f;                                    // (lin_fwd_kernel's "+ bias" without one: -0 becomes +0)
      }
      if (ok) cb_store4f(go + (size_t)gm * gp + c0, true, v);
      if constexpr (PRE) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = ok ? v[r] * act_grad_from_out(yv[q][r], S2P_ACT_LRELU, CH_SLOPE) : 0.f;
        cb_store4(os + i * op + c0, v);
      } else {
        *(f32x4*)(os + i * op + c0) = ok ? (f32x4){v[0], v[1], v[2], v[3]} : (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    }
  }

  __device__ __forceinline__ void run(const __bf16* xs, int xp, int row0, int B, float* go, int gp, Out* os, int op) {
    run_part<0, NF>(xs, xp, row0, B, go, gp, os, op);
    if (NF < NT && has(NF)) run_part<NF, NT>(xs, xp, row0, B, go, gp, os, op);
  }
};

// The head backward of D columns at step t: -> draw [B][2 D] of slot t - 1 in global memory, unrounded, and rounded to dr[:, : 2 D].
// WIDE (the z2 head): no dmean / dstd, and the carried gradient dx[:, 32:] only when `carry`; else (z1): dmean, dstd and dx[:, :32].
template <int D, bool WIDE>
__device__ __forceinline__ void cb_head_bwd(const ChainBwdArgsB& a, const float* raw, float* draw, int t, bool carry, int row0,
                                            const float* dx, __bf16* dr) {
  constexpr int off = WIDE ? CH_Z1 : 0;
  for (int e = threadIdx.x; e < CH_ROWS * D; e += CH_THREADS) {
    const int row = e / D, d = e % D, gm = row0 + row;
    GaussHeadGrad g = {0.f, 0.f};
    if (gm < a.B) {
      const size_t bt = (size_t)gm * a.T + t;
      const float dzv = a.dz[bt * a.dz_pitch + off + d], ev = a.eps[bt * a.eps_pitch + off + d], dz2 = dx[row * CB_DX_P + off + d];
      const float rs = raw[(size_t)gm * (2 * D) + D + d];
      if (WIDE) g = gauss_head_grad(true, dzv, carry, dz2, false, 0.f, false, 0.f, true, ev, rs);
      else g = gauss_head_grad(true, dzv, true, dz2, true, a.dmean[bt * a.dmean_pitch + d], true, a.dstd[bt * a.dstd_pitch + d], true, ev, rs);
      draw[(size_t)gm * (2 * D) + d] = g.dmu;
      draw[(size_t)gm * (2 * D) + D + d] = g.draw_std;
    }
    dr[row * CB_DR_P + d] = (__bf16)g.dmu;
    dr[row * CB_DR_P + D + d] = (__bf16)g.draw_std;
  }
}

// A gradient is asked for one stage early where the operands of two stages fit the registers beside an epilogue (the sums are
// in DESIGN.md section 6b.25): a3, a2 and a1 before the stage in front of each runs; b3, b2 and b1 after it, before its barrier.
__global__ __launch_bounds__(CH_THREADS) void posterior_chain_bwd_bf16_kernel(const ChainBwdArgsB a) {
  __shared__ __attribute__((aligned(16))) __bf16 dr[CH_ROWS * CB_DR_P], ta[CH_ROWS * CB_H_P], tb[CH_ROWS * CB_H_P];
  __shared__ __attribute__((aligned(16))) float dx[CH_ROWS * CB_DX_P];
  const int row0 = blockIdx.x * CH_ROWS, B = a.B, S = a.T - 1;
  const s2p_chain_mlp_bwd_bf16& ma = a.m[0];
  const s2p_chain_mlp_bwd_bf16& mb = a.m[1];
  for (int e = threadIdx.x; e < CH_ROWS * CB_DX_P; e += CH_THREADS) dx[e] = 0.f;   // (read at t = S only as an operand that is not added)
  __syncthreads();
  for (int t = S; t >= 1; --t) {
    const size_t r = (size_t)(t - 1) * B;                  // the first row of slot t - 1
    const int tid = ib_tid();
    // the z2 MLP: head, 512 -> 256, 256 -> 256, 256 -> 288
    CbDgrad<2 * CH_Z2, CH_HID, false, true> b3(tid);
    CbDgrad<CH_HID, CH_HID, false, true> b2(tid);
    CbDgrad<CH_HID, CH_Z, false, false> b1(tid);
    // the z1 MLP: head, 64 -> 256, 256 -> 256, 256 -> 256 added to dxz[:, 32:], the gradient at z2(t-1) that step t - 1 takes up
    CbDgrad<2 * CH_Z1, CH_HID, false, true> a3(tid);
    CbDgrad<CH_HID, CH_HID, false, true> a2(tid);
    CbDgrad<CH_HID, CH_Z2, true, false> a1(tid);
    b3.ask(mb.w3t, 2 * CH_Z2, a.s.h2b + r * CH_HID, row0, B);
    cb_head_bwd<CH_Z2, true>(a, a.s.rawb + r * 2 * CH_Z2, a.g.drawb + r * 2 * CH_Z2, t, t < S, row0, dx, dr);
    __syncthreads();
    b3.run(dr, CB_DR_P, row0, B, a.g.dh2b + r * CH_HID, CH_HID, ta, CB_H_P);
    b2.ask(mb.w2t, CH_HID, a.s.h1b + r * CH_HID, row0, B);
    __syncthreads();
    b2.run(ta, CB_H_P, row0, B, a.g.dh1b + r * CH_HID, CH_HID, tb, CB_H_P);
    b1.ask(mb.w1t, mb.w1t_row, nullptr, row0, B);
    __syncthreads();
    a3.ask(ma.w3t, 2 * CH_Z1, a.s.h2a + r * CH_HID, row0, B);
    b1.run(tb, CB_H_P, row0, B, a.g.dxz + r * CH_Z, CH_Z, dx, CB_DX_P);
    __syncthreads();
    cb_head_bwd<CH_Z1, false>(a, a.s.rawa + r * 2 * CH_Z1, a.g.drawa + r * 2 * CH_Z1, t, true, row0, dx, dr);
    __syncthreads();
    a2.ask(ma.w2t, CH_HID, a.s.h1a + r * CH_HID, row0, B);
    a3.run(dr, CB_DR_P, row0, B, a.g.dh2a + r * CH_HID, CH_HID, ta, CB_H_P);
    __syncthreads();
    a1.ask(ma.w1t, ma.w1t_row, nullptr, row0, B);
    a2.run(ta, CB_H_P, row0, B, a.g.dh1a + r * CH_HID, CH_HID, tb, CB_H_P);
    __syncthreads();
    a1.run(tb, CB_H_P, row0, B, a.g.dxz + r * CH_Z + CH_Z1, CH_Z, dx + CH_Z1, CB_DX_P);
    __syncthreads();
  }
}

// ---- bf16 packs of fp32 matrices, several per launch (s2p_chain_pack_bf16) ------------------------------------------------------------
constexpr int PK_JOBS = 16, PK_TILE = 32, PK_THREADS = 256;
struct ChainPackArgs { s2p_bf16_pack_job j[PK_JOBS]; };

// fp32 -> bf16 bits, round to nearest even in integer arithmetic: what a cast gives for every finite value, +-0 and +-inf (a finite
// value past the largest bf16 becomes inf); a NaN becomes the quiet NaN of its sign.
__device__ __forceinline__ uint16_t pk_round(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x7fc0u);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// grid (tiles, jobs): a workgroup rounds one 32 x 32 tile of its job, writes it to dst and, through LDS, transposed to dst_t, both
// with unit stride along the lanes.  Nothing outside [rows][cols] of dst and [cols][rows] of dst_t is written.
__global__ __launch_bounds__(PK_THREADS) void chain_pack_bf16_kernel(const ChainPackArgs a) {
  __shared__ uint16_t tile[PK_TILE][PK_TILE + 1];
  const s2p_bf16_pack_job& job = a.j[blockIdx.y];
  const int rows = job.rows, cols = job.cols, tcols = (cols + PK_TILE - 1) / PK_TILE, trows = (rows + PK_TILE - 1) / PK_TILE;
  if ((int)blockIdx.x >= tcols * trows) return;                                // (uniform for the workgroup)
  const int r0 = PK_TILE * (blockIdx.x / tcols), c0 = PK_TILE * (blockIdx.x % tcols), tx = threadIdx.x % PK_TILE, ty = threadIdx.x / PK_TILE;
  for (int k = ty; k < PK_TILE; k += PK_THREADS / PK_TILE) {
    const int row = r0 + k, col = c0 + tx;
    if (row < rows && col < cols) {
      const uint16_t v = pk_round(job.src[(size_t)row * job.src_pitch + col]);
      if (job.dst) job.dst[(size_t)row * job.dst_pitch + col] = v;
      tile[k][tx] = v;
    }
  }
  __syncthreads();
  if (!job.dst_t) return;
  for (int k = ty; k < PK_TILE; k += PK_THREADS / PK_TILE) {
    const int row = r0 + tx, col = c0 + k;
    if (row < rows && col < cols) job.dst_t[(size_t)col * job.dst_t_pitch + row] = tile[tx][k];
  }
}
}  // namespace

// ---- host side: the operand checks and the launch frame are gauss_chain_common.h's; set_vec() is this mode's own ----------------------
extern "C" int s2p_posterior_chain_fwd_bf16(const float* feat, int feat_pitch, const float* ra, const float* rb, const float* eps,
                                            int eps_pitch, const s2p_chain_mlp_bf16* mlps, float* mean, int mean_pitch, float* std,
                                            int std_pitch, float* z, int z_pitch, int B, int T, void* stream) {
  const char* who = "s2p_posterior_chain_fwd_bf16";
  if (int e = chain_sizes(who, B, T); e <= 0) return e;
  ChainArgsB a{};
  if (int e = posterior_chain_take(who, feat, feat_pitch, ra, rb, eps, eps_pitch, mlps, mean, mean_pitch, std, std_pitch, z, z_pitch, B, T, a))
    return e;
  a.set_vec(T > 1 ? 4 : 2);
  return chain_launch("posterior_chain_bf16_kernel", posterior_chain_bf16_kernel, B, stream, a);
}

extern "C" int s2p_posterior_chain_fwd_save_bf16(const float* feat, int feat_pitch, const float* ra, const float* rb, const float* eps,
                                                 int eps_pitch, const s2p_chain_mlp_bf16* mlps, float* mean, int mean_pitch, float* std,
                                                 int std_pitch, float* z, int z_pitch, const s2p_chain_state* state, int B, int T,
                                                 void* stream) {
  const char* who = "s2p_posterior_chain_fwd_save_bf16";
  if (int e = chain_sizes(who, B, T); e <= 0) return e;
  ChainArgsB a{};
  if (int e = posterior_chain_take(who, feat, feat_pitch, ra, rb, eps, eps_pitch, mlps, mean, mean_pitch, std, std_pitch, z, z_pitch, B, T, a))
    return e;
  if (int e = chain_check_state(who, state, T)) return e;
  a.set_vec(T > 1 ? 4 : 2);
  return chain_launch("posterior_chain_save_bf16_kernel", posterior_chain_save_bf16_kernel, B, stream, a, *state);
}

extern "C" int s2p_posterior_chain_bwd_bf16(const float* eps, int eps_pitch, const float* dmean, int dmean_pitch, const float* dstd,
                                            int dstd_pitch, const float* dz, int dz_pitch, const s2p_chain_mlp_bwd_bf16* mlps,
                                            const s2p_chain_state* state, const s2p_chain_grads* grads, int B, int T, void* stream) {
  const char* who = "s2p_posterior_chain_bwd_bf16";
  if (int e = chain_sizes(who, B, T, 2); e <= 0) return e;    // (T == 1: the chain has no step)
  ChainBwdArgsB a{};
  if (int e = posterior_bwd_take(who, eps, eps_pitch, dmean, dmean_pitch, dstd, dstd_pitch, dz, dz_pitch, mlps, state, grads, B, T, a))
    return e;
  return chain_launch("posterior_chain_bwd_bf16_kernel", posterior_chain_bwd_bf16_kernel, B, stream, a);
}

extern "C" int s2p_chain_pack_bf16(const s2p_bf16_pack_job* jobs, int n_jobs, void* stream) {
  const char* who = "s2p_chain_pack_bf16";
  S2P_REQUIRE(n_jobs >= 0, "%s: negative size", who);
  if (n_jobs == 0) return 0;
  S2P_REQUIRE(jobs, "%s: null pointer (jobs is required)", who);
  for (int n = 0; n < n_jobs; ++n) {
    const s2p_bf16_pack_job& j = jobs[n];
    S2P_REQUIRE(j.rows >= 0 && j.cols >= 0, "%s: job %d: negative size", who, n);
    if (j.rows == 0 || j.cols == 0) continue;
    S2P_REQUIRE(j.src && (j.dst || j.dst_t), "%s: job %d: null pointer (src and one of dst, dst_t are required)", who, n);
    S2P_REQUIRE(j.src_pitch >= j.cols && (!j.dst || j.dst_pitch >= j.cols) && (!j.dst_t || j.dst_t_pitch >= j.rows),
                "%s: job %d: a pitch is below its row (src cols, dst cols, dst_t rows)", who, n);
  }
  ChainPackArgs a{};
  int m = 0, tiles = 0;
  for (int n = 0; n < n_jobs; ++n) {
    const s2p_bf16_pack_job& j = jobs[n];
    if (j.rows > 0 && j.cols > 0) {
      a.j[m++] = j;
      tiles = std::max(tiles, cdiv(j.rows, PK_TILE) * cdiv(j.cols, PK_TILE));
    }
    if (m == PK_JOBS || (n + 1 == n_jobs && m > 0)) {                          // (at most PK_JOBS jobs ride in one launch's arguments)
      hipLaunchKernelGGL(chain_pack_bf16_kernel, dim3(tiles, m), dim3(PK_THREADS), 0, (hipStream_t)stream, a);
      S2P_CHECK_LAUNCH("chain_pack_bf16_kernel");
      m = tiles = 0;
    }
  }
  return 0;
}

extern "C" int s2p_prior_chain_fwd_bf16(const float* z2_0, int z2_0_pitch, const float* rc, const float* rb, const float* eps,
                                        int eps_pitch, const s2p_chain_mlp_bf16* mlps, float* mean, int mean_pitch, float* std,
                                        int std_pitch, float* z, int z_pitch, int B, int H, void* stream) {
  const char* who = "s2p_prior_chain_fwd_bf16";
  if (int e = chain_sizes(who, B, H); e <= 0) return e;
  ChainArgsB a{};
  if (int e = prior_chain_take(who, z2_0, z2_0_pitch, rc, rb, eps, eps_pitch, mlps, mean, mean_pitch, std, std_pitch, z, z_pitch, B, H, a))
    return e;
  a.set_vec(2);
  return chain_launch("prior_chain_bf16_kernel", prior_chain_bf16_kernel, B, stream, a);
}

extern "C" int s2p_imagine_chain_fwd_bf16(const float* z0, int z0_pitch, const float* eps, int eps_pitch, const s2p_chain_mlp_bf16* mlps,
                                          const float* wc, int wc_row, const float* wb, int wb_row, int A,
                                          const s2p_policy_mlp_bf16* policy, float* act, int act_pitch, float* mean, int mean_pitch,
                                          float* std, int std_pitch, float* z, int z_pitch, int B, int H, void* stream) {
  const char* who = "s2p_imagine_chain_fwd_bf16";
  if (int e = chain_sizes(who, B, H); e <= 0) return e;
  ImagineArgsB g{};
  if (int e = imagine_chain_take(who, z0, z0_pitch, eps, eps_pitch, mlps, wc, wc_row, wb, wb_row, A, policy, act, act_pitch, mean, mean_pitch,
                                 std, std_pitch, z, z_pitch, B, H, g))
    return e;
  g.c.set_vec(2);
  g.c.vec_in &= s2p_al16(g.p.b1) && s2p_al16(g.p.b2);      // (the policy's hidden layers read their biases with cb_load4)
  return chain_launch("imagine_chain_bf16_kernel", imagine_chain_bf16_kernel, B, stream, g);
}
