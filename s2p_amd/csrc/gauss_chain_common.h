// What the fused SLAC latent chains share between their two compute modes: gauss_chain.hip (fp32; SPEC.md N3h, N3i, N3j, N3k) and
// gauss_chain_bf16.hip (bf16 operands, fp32 sums; N3m, N3n, N3p).  Both are one design -- a workgroup owns 16 batch rows and every output column
// of every layer, workgroup barriers only (the head of gauss_chain.hip has the reasoning) -- and differ in how a LAYER multiplies.  A file
// keeps its layers, its kernels and its entry points and names the layers in a MODE type (ChainF32, ChainBf16):
//   Args, Mlp, Elem            the kernel-argument struct, the host struct of one MLP's operands, the element of the LDS activation tiles
//   XZ_P, H_P, PAD             the row pitches of xz and of h1 / h2, the padding in them
//   Hidden<K, ADD>, Head<D>    ask(a, ...): everything that does not depend on the layer in front, asked for before the barrier that ends
//                              it; run(...) after that barrier; Hidden::forget(): bf16 drops the operands where a step asks for no next one
//   AHEAD                      layer 2 of an MLP is asked for before layer 1 runs (bf16: S2P_CHAIN_BF16_AHEAD) or after it (fp32)
//   put4(dst, v)               four fp32 values to an LDS activation row
// Here, once: the dimensions and build knobs; ChainLane; ChainSaveT; the control skeleton chain_mlp / chain_step / chain_load_rows over a
// mode; chain_stream_gemm, the policy half's GEMM over an operand-traits type (Vec, X, W, KSTEP, mma()); and the host side: head tables,
// operand checks, launch frame.  All of it is __forceinline__ with compile-time mode choices, and the eight kernels' instruction streams
// are what they were when each file spelled it out.  They sit AT the register ceiling and hipcc's result there
// depends on the ORDER it inlines in: a change here is judged by -Rpass-analysis=kernel-resource-usage and the assembly of all eight.
// That is also why the kernel bodies and the policy layers' epilogues are still written per file (section 6b.24 has what was tried).
//
// The ORDER of the operand checks, the same in both modes (a call that breaks several conditions gets the first one's message):
//   1. a negative size; B == 0 or T == 0 (the backward: T < 2) is a no-op that looks at no pointer
//   2. the entry's own pointers (posterior: feat, mlps, then ra / rb when T > 1; prior: z2_0, rc, rb, mlps; imagination: z0, mlps, wc, wb,
//      policy, act, then the action width; backward: all seven, then its pitches)
//   3. chain_take_views: eps, mean, std, z, then their pitches     4. the source rows: pitch (imagination: z0 288 and act A), alignment
//   5. imagination: wc_row / wb_row, alignment of wc / wb          6. chain_take_mlps, head by head: null operand, k1, row, alignment
//   7. imagination: chain_check_policy: null operand, width, w1_row, alignment;  save form and backward: state (and grads) buffers
#pragma once
#include "gauss_dev.h"

namespace {
// ---- dimensions, limits and knobs ---------------------------------------------------------------------------------------------------
constexpr int CH_Z1 = 32, CH_Z2 = 256, CH_Z = CH_Z1 + CH_Z2, CH_HID = 256, CH_FEAT = 256;
#ifndef S2P_CHAIN_THREADS
#define S2P_CHAIN_THREADS 512
#endif
#ifndef S2P_CHAIN_INFLIGHT
#define S2P_CHAIN_INFLIGHT 8                               // fp32: weight loads (16 bytes per lane) a wave asks for per block of k-chunks
#endif
#ifndef S2P_CHAIN_PAD
#define S2P_CHAIN_PAD 4                                    // fp32: floats added to the LDS row pitch of the activation tiles
#endif
#ifndef S2P_CHAIN_BF16_AHEAD
#define S2P_CHAIN_BF16_AHEAD 1                             // bf16: 1: an MLP's layer 2 is asked for before its layer 1 runs; 0: after
#endif
constexpr int CH_THREADS = S2P_CHAIN_THREADS, CH_WAVES = CH_THREADS / 64, CH_ROWS = 16;
constexpr float CH_SLOPE = 0.2f;
constexpr bool CB_AHEAD = S2P_CHAIN_BF16_AHEAD != 0;
constexpr int IM_WMAX = 1024, IM_AP = 8;                   // widest policy hidden layer; columns of the fp32 LDS action tile (A <= 8)

// A lane's place in the 16 x 16 MFMA tile of its wave: lane 16 j + i.  `tid`: threadIdx.x, or the bf16 imagination kernel's ib_tid().
struct ChainLane {
  int lane, wave, i, j;
  __device__ __forceinline__ explicit ChainLane(int tid) : lane(tid & 63), wave(tid >> 6), i(lane & 15), j(lane >> 4) {}
};

// What the training form of the posterior chain (SPEC.md N3k) stores of one MLP at one time step, beside what every chain stores:
// h1, h2 [B][256], raw [B][2 D] = acc + bias of the last layer, and the sample at its place in the saved input rows xz ([B][288] rows
// of the step that reads it; nullptr: no step does).  ChainSaveT<false> holds nothing and every use of it is compiled out.
template <bool SAVE>
struct ChainSaveT {
  static constexpr bool on = false;
  __device__ __forceinline__ ChainSaveT() {}
  __device__ __forceinline__ ChainSaveT(float*, float*, float*, float*) {}
};
template <>
struct ChainSaveT<true> {
  static constexpr bool on = true;
  float *h1, *h2, *raw, *xz;
  __device__ __forceinline__ ChainSaveT(float* h1_, float* h2_, float* raw_, float* xz_) : h1(h1_), h2(h2_), raw(raw_), xz(xz_) {}
};
using ChainNoSave = ChainSaveT<false>;

// The imagination chain's arguments: C the mode's chain arguments, P its policy struct.
template <typename C, typename P>
struct ImagineArgsT {
  C c;                                                     // feat / ra / rb unused; m[0] / m[1] = z1_prior / z2_prior; T = H
  const float* z0; const float* wc; const float* wb; float* act;
  int z0_pitch, wc_row, wb_row, act_pitch, A;
  P p;
};

// ---- the control skeleton ---------------------------------------------------------------------------------------------------------------
// Layers 2 and 3 of a Gaussian MLP whose first layer `l1` has been asked for: input xs, output z(t)[:, off : off + D].  After the head,
// before the next MLP's first barrier, it asks for the first layer of the NEXT MLP through `next()`.  M::AHEAD: layer 2, which depends
// on nothing, is asked for before layer 1 runs instead of after it (bf16: 136 VGPRs of weights live; the same for the head or for
// next() would put 192 to 216 VGPRs of weights beside the epilogue's operands and hipcc then spills 112 to 316 bytes per lane).
// `sv`: where the SAVE variant stores this MLP's h1, h2, raw and sample (ChainNoSave: nowhere).
template <typename M, int D, typename L1, typename Next, typename Save = ChainNoSave>
__device__ __forceinline__ void chain_mlp(const typename M::Args& a, const typename M::Mlp& m, L1& l1, const typename M::Elem* xs, int t, int off,
                                          int row0, typename M::Elem* xz, typename M::Elem* h1, typename M::Elem* h2, Next next,
                                          const Save sv = Save()) {
  typename M::template Hidden<CH_HID, false> l2;
  typename M::template Head<D> l3;
  __syncthreads();
  if (M::AHEAD) l2.ask(a, m.w2, CH_HID, m.b2, nullptr, row0);
  if constexpr (Save::on) l1.template run<true>(xs, M::XZ_P, row0, a.B, h1, sv.h1);
  else l1.run(xs, M::XZ_P, row0, a.B, h1);
  if (!M::AHEAD) l2.ask(a, m.w2, CH_HID, m.b2, nullptr, row0);
  __syncthreads();
  if constexpr (Save::on) l2.template run<true>(h1, M::H_P, row0, a.B, h2, sv.h2);
  else l2.run(h1, M::H_P, row0, a.B, h2);
  l3.ask(a, m.w3, m.b3, t, off, row0);
  __syncthreads();
  if constexpr (Save::on) l3.run(a, h2, t, off, row0, xz, sv);
  else l3.run(a, h2, t, off, row0, xz);
  next();
}

// One chain step, shared by the posterior chain (t >= 1), the prior chain and the imagination chain (every step): the z1 MLP `ma` on
// xz[:, 32:288] = z2(t-1) with its first layer `a1` already asked for, then the z2 MLP `mb` on xz = z1(t) | z2(t-1) with the additive
// term `add_b`: a global pointer ([B][256] rows of this step) or the mode's action term.  Results go to slot t of eps / mean / std / z.
// `next()` asks for whatever follows the step, before the step's last barrier.  `sa` / `sb`: the two MLPs' ChainSaveT.
template <typename M, typename Add, typename Next, typename Save = ChainNoSave>
__device__ __forceinline__ void chain_step(const typename M::Args& a, const typename M::Mlp& ma, const typename M::Mlp& mb,
                                           typename M::template Hidden<CH_Z2, true>& a1, typename M::template Hidden<CH_Z, true>& b1,
                                           const Add add_b, int t, int row0, typename M::Elem* xz, typename M::Elem* h1, typename M::Elem* h2,
                                           Next next, const Save sa = Save(), const Save sb = Save()) {
  chain_mlp<M, CH_Z1>(a, ma, a1, xz + CH_Z1, t, 0, row0, xz, h1, h2, [&] { b1.ask(a, mb.w1, mb.w1_row, mb.b1, add_b, row0); }, sa);
  chain_mlp<M, CH_Z2>(a, mb, b1, xz, t, CH_Z1, row0, xz, h1, h2, next, sb);
}

// src[16 rows][W] fp32 -> xz[:, C0 : C0 + W]; rows >= B are zeros, and so is every activation row derived from them
template <typename M, int C0, int W>
__device__ __forceinline__ void chain_load_rows(const float* src, int pitch, int row0, int B, typename M::Elem* xz) {
  for (int idx = threadIdx.x; idx < CH_ROWS * (W / 4); idx += CH_THREADS) {
    const int row = idx / (W / 4), c4 = idx % (W / 4), gm = row0 + row;
    const f32x4 v = gm < B ? *(const f32x4*)(src + (size_t)gm * pitch + 4 * c4) : (f32x4){0.f, 0.f, 0.f, 0.f};
    M::put4(xz + row * M::XZ_P + C0 + 4 * c4, v);
  }
}

// ---- the policy half of the closed-loop imagination chain (SPEC.md N3j, N3n) -------------------------------------------------------------
// One 16 x 16 tile of x[16 rows][KSTEP nc] . w[16 columns][KSTEP nc]^T: O::mma over the k-steps 0 .. nc - 1 in ascending order from a
// zero accumulator (fp32: lin_mfma_chunk, what lin_fwd_kernel does for an element; its zero chunks past K add nothing).  nc is a
// run-time value (the policy's width): blocks of 8 k-steps, the next block's operands load while this one is multiplied.  xr / wr: this
// lane's LDS activation row and weight row at its first k; wok false (a column past N): zero weights, as lin_fwd_kernel feeds them.
template <typename O>
__device__ __forceinline__ f32x4 chain_stream_gemm(const typename O::X* xr, const typename O::W* wr, int nc, bool wok) {
  using Vec = typename O::Vec;
  constexpr int U = 8;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  Vec xa[U], wa[U], xb[U], wb[U];
  auto load = [&](Vec (&xv)[U], Vec (&wv)[U], int c0) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (c0 + u < nc) {
        xv[u] = *(const Vec*)(xr + O::KSTEP * (c0 + u));
        wv[u] = wok ? *(const Vec*)(wr + O::KSTEP * (c0 + u)) : Vec{};
      }
  };
  auto mul = [&](const Vec (&xv)[U], const Vec (&wv)[U], int c0) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (c0 + u < nc) acc = O::mma(xv[u], wv[u], acc);
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

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
struct ChainHeadSpec { int k1; const char* name; };        // the chain columns of a head's first layer, and the head's name in messages
const ChainHeadSpec CH_POSTERIOR_HEADS[4] = {{CH_FEAT, "z1_posterior_init"}, {CH_Z1, "z2_prior_init"}, {CH_Z2, "z1_posterior"}, {CH_Z, "z2_prior"}};
const ChainHeadSpec CH_PRIOR_HEADS[2] = {{CH_Z2, "z1_prior"}, {CH_Z, "z2_prior"}};

// A weight row is read 16 bytes at a time: the multiple of elements its pitch must be, and how a message says so.
template <typename W> struct ChainRowUnit;
template <> struct ChainRowUnit<float> { static constexpr int mult = 4; static constexpr const char* text = "4 floats"; };
template <> struct ChainRowUnit<uint16_t> { static constexpr int mult = 8; static constexpr const char* text = "8 bf16 elements"; };
template <typename S> using ChainRowOf = ChainRowUnit<std::remove_cv_t<std::remove_pointer_t<decltype(S::w1)>>>;

// How chain_take_mlps reads a host struct of one MLP's operands: s2p_chain_mlp and s2p_chain_mlp_bf16 here, the transposed packs of
// the two backwards below.
template <typename Mlp>
struct ChainMlpFields {
  using Unit = ChainRowOf<Mlp>;
  static constexpr const char *row_name = "w1_row", *least_name = "K";
  static bool given(const Mlp& m) { return m.w1 && m.b1 && m.w2 && m.b2 && m.w3 && m.b3; }
  static bool aligned(const Mlp& m) { return s2p_al16(m.w1) && s2p_al16(m.w2) && s2p_al16(m.w3); }
  static int row(const Mlp& m) { return m.w1_row; }
  static int least(const Mlp& m) { return m.k1; }
};

// The transposed packs of the backward (s2p_chain_mlp_bwd: fp32; s2p_chain_mlp_bwd_bf16: bf16 bits): all three given and aligned, a
// w1t row holds the 256 hidden columns.
template <typename Mlp, typename W>
struct ChainMlpBwdFields {
  using Unit = ChainRowUnit<W>;
  static constexpr const char *row_name = "w1t_row", *least_name = "256";
  static bool given(const Mlp& m) { return m.w1t && m.w2t && m.w3t; }
  static bool aligned(const Mlp& m) { return s2p_al16(m.w1t) && s2p_al16(m.w2t) && s2p_al16(m.w3t); }
  static int row(const Mlp& m) { return m.w1t_row; }
  static int least(const Mlp&) { return CH_HID; }
};
template <> struct ChainMlpFields<s2p_chain_mlp_bwd> : ChainMlpBwdFields<s2p_chain_mlp_bwd, float> {};
template <> struct ChainMlpFields<s2p_chain_mlp_bwd_bf16> : ChainMlpBwdFields<s2p_chain_mlp_bwd_bf16, uint16_t> {};

// Checks `n` host structs against `spec` and copies them into a.m. 0, or S2P_REQUIRE's value with the error text set.
template <typename Mlp, typename Args>
int chain_take_mlps(const char* who, const Mlp* mlps, const ChainHeadSpec* spec, int n, Args& a) {
  using F = ChainMlpFields<Mlp>;
  for (int g = 0; g < n; ++g) {
    const Mlp& m = mlps[g];
    const char* name = spec[g].name;
    S2P_REQUIRE(F::given(m), "%s: %s: null operand", who, name);
    S2P_REQUIRE(m.k1 == spec[g].k1, "%s: %s: the first layer's K is %d, %d is built", who, name, (int)m.k1, spec[g].k1);
    S2P_REQUIRE(F::row(m) >= F::least(m) && F::row(m) % F::Unit::mult == 0, "%s: %s: %s must be a multiple of %s and at least %s", who, name,
                F::row_name, F::Unit::text, F::least_name);
    S2P_REQUIRE(F::aligned(m), "%s: %s: the weights must be 16-byte aligned", who, name);
    a.m[g] = m;
  }
  return 0;
}

// Checks the [B, T, C] views every chain reads (eps) and writes (mean, std, z) and fills them, B and T into `a`.  Returns as above.
template <typename Args>
int chain_take_views(const char* who, const float* eps, int eps_pitch, float* mean, int mean_pitch, float* std, int std_pitch, float* z,
                     int z_pitch, int B, int T, Args& a) {
  S2P_REQUIRE(eps && mean && std && z, "%s: null pointer (eps, mean, std and z are required)", who);
  S2P_REQUIRE(eps_pitch >= CH_Z && mean_pitch >= CH_Z1 && std_pitch >= CH_Z1 && z_pitch >= CH_Z,
              "%s: a pitch is below its row (eps 288, mean 32, std 32, z 288)", who);
  a.eps = eps; a.eps_pitch = eps_pitch; a.mean = mean; a.mean_pitch = mean_pitch; a.std = std; a.std_pitch = std_pitch; a.z = z;
  a.z_pitch = z_pitch; a.B = B; a.T = T;
  return 0;
}

// The [B][>= 256] fp32 source rows chain_load_rows reads 16 bytes at a time (feat, z2_0; z0, whose 288 the caller has checked)
int chain_check_src(const char* who, const char* name, const float* src, int pitch) {
  S2P_REQUIRE(pitch >= 256, "%s: the pitch of %s is below its row of 256", who, name);
  S2P_REQUIRE(s2p_al16(src) && pitch % 4 == 0, "%s: %s must be 16-byte aligned, its pitch a multiple of 4 floats", who, name);
  return 0;
}

// The operand checks of the posterior chain, for all of its forms.  0 with `a` filled, or S2P_REQUIRE's value with the error text set.
template <typename Mlp, typename Args>
int posterior_chain_take(const char* who, const float* feat, int feat_pitch, const float* ra, const float* rb, const float* eps,
                         int eps_pitch, const Mlp* mlps, float* mean, int mean_pitch, float* std, int std_pitch, float* z, int z_pitch,
                         int B, int T, Args& a) {
  S2P_REQUIRE(feat && mlps, "%s: null pointer (feat and mlps are required)", who);
  S2P_REQUIRE(T == 1 || (ra && rb), "%s: ra and rb are required when T > 1", who);
  if (int e = chain_take_views(who, eps, eps_pitch, mean, mean_pitch, std, std_pitch, z, z_pitch, B, T, a)) return e;
  if (int e = chain_check_src(who, "feat", feat, feat_pitch)) return e;
  if (int e = chain_take_mlps(who, mlps, CH_POSTERIOR_HEADS, T > 1 ? 4 : 2, a)) return e;
  a.feat = feat; a.feat_pitch = feat_pitch; a.ra = ra; a.rb = rb;
  return 0;
}

// The same for the prior chain
template <typename Mlp, typename Args>
int prior_chain_take(const char* who, const float* z2_0, int z2_0_pitch, const float* rc, const float* rb, const float* eps, int eps_pitch,
                     const Mlp* mlps, float* mean, int mean_pitch, float* std, int std_pitch, float* z, int z_pitch, int B, int H, Args& a) {
  S2P_REQUIRE(z2_0 && rc && rb && mlps, "%s: null pointer (z2_0, rc, rb and mlps are required)", who);
  if (int e = chain_take_views(who, eps, eps_pitch, mean, mean_pitch, std, std_pitch, z, z_pitch, B, H, a)) return e;
  if (int e = chain_check_src(who, "z2_0", z2_0, z2_0_pitch)) return e;
  if (int e = chain_take_mlps(who, mlps, CH_PRIOR_HEADS, 2, a)) return e;
  a.feat = z2_0; a.feat_pitch = z2_0_pitch; a.ra = rc; a.rb = rb;
  return 0;
}

// The policy of the imagination chain: s2p_policy_mlp or s2p_policy_mlp_bf16
template <typename P>
int chain_check_policy(const char* who, const P& p) {
  S2P_REQUIRE(p.w1 && p.b1 && p.w2 && p.b2 && p.w3 && p.b3, "%s: policy: null operand", who);
  S2P_REQUIRE(p.width >= 128 && p.width <= IM_WMAX && p.width % 128 == 0,
              "%s: policy: hidden width %d, multiples of 128 from 128 to 1024 are built", who, (int)p.width);
  S2P_REQUIRE(p.w1_row >= CH_Z && p.w1_row % ChainRowOf<P>::mult == 0, "%s: policy: w1_row must be a multiple of %s and at least K", who,
              ChainRowOf<P>::text);
  S2P_REQUIRE(s2p_al16(p.w1) && s2p_al16(p.w2) && s2p_al16(p.w3), "%s: policy: the weights must be 16-byte aligned", who);
  return 0;
}

// The same for the imagination chain: its own operands (A, z0, act, wc, wb), the views, the two prior heads and the policy -> `g`.
template <typename Mlp, typename P, typename G>
int imagine_chain_take(const char* who, const float* z0, int z0_pitch, const float* eps, int eps_pitch, const Mlp* mlps, const float* wc,
                       int wc_row, const float* wb, int wb_row, int A, const P* policy, float* act, int act_pitch, float* mean,
                       int mean_pitch, float* std, int std_pitch, float* z, int z_pitch, int B, int H, G& g) {
  S2P_REQUIRE(z0 && mlps && wc && wb && policy && act, "%s: null pointer (z0, mlps, wc, wb, policy and act are required)", who);
  S2P_REQUIRE(A >= 1 && A <= IM_AP, "%s: action width %d, 1 .. 8 is built", who, A);
  const int kp = (A + 3) / 4 * 4;
  if (int e = chain_take_views(who, eps, eps_pitch, mean, mean_pitch, std, std_pitch, z, z_pitch, B, H, g.c)) return e;
  S2P_REQUIRE(z0_pitch >= CH_Z && act_pitch >= A, "%s: a pitch is below its row (z0 288, act A)", who);
  if (int e = chain_check_src(who, "z0", z0, z0_pitch)) return e;
  S2P_REQUIRE(wc_row >= kp && wc_row % 4 == 0 && wb_row >= kp && wb_row % 4 == 0,
              "%s: wc_row and wb_row must be multiples of 4 floats and at least A padded to 4", who);
  S2P_REQUIRE(s2p_al16(wc) && s2p_al16(wb), "%s: wc and wb must be 16-byte aligned", who);
  if (int e = chain_take_mlps(who, mlps, CH_PRIOR_HEADS, 2, g.c)) return e;
  if (int e = chain_check_policy(who, *policy)) return e;
  g.p = *policy; g.z0 = z0; g.z0_pitch = z0_pitch; g.wc = wc; g.wc_row = wc_row; g.wb = wb; g.wb_row = wb_row; g.A = A; g.act = act;
  g.act_pitch = act_pitch;
  return 0;
}

// every buffer of `n` is given and 16-byte aligned
inline bool chain_bufs_ok(float* const* p, int n) {
  for (int i = 0; i < n; ++i)
    if (!p[i] || !s2p_al16(p[i])) return false;
  return true;
}

// The state buffers of the save forms of the posterior chain (fp32 and bf16 compute): the six of t = 0 and, with T > 1, the chain's seven
inline int chain_check_state(const char* who, const s2p_chain_state* state, int T) {
  S2P_REQUIRE(state, "%s: null pointer (state is required)", who);
  float* const bufs[13] = {state->a0_h1, state->a0_h2, state->a0_raw, state->b0_h1, state->b0_h2, state->b0_raw, state->h1a,
                           state->h2a, state->rawa, state->h1b, state->h2b, state->rawb, state->xz};
  S2P_REQUIRE(chain_bufs_ok(bufs, T > 1 ? 13 : 6), "%s: state: a buffer is NULL or not 16-byte aligned", who);
  return 0;
}

// The operand checks of the posterior chain's backward, for both compute modes (Mlp: s2p_chain_mlp_bwd or s2p_chain_mlp_bwd_bf16).
// 0 with `a` filled, or S2P_REQUIRE's value with the error text set.
template <typename Mlp, typename Args>
int posterior_bwd_take(const char* who, const float* eps, int eps_pitch, const float* dmean, int dmean_pitch, const float* dstd,
                       int dstd_pitch, const float* dz, int dz_pitch, const Mlp* mlps, const s2p_chain_state* state,
                       const s2p_chain_grads* grads, int B, int T, Args& a) {
  S2P_REQUIRE(eps && dmean && dstd && dz && mlps && state && grads,
              "%s: null pointer (eps, dmean, dstd, dz, mlps, state and grads are required)", who);
  S2P_REQUIRE(eps_pitch >= CH_Z && dz_pitch >= CH_Z && dmean_pitch >= CH_Z1 && dstd_pitch >= CH_Z1,
              "%s: a pitch is below its row (eps 288, dz 288, dmean 32, dstd 32)", who);
  if (int e = chain_take_mlps(who, mlps, CH_POSTERIOR_HEADS + 2, 2, a)) return e;
  float* const sb[6] = {state->h1a, state->h2a, state->rawa, state->h1b, state->h2b, state->rawb};
  S2P_REQUIRE(chain_bufs_ok(sb, 6), "%s: state: a chain buffer is NULL or not 16-byte aligned", who);
  float* const gb[7] = {grads->drawa, grads->dh2a, grads->dh1a, grads->drawb, grads->dh2b, grads->dh1b, grads->dxz};
  S2P_REQUIRE(chain_bufs_ok(gb, 7), "%s: grads: a buffer is NULL or not 16-byte aligned", who);
  a.eps = eps; a.eps_pitch = eps_pitch; a.dmean = dmean; a.dmean_pitch = dmean_pitch; a.dstd = dstd; a.dstd_pitch = dstd_pitch; a.dz = dz;
  a.dz_pitch = dz_pitch; a.B = B; a.T = T; a.s = *state; a.g = *grads;
  return 0;
}

// The sizes of a call: a negative one is refused (< 0); B == 0 or T < tmin is a no-op (0); else 1.
int chain_sizes(const char* who, int B, int T, int tmin = 1) {
  S2P_REQUIRE(B >= 0 && T >= 0, "%s: negative size", who);
  return B == 0 || T < tmin ? 0 : 1;
}

// One workgroup of CH_THREADS per 16 batch rows.  0, or S2P_CHECK_LAUNCH's value with the error text set.
template <typename Kernel, typename... A>
int chain_launch(const char* name, Kernel kernel, int B, void* stream, const A&... args) {
  hipLaunchKernelGGL(kernel, dim3(cdiv(B, CH_ROWS)), dim3(CH_THREADS), 0, (hipStream_t)stream, args...);
  S2P_CHECK_LAUNCH(name);
  return 0;
}
}  // namespace
