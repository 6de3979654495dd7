// What the plane-resident conv kernels share BEHIND their K loops (conv_plane.hip: conv_plane_kernel, conv_plane_pair_kernel;
// conv_planeg.hip: conv_planeg_kernel), bf16: the accumulator exchange of a wave pair, bias + activation + [pixel][co] staging, the
// conv's own residual / producer-activation-gradient epilogue, and the fused InstanceNorm + MAT-modulation tails (forward, backward)
// of the plane a workgroup owns.  The single copy: the K loops, their DMA schedules and the LDS maps stay in the kernels' files.
// Everything here is __forceinline__ and is called behind the loop only (a helper inside the K loop changes its register allocation).
#pragma once
#include "s2p_common.h"
#include "conv_plane.h"
#include "norm_stats.h"

typedef Chunk<__bf16> PeChunk;
constexpr int PE_ERS = 144;                  // epilogue staging row: 64 co x 2 B + 16

// ---- staging rows: address of pixel px's 16-byte chunk c (8 channels).  The one thing that differs between the callers ------------
struct PeRows144 {                           // 144-byte rows (the pair kernel: base = its wave set's rows)
  char* base;
  __device__ __forceinline__ char* operator()(int px, int c) const { return base + px * PE_ERS + c * 16; }
};
struct PeRowsSwz128 {                        // 128-byte rows, the chunk index XOR px & 7 (the gamma|beta-staging form of conv_plane.hip)
  char* base;
  __device__ __forceinline__ char* operator()(int px, int c) const { return base + px * 128 + ((c ^ (px & 7)) << 4); }
};

// ---- add the two partial accumulators of a wave pair through LDS: the pair exchanges halves (set 0, IB = 0, ends up with the sums
//      of co blocks 0-1, set 1, IB = 2, with co blocks 2-3), so all eight waves share the epilogue.  One round; xbase: 4 * 4 PB KB ------
template <int PB, int IB>
__device__ __forceinline__ void pe_exchange(f32x4 (&acc)[4][PB], char* xbase, int wq, int lane) {
  char* mb = xbase + (size_t)(wq * 4 * PB) * 1024 + lane * 16;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < PB; ++j) *(f32x4*)(mb + ((2 - IB + i) * PB + j) * 1024) = acc[2 - IB + i][j];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < PB; ++j) acc[IB + i][j] += *(const f32x4*)(mb + ((IB + i) * PB + j) * 1024);
  __syncthreads();                                              // the staging rows overlap the exchange area
}

// ---- bias + activation in registers, then [pixel][co] staging rows (transpose through LDS): co blocks IB .. IB + NB - 1 of this
//      wave's tiles.  bias: the slab's 64 values or NULL ----------------------------------------------------------------------------
template <int PB, int NB, int IB, typename Rows>
__device__ __forceinline__ void pe_stage_out(const f32x4 (&acc)[4][PB], const float* bias, int act, float slope, int wq, int q, int l15,
                                             Rows srow) {
  float bv[NB][4];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) bv[i][e] = bias ? bias[16 * (IB + i) + 4 * q + e] : 0.f;
  // the activation selector is resolved ONCE (a uniform branch around the whole pass), never per element
  auto pass = [&](auto f) {
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int j = 0; j < PB; ++j) {
        const int px = (wq * PB + j) * 16 + l15;
        const f32x4 v = acc[IB + i][j];
        bf16x4 o = {(__bf16)f(v[0] + bv[i][0]), (__bf16)f(v[1] + bv[i][1]), (__bf16)f(v[2] + bv[i][2]), (__bf16)f(v[3] + bv[i][3])};
        *(bf16x4*)(srow(px, 2 * (IB + i) + (q >> 1)) + (q & 1) * 8) = o;
      }
  };
  if (act == S2P_ACT_TANH) pass([](float v) { return tanhf(v); });
  else if (act == S2P_ACT_SWISH) pass([](float v) { return v / (1.f + expf(-v)); });
  else if (act == S2P_ACT_NONE) pass([](float v) { return v; });                 // (dgrads, gamma/beta conv: the pass is VALU-bound)
  else {
    const float ns = act == S2P_ACT_RELU ? 0.f : slope;                          // relu / lrelu
    pass([ns](float v) { return lrelu_ns(v, ns); });
  }
}

// ---- one (pixel row, 8-channel chunk) item of the output: staged value (+ residual / producer-activation-gradient epilogue) -------
struct PeOut {                               // the conv's own epilogue, resolved once per thread; goff: the group's offset in y / aux
  const __bf16* aux; const __bf16* aux2; int epi; bool add, g_tanh; float gneg;
  __device__ __forceinline__ PeOut(const void* aux_, const void* aux2_, size_t goff, int epi_, int gact, float gslope)
      : aux(aux_ ? (const __bf16*)aux_ + goff : nullptr), aux2(aux2_ ? (const __bf16*)aux2_ + goff : nullptr), epi(epi_),
        add(epi_ == S2P_EPI_ADD), g_tanh(gact == S2P_ACT_TANH),
        gneg(gact == S2P_ACT_RELU ? 0.f : (gact == S2P_ACT_LRELU ? gslope : 1.f)) {}
};
template <typename Rows>
__device__ __forceinline__ PeChunk pe_out_chunk(const PeOut& o, Rows srow, int row, int ch, size_t go, const PeChunk* pre = nullptr) {   // pre: aux chunk already in registers
  PeChunk c;
  c.raw = *(const u32x4*)srow(row, ch);
  if (o.epi != S2P_EPI_STORE) {
    PeChunk x, x2;
    if (pre) x = *pre; else x.raw = *(const u32x4*)(o.aux + go);
    x2.raw = (u32x4){0u, 0u, 0u, 0u};
    if (o.aux2) x2.raw = *(const u32x4*)(o.aux2 + go);
    float ov[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = c.get(e), xv = x.get(e);
      const float f = o.g_tanh ? 1.f - xv * xv : (xv > 0.f ? 1.f : o.gneg);
      ov[e] = o.add ? v + xv : (v + x2.get(e)) * f;
    }
    c.pack(ov);
  }
  return c;
}

// ---- the fused norm tails ------------------------------------------------------------------------------------------------------
// Thread (row lane r0 = tid >> 3, chunk ch = tid & 7) holds the rows r0, r0 + 64, ... (MAXR row groups) of its 8 channels.
struct PeTail {
  int tid, lane, wave;
  int img, co_base, Cout, HW;                // image, first channel of the 64-channel slab, the norm's channels, pixels of the plane
  size_t pix0;                               // index of the plane's first pixel in the produced tensor (img * HW where the plane is the image)
  char* scratch;                             // LDS, free once the staging rows are dead: 9.5 KB in the backward form, 3 KB in the forward
  __bf16* y; int y_pitch;                    // forward: the conv output (NULL: not stored)
  const PlaneNorm* n;
};

// gamma|beta source policies.  fetch(): request row group k's chunks (top of the tail); get(): the chunks where they are used;
// aux() / xn(): the conv epilogue's residual chunk and the norm input of row group k.
struct PeGbNone {                            // plain InstanceNorm: compile-time zeros, no registers
  __device__ __forceinline__ void fetch(int, int, const __bf16*, const PeTail&) {}
  __device__ __forceinline__ void get(int, PeChunk& gk, PeChunk& bk) const { gk.raw = (u32x4){0u, 0u, 0u, 0u}; bk.raw = gk.raw; }
  __device__ __forceinline__ const PeChunk* aux(int) const { return nullptr; }
  __device__ __forceinline__ PeChunk xn(int, int row, const __bf16* xb, const PeTail& t) const {
    PeChunk x; x.raw = (u32x4){0u, 0u, 0u, 0u};
    if (row < t.HW) x.raw = *(const u32x4*)(xb + (size_t)row * t.n->xn_pitch);
    return x;
  }
};
template <int MAXR> struct PeGbGlobal : PeGbNone {      // maps in HBM (gbb may be NULL): chunks loaded into registers at the top of the tail
  PeChunk gv[MAXR], bv[MAXR];
  __device__ __forceinline__ void fetch(int k, int row, const __bf16* gbb, const PeTail& t) {
    gv[k].raw = (u32x4){0u, 0u, 0u, 0u}; bv[k].raw = gv[k].raw;
    if (gbb && row < t.HW) {
      gv[k].raw = *(const u32x4*)(gbb + (size_t)row * t.n->gb_pitch);
      bv[k].raw = *(const u32x4*)(gbb + (size_t)row * t.n->gb_pitch + t.Cout);
    }
  }
  __device__ __forceinline__ void get(int k, PeChunk& gk, PeChunk& bk) const { gk = gv[k]; bk = bv[k]; }
};
// Maps staged in LDS under the K loop (conv_plane.hip, GST).  Row groups k < KG0 come from the LDS rows: a row is 256 B, rows below
// ROWS_B lie at smem + GB_B, the others from smem on; gamma sits at ((r0 & 1) << 7) + 16 ch, beta at that address ^ 128, and row
// r0 + 64 k keeps r0's parity.  A masked row reads some other row: its operand is zero, so the value does not matter.
// The last row group's gamma | beta, xn and aux come from registers that the kernel requested right behind the loop.
template <int KG0, int GB_B, int ROWS_B> struct PeGbStaged {
  const char* smem; int tid;
  const PeChunk *pre_g, *pre_b, *pre_x, *pre_a;
  __device__ __forceinline__ void fetch(int, int, const __bf16*, const PeTail&) {}
  __device__ __forceinline__ int gst_row(int k) const {
    const int r0 = tid >> 3, ch = tid & 7, row = r0 + 64 * k;
    return (row < ROWS_B ? GB_B + row * 256 : (row - ROWS_B) * 256) + ((r0 & 1) << 7) + ch * 16;
  }
  __device__ __forceinline__ void get(int k, PeChunk& gk, PeChunk& bk) const {
    if (k < KG0) { const int go = gst_row(k); gk.raw = *(const u32x4*)(smem + go); bk.raw = *(const u32x4*)(smem + (go ^ 128)); }
    else { gk = pre_g[k < KG0 ? 0 : k - KG0]; bk = pre_b[k < KG0 ? 0 : k - KG0]; }
  }
  __device__ __forceinline__ const PeChunk* aux(int k) const { return &pre_a[k]; }
  __device__ __forceinline__ PeChunk xn(int k, int, const __bf16*, const PeTail&) const { return pre_x[k]; }
};

// ---- fused InstanceNorm + MAT modulation + activation (norm.hip: in_fused_fwd_kernel) on the plane this workgroup owns ------------
// The conv output (as stored: bf16) stays in registers, the statistics are the exact two-pass ones (mean, then centred second
// moment), summed in a fixed order (lanes, then waves, then the 8-wave column sum), and the modulated tensor is written from the same
// registers.  KFULL: row groups that exist in every thread -- no bounds select on their squares (an explicit fma there).
template <int MAXR, int KFULL, typename Gb, typename Rows>
__device__ __forceinline__ void pe_norm_fwd(const PeTail& t, const PeOut& eo, Rows srow, Gb& gb) {
  typedef __bf16 T;
  const PlaneNorm& n = *t.n;
  const int tid = t.tid, lane = t.lane, wave = t.wave, HW = t.HW, co_base = t.co_base;
  const int ch = tid & 7, r0 = tid >> 3;
  const T* gbb = n.gb ? (const T*)n.gb + t.pix0 * n.gb_pitch + co_base + ch * 8 : nullptr;
#pragma unroll
  for (int k = 0; k < MAXR; ++k) gb.fetch(k, r0 + 64 * k, gbb, t);      // gamma / beta first: their latency runs under the rest
  // The plane stays in registers UNPACKED from here on (8 MAXR floats: the accumulators are dead): round 4 kept it packed and paid
  // three unpack passes; with the centred values kept from the second pass, the maximum form of the activation and paired
  // bf16 conversions the tail is ~330 VALU instructions per wave shorter (of 1 320)
  float xf[MAXR][8];
#pragma unroll
  for (int k = 0; k < MAXR; ++k) {
    const int row = r0 + 64 * k;
    PeChunk xv;
    xv.raw = (u32x4){0u, 0u, 0u, 0u};
    if (row < HW) {
      const size_t go = (t.pix0 + row) * t.y_pitch + co_base + ch * 8;
      xv = pe_out_chunk(eo, srow, row, ch, go, gb.aux(k));
      if (t.y) *(u32x4*)(t.y + go) = xv.raw;                    // (y == NULL: the caller keeps only the modulated tensor -- a forward without a backward)
    }
    xv.unpack(xf[k]);                                           // rows beyond HW hold zeros
  }
  __syncthreads();                                              // the staging rows are dead: LDS is scratch from here on
  float* red = (float*)t.scratch;                               // [8 waves][64]
  float* cst = red + 8 * 64;                                    // [4][64]: plane sum / M2, then 1 + gamma_st, beta_st
  auto plane_sum = [&](float (&v)[8], int slot) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
#pragma unroll
      for (int o = 8; o < 64; o <<= 1) v[e] += __shfl_xor(v[e], o, 64);
    }
    __syncthreads();
    if (lane < 8) {
#pragma unroll
      for (int e = 0; e < 8; ++e) red[wave * 64 + lane * 8 + e] = v[e];
    }
    __syncthreads();
    if (tid < 64) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) s += red[w * 64 + tid];
      cst[slot * 64 + tid] = s;
    }
    __syncthreads();
  };
  const float inv = 1.f / (float)HW;
  float sacc[8], mean[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    sacc[e] = 0.f;
#pragma unroll
    for (int k = 0; k < MAXR; ++k) sacc[e] += xf[k][e];
  }
  plane_sum(sacc, 0);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    mean[e] = cst[ch * 8 + e] * inv;
    sacc[e] = 0.f;
#pragma unroll
    for (int k = 0; k < MAXR; ++k) {
      const float d = xf[k][e] - mean[e];
      xf[k][e] = d;                                             // the centred value is what the last pass needs
      if (k < KFULL) sacc[e] = __builtin_fmaf(d, d, sacc[e]);
      else sacc[e] += (r0 + 64 * k < HW) ? d * d : 0.f;
    }
  }
  plane_sum(sacc, 1);
  if (tid < 64) {
    const int c = co_base + tid;
    float* o = stats_slot(n.stats, t.img, t.Cout, c, 1, 0);    // one split: the plane
    o[0] = cst[tid] * inv; o[1] = cst[64 + tid];
    if (c == 0 && t.img == 0) stats_store_header(n.stats, 1, HW);
    cst[2 * 64 + tid] = n.gbst ? 1.f + n.gbst[(size_t)t.img * n.gbst_pitch + c] : 1.f;
    cst[3 * 64 + tid] = n.gbst ? n.gbst[(size_t)t.img * n.gbst_pitch + t.Cout + c] : 0.f;
  }
  __syncthreads();
  float rstd[8], gs[8], bs[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    rstd[e] = 1.f / sqrtf(cst[64 + ch * 8 + e] * inv + n.eps);
    gs[e] = cst[2 * 64 + ch * 8 + e]; bs[e] = cst[3 * 64 + ch * 8 + e];
  }
  const float nns = n.n_act == S2P_ACT_RELU ? 0.f : (n.n_act == S2P_ACT_LRELU ? n.n_slope : 1.f);   // none / relu / lrelu (host)
  T* y2 = (T*)n.y2 + t.pix0 * n.y2_pitch + co_base + ch * 8;
#pragma unroll
  for (int k = 0; k < MAXR; ++k) {
    const int row = r0 + 64 * k;
    if (row >= HW) break;
    PeChunk o0, gk, bk;
    gb.get(k, gk, bk);
    float ov[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float gg = gs[e] + gk.get(e), bb = bs[e] + bk.get(e);
      float xh;
      ov[e] = lrelu_ns(mat_value_centred(xf[k][e], rstd[e], gg, bb, xh), nns);
    }
    o0.pack(ov);
    *(u32x4*)(y2 + (size_t)row * n.y2_pitch) = o0.raw;
  }
}

// ---- fused backward of InstanceNorm + MAT modulation + activation (norm.hip: in_fused_bwd_kernel) ----------------------------------
// The launch is the dgrad of the conv that CONSUMED the norm's output, so the staged plane is dL/d(norm output) for the (image,
// 64-channel slab) this workgroup owns; it never goes to HBM.  conv_planeg_kernel also adds the aux gradient of EPI_ADD to it (e.g. a
// feature-matching tap); conv_plane_kernel passes an `eo` without an epilogue, as it never read aux in this form.  The thread
// takes the norm INPUT xn, gamma and beta of its rows, forms the four plane sums (lanes, then waves, then the 8-wave column sum:
// fixed order) and writes dL/d(xn) (+ the skip gradient `res`), d(gamma_img | beta_img) and the state-affine gradient.
// FSUM: the three product sums of pass 1 as explicit fma -- what conv_planeg_kernel's own (channels-outermost) loop contracted every
// term to before the tails were shared; false leaves the contraction to the compiler, as conv_plane_kernel always had it (there it
// keeps some products for pass 2 and adds them unfused).  Not the same rounding, hence a parameter and not one form for both.
template <int MAXR, bool FSUM, typename Gb, typename Rows>
__device__ __forceinline__ void pe_norm_bwd(const PeTail& t, const PeOut& eo, Rows srow, Gb& gb) {
  typedef __bf16 T;
  const PlaneNorm& n = *t.n;
  const int tid = t.tid, lane = t.lane, wave = t.wave, HW = t.HW, co_base = t.co_base;
  const int ch = tid & 7, r0 = tid >> 3, lc = co_base + ch * 8;
  const T* xb = (const T*)n.xn + t.pix0 * n.xn_pitch + lc;
  const T* gbb = n.gb ? (const T*)n.gb + t.pix0 * n.gb_pitch + lc : nullptr;
  PeChunk xv[MAXR], dv[MAXR];
#pragma unroll
  for (int k = 0; k < MAXR; ++k) {
    const int row = r0 + 64 * k;
    xv[k] = gb.xn(k, row, xb, t);
    gb.fetch(k, row, gbb, t);
    dv[k].raw = (u32x4){0u, 0u, 0u, 0u};                        // rows beyond HW stay zero: they add nothing to the sums
    if (row < HW) dv[k] = pe_out_chunk(eo, srow, row, ch, (t.pix0 + row) * t.y_pitch + lc);
  }
  __syncthreads();                                              // the staging rows are dead: LDS is scratch from here on
  float* red = (float*)t.scratch;                               // [4 sums][8 waves][64]
  float* cst = red + 4 * 8 * 64;                                // [6][64]: mean, rstd, 1 + gamma_st, beta_st, s1 / HW, s2 / HW
  if (tid < 64) {
    const int c = co_base + tid;
    stats_mean_rstd(n.stats, t.img, t.Cout, c, HW, n.eps, cst[tid], cst[64 + tid]);   // (S = 1 when a fused forward kernel wrote them)
    cst[2 * 64 + tid] = n.gbst ? 1.f + n.gbst[(size_t)t.img * n.gbst_pitch + c] : 1.f;
    cst[3 * 64 + tid] = n.gbst ? n.gbst[(size_t)t.img * n.gbst_pitch + t.Cout + c] : 0.f;
  }
  __syncthreads();
  const float nneg = n.n_act == S2P_ACT_RELU ? 0.f : (n.n_act == S2P_ACT_LRELU ? n.n_slope : 1.f);
  // ---- pass 1: the four plane sums.  Rows outermost (one read of the gamma | beta chunk per row); every sum adds its rows in
  // ascending order.  The normalised input xh and the gradient dy behind the activation stay in registers for pass 2 (16 MAXR floats:
  // the accumulators are dead) -- round 4 recomputed both there from the packed chunks and a 64-bit mask of the activation
  // branches: 40 VALU instructions per element over the two passes, now ~23
  float xhf[MAXR][8], dyf[MAXR][8];
  {
    float mm[8], rr[8], g1[8], b1[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { const int cl = ch * 8 + e; mm[e] = cst[cl]; rr[e] = cst[64 + cl]; g1[e] = cst[128 + cl]; b1[e] = cst[192 + cl]; }
    float q0[8], q1[8], q2[8], q3[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { q0[e] = 0.f; q1[e] = 0.f; q2[e] = 0.f; q3[e] = 0.f; }
#pragma unroll
    for (int k = 0; k < MAXR; ++k) {
      PeChunk gk, bk;
      gb.get(k, gk, bk);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float gg = g1[e] + gk.get(e), bb = b1[e] + bk.get(e);
        float xh;
        const float yv = mat_value(xv[k].get(e), mm[e], rr[e], gg, bb, xh);          // (the forward's rounding)
        const float dvv = dv[k].get(e);
        const float dy = yv > 0.f ? dvv : dvv * nneg;
        const float dxh = dy * gg;
        xhf[k][e] = xh; dyf[k][e] = dy;
        if constexpr (FSUM) { q0[e] = __builtin_fmaf(dy, gg, q0[e]); q1[e] = __builtin_fmaf(dxh, xh, q1[e]); q2[e] = __builtin_fmaf(dy, xh, q2[e]); }
        else { q0[e] += dxh; q1[e] += dxh * xh; q2[e] += dy * xh; }
        q3[e] += dy;
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int cl = ch * 8 + e;
#pragma unroll
      for (int o = 8; o < 64; o <<= 1) {
        q0[e] += __shfl_xor(q0[e], o, 64); q1[e] += __shfl_xor(q1[e], o, 64); q2[e] += __shfl_xor(q2[e], o, 64); q3[e] += __shfl_xor(q3[e], o, 64);
      }
      if (lane < 8) { red[(0 * 8 + wave) * 64 + cl] = q0[e]; red[(1 * 8 + wave) * 64 + cl] = q1[e]; red[(2 * 8 + wave) * 64 + cl] = q2[e]; red[(3 * 8 + wave) * 64 + cl] = q3[e]; }
    }
  }
  __syncthreads();
  if (tid < 64) {
    float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) { t0 += red[(0 * 8 + w) * 64 + tid]; t1 += red[(1 * 8 + w) * 64 + tid]; t2 += red[(2 * 8 + w) * 64 + tid]; t3 += red[(3 * 8 + w) * 64 + tid]; }
    const float inv = 1.f / (float)HW;
    cst[4 * 64 + tid] = t0 * inv; cst[5 * 64 + tid] = t1 * inv;
    const int c = co_base + tid;
    if (n.dgbst) {
      n.dgbst[(size_t)t.img * n.dgbst_pitch + c] = t2;
      n.dgbst[(size_t)t.img * n.dgbst_pitch + t.Cout + c] = t3;
    }
  }
  __syncthreads();
  // ---- pass 2: outputs
  T* dxo = (T*)n.y2 + t.pix0 * n.y2_pitch + lc;
  T* dgo = n.dgb ? (T*)n.dgb + t.pix0 * n.dgb_pitch + lc : nullptr;
  const T* rsb = n.res ? (const T*)n.res + t.pix0 * n.res_pitch + lc : nullptr;
  float rr2[8], g12[8], s1v[8], s2v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { const int cl = ch * 8 + e; rr2[e] = cst[64 + cl]; g12[e] = cst[128 + cl]; s1v[e] = cst[256 + cl]; s2v[e] = cst[320 + cl]; }
#pragma unroll
  for (int k = 0; k < MAXR; ++k) {
    const int row = r0 + 64 * k;
    if (row >= HW) break;
    PeChunk o0, o1, o2, gk, bk;
    gb.get(k, gk, bk);
    float v0[8], v1[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float gg = g12[e] + gk.get(e);
      const float xh = xhf[k][e], dy = dyf[k][e];
      const float dxh = dy * gg;
      v0[e] = rr2[e] * (dxh - s1v[e] - xh * s2v[e]);
      v1[e] = dy * xh;
    }
    if (rsb) {                                                  // skip-connection gradient folded into the store
      PeChunk rv; rv.raw = *(const u32x4*)(rsb + (size_t)row * n.res_pitch);
      // (round 4 rounded dx to bf16 before the add: o0.get(e) + rv.get(e); kept, bit for bit)
      o0.pack(v0);
#pragma unroll
      for (int e = 0; e < 8; ++e) v0[e] = o0.get(e) + rv.get(e);
    }
    o0.pack(v0); o1.pack(v1); o2.pack(dyf[k]);
    *(u32x4*)(dxo + (size_t)row * n.y2_pitch) = o0.raw;
    if (dgo) {
      *(u32x4*)(dgo + (size_t)row * n.dgb_pitch) = o1.raw;
      *(u32x4*)(dgo + (size_t)row * n.dgb_pitch + t.Cout) = o2.raw;
    }
  }
}
