// Padded-raster weight gradient of the PatchGAN 4x4 convolutions (round 4): stride 2 (64 -> 128, 128 -> 256 on both scales) and
// stride 1 / pad 2 (256 -> 512).
//
//   dW[a][t][b] += sum over positions (n, r, c) of the A grid:  A[n, r, c][a] * B[n, s*r + dy_t, s*c + dx_t][b]
//   (conv: A = dY, B = X;  transposed conv: A = X, B = dY -- the same sum, see wgrad_igemm.hip)
//
// Why: in the implicit GEMM (wgrad_dma_kernel) a 128 x 128 output tile is ONE tap x 128 channels, so every tap re-streams its own
// gathered copy of B and every tile re-streams A: the 90-GFLOP 256 -> 512 layer runs at 540 TFLOP/s.  wgrad_slab.hip removes that
// for stride-1 3x3 convs with a padded raster on which a tap is a row shift of ONE resident window.  This file is the same kernel
// with the three things the 4x4 layers need:
//   * STRIDE 2 as parity classes.  dy_t = 2*a_t + py_t: tap t reads the parity sub-plane (py, px) of B at the stride-1 shift
//     (a_t, b_t).  The taps of one parity form a TILE CLASS: its workgroups stage the window of that sub-plane (the space-to-depth
//     is done by the LDS-DMA's per-lane source address: pixel (2r + py, 2c + px)) and keep one accumulator tile per tap of the
//     class -- four classes of 4 taps for 4x4 stride 2.  The 16 taps of a 4x4 stride-1 conv are two classes of 8 (ky < 2, ky >= 2).
//   * A and B live on DIFFERENT grids (13x13 against 12x12 for the pad-2 layer; 22x22 against the parity planes of 43x43): the
//     common raster is Hp x Wp with Hp = max(Ha + amax, Hsub - amin) (Wp likewise), every shifted read that leaves B's grid lands on
//     a position where B's DMA returns zeros, every pad position of A contributes 0.
//   * The tap count of a workgroup is a run-time property of its class (the body is instantiated for 4 and 8 taps and selected by
//     a wave-uniform branch).  Partial tiles go to a slab with plain stores, a second kernel adds them in a fixed order: no atomics.
// Staging, swizzle, fragment reads (`ds_read_b64_tr_b16`), the 3-stage LDS-DMA pipeline with counted vmcnt and the slab stores are
// wgrad_slab_core.h, shared with wgrad_slab.hip.  This file: the class table, workgroup -> (class, tile, split), the run-time
// tap-count dispatch, the 4-segment reduce and the plan.
// The 3x3 stride-2 convs of the encoder / decoder (classes of 4 / 2 / 2 / 1 taps) were measured on this kernel too: 47-53 us against
// 45-48 us on the implicit GEMM -- a stride-2 gather touches a quarter of B per tap, so there the re-streaming is cheap and the
// short-tap classes are bound by the L2 -> LDS bytes of their windows; they stay on wgrad_dma_kernel.
#include "wgrad_slab_core.h"

constexpr int SG_MAX_CLS = 4, SG_MAX_T = 8;
struct WgSlabGArgs {
  const void* A; const void* B; float* dW; float* db;
  float* slab; float* slabb;
  WgsRaster g;                                   // (py, px: per class, below)
  int co_tiles, tiles_per_cls;                   // Ca / 64, (Ca / 64) * (Cb / 64)
  int dw_row, Cb;                                // floats per dW row (taps * Cb)
  int ncls;
  int cls_T[SG_MAX_CLS], cls_py[SG_MAX_CLS], cls_px[SG_MAX_CLS], cls_hneg[SG_MAX_CLS];
  int cls_S[SG_MAX_CLS], cls_bps[SG_MAX_CLS];    // K splits of the class, raster blocks per split
  int cls_wg0[SG_MAX_CLS + 1];                   // first workgroup of the class (cumulative)
  int cls_red0[SG_MAX_CLS + 1];                  // first workgroup of the class in the reduce launch (tiles_per_cls * T each)
  long long cls_slab0[SG_MAX_CLS];               // first float of the class's partial tiles in `slab`
  int toff[SG_MAX_CLS][SG_MAX_T];                // raster offset a_t * Wp + b_t
  int wt[SG_MAX_CLS][SG_MAX_T];                  // tap index in dW
  int nblocks, total_wgs;
  int tbl;                                       // DMA offsets from the tabulated padded raster (wgrad_slab_core.h)
};

// one (tile, split) of a class of T taps: its partial tile [64 A rows][T][64 B channels] into the slab
template <int T, int NXI, bool TBL>
__device__ __forceinline__ void sg_body(const WgSlabGArgs& a, char* lds_all, const int cls, const int tile, const int split) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int co_t = tile % a.co_tiles, ci_s = tile / a.co_tiles;
  const int bps = a.cls_bps[cls];
  const int b0 = split * bps;
  int b1 = b0 + bps; if (b1 > a.nblocks) b1 = a.nblocks;
  const int nblk = b1 - b0;                                   // >= 1 by construction
  const bool do_bias = a.db != nullptr && cls == 0 && ci_s == 0 && (wave & 1) == 0;         // wave-uniform
  WgsRaster g = a.g;
  g.py = a.cls_py[cls]; g.px = a.cls_px[cls];

  f32x16 acc[T];
  f32x16 accb;
  wgs_accumulate<T, NXI, TBL>(g, a.A, a.B, a.toff[cls], a.cls_hneg[cls], co_t, ci_s, b0, nblk, do_bias,
                              lds_all + WGS_TBL_BYTES, (unsigned*)lds_all, acc, accb);

  const int S = a.cls_S[cls];
  wgs_store_slab<T>(a.slab + a.cls_slab0[cls] + ((size_t)tile * S + split) * (64 * T * 64), a.slabb + ((size_t)co_t * S + split) * 64,
                    acc, accb, do_bias);
}

template <int NXI>
__global__ __launch_bounds__(256, 2) void wgrad_slabg_kernel(const WgSlabGArgs a) {
  // the two offset tables at LDS address 0 (also where a launch does not use them), the stages behind them
  __shared__ __attribute__((aligned(1024))) char lds_all[WGS_TBL_BYTES + WGS_NST * wgs_stage_bytes(NXI)];
  // class-major, split-major inside a class: the tiles of one (class, split) stream the same A / B rows
  const int f = wgs_xcd_spread(blockIdx.x, a.total_wgs);
  int cls = 0;
#pragma unroll
  for (int c = 1; c < SG_MAX_CLS; ++c) cls += (c < a.ncls && f >= a.cls_wg0[c]) ? 1 : 0;
  cls = __builtin_amdgcn_readfirstlane(cls);
  const int rem = f - a.cls_wg0[cls];
  const int split = rem / a.tiles_per_cls, tile = rem - split * a.tiles_per_cls;
  const int T = a.cls_T[cls];
  if (a.tbl) {
    if (T == 8) sg_body<8, NXI, true>(a, lds_all, cls, tile, split);
#ifdef S2P_DIAG_BUILD
    else if (T == 2) sg_body<2, NXI, true>(a, lds_all, cls, tile, split);
    else if (T == 1) sg_body<1, NXI, true>(a, lds_all, cls, tile, split);
#endif
    else sg_body<4, NXI, true>(a, lds_all, cls, tile, split);
    return;
  }
  if (T == 8) sg_body<8, NXI, false>(a, lds_all, cls, tile, split);
#ifdef S2P_DIAG_BUILD
  else if (T == 2) sg_body<2, NXI, false>(a, lds_all, cls, tile, split);
  else if (T == 1) sg_body<1, NXI, false>(a, lds_all, cls, tile, split);
#endif
  else sg_body<4, NXI, false>(a, lds_all, cls, tile, split);
}

// dW[tile] += sum over the S partial tiles of the class, in a fixed order (bitwise reproducible).  These layers have few tiles and
// many splits (8 tiles x 64 splits for the 64 -> 128 convs), so the reduce is spread as well: one workgroup per (class, tile, tap,
// group of 4 rows) = 64 float4 outputs, each summed by FOUR threads (a quarter of the splits each, eight loads in flight) whose
// partial sums are combined in segment order.
__global__ __launch_bounds__(256) void wgrad_slabg_reduce_kernel(const WgSlabGArgs a) {
  __shared__ f32x4 red[4][64];
  __shared__ float redb[4][64];
  const int blk = blockIdx.x >> 4, rq = blockIdx.x & 15;
  int cls = 0;
#pragma unroll
  for (int c = 1; c < SG_MAX_CLS; ++c) cls += (c < a.ncls && blk >= a.cls_red0[c]) ? 1 : 0;
  const int T = a.cls_T[cls], S = a.cls_S[cls];
  const int rem = blk - a.cls_red0[cls];
  const int tile = rem / T, t = rem - tile * T;
  const int co_t = tile % a.co_tiles, ci_s = tile / a.co_tiles;
  const size_t chunk = (size_t)64 * T * 64;
  const float* sl = a.slab + a.cls_slab0[cls] + (size_t)tile * S * chunk;
  const int seg = threadIdx.x >> 6, j = threadIdx.x & 63;
  const int per = (S + 3) >> 2, k0 = seg * per, k1 = k0 + per < S ? k0 + per : S;
  const int qd = j & 15, row = rq * 4 + (j >> 4);
  const size_t so = ((size_t)(row * T + t) * 16 + qd) * 4;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  int k = k0;
  for (; k + 8 <= k1; k += 8) {
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = *(const f32x4*)(sl + (size_t)(k + u) * chunk + so);
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; k < k1; ++k) s += *(const f32x4*)(sl + (size_t)k * chunk + so);
  red[seg][j] = s;
  const bool bias = cls == 0 && t == 0 && rq == 0 && ci_s == 0 && a.db != nullptr;          // workgroup-uniform
  if (bias) {
    const float* sb = a.slabb + (size_t)co_t * S * 64;
    float b = 0.f;
    for (int kk = k0; kk < k1; ++kk) b += sb[kk * 64 + j];
    redb[seg][j] = b;
  }
  __syncthreads();
  if (seg == 0) {
    const f32x4 tot = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
    float* o = a.dW + (size_t)(co_t * 64 + row) * a.dw_row + a.wt[cls][t] * a.Cb + ci_s * 64 + qd * 4;
    *(f32x4*)o = *(const f32x4*)o + tot;
    if (bias) a.db[co_t * 64 + j] += ((redb[0][j] + redb[1][j]) + redb[2][j]) + redb[3][j];
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// fills everything but the pointers; false: the layer is outside this kernel's scope.  `nxi` = window rows / 32 (3 or 4)
static bool sg_plan(const s2p_conv_desc* d, int cin_real, int cout_real, WgSlabGArgs& a, int& nxi, size_t& ws_floats) {
  if (!d || d->dtype != S2P_BF16 || d->reflect || d->groups != 1 || d->KH != d->KW) return false;
  if (d->Cin % 64 || d->Cout % 64 || cin_real != d->Cin || cout_real != d->Cout) return false;
  const int K = d->KH, s = d->stride, pad = d->pad;
  const bool k4 = K == 4 && pad == 2 && (s == 2 || (s == 1 && !d->transposed));
  const bool k3 = K == 3 && pad == 1 && s == 2 && S2P_DIAG_SWITCH(6);      // diagnostics build only: the encoder / decoder convs
  if (!k4 && !k3) return false;
  int Ca, Cb;
  WgsRaster& g = a.g;
  if (!d->transposed) { g.Ha = d->Ho; g.Wa = d->Wo; g.Hb = d->H; g.Wb = d->W; Ca = d->Cout; Cb = d->Cin; g.a_pitch = d->y_pitch; g.b_pitch = d->x_pitch; }
  else { g.Ha = d->H; g.Wa = d->W; g.Hb = d->Ho; g.Wb = d->Wo; Ca = d->Cin; Cb = d->Cout; g.a_pitch = d->x_pitch; g.b_pitch = d->y_pitch; }
  g.N = d->N; g.bs = s; a.Cb = Cb; a.dw_row = K * K * Cb;
  a.co_tiles = Ca / 64; a.tiles_per_cls = a.co_tiles * (Cb / 64);
  // taps -> (class, stride-1 shift)
  int ta[16], tb[16], tc[16];
  int amin = 0, amax = 0, bmin = 0, bmax = 0;
  for (int ky = 0; ky < K; ++ky)
    for (int kx = 0; kx < K; ++kx) {
      const int t = ky * K + kx, dy = ky - pad, dx = kx - pad;
      if (s == 2) {
        const int py = dy & 1, px = dx & 1;
        ta[t] = (dy - py) >> 1; tb[t] = (dx - px) >> 1; tc[t] = py * 2 + px;
      } else { ta[t] = dy; tb[t] = dx; tc[t] = ky >> 1; }
      amin = ta[t] < amin ? ta[t] : amin; amax = ta[t] > amax ? ta[t] : amax;
      bmin = tb[t] < bmin ? tb[t] : bmin; bmax = tb[t] > bmax ? tb[t] : bmax;
    }
  const int Hsub = s == 2 ? (g.Hb + 1) / 2 : g.Hb, Wsub = s == 2 ? (g.Wb + 1) / 2 : g.Wb;
  g.Hp = g.Ha + amax > Hsub - amin ? g.Ha + amax : Hsub - amin;
  g.Wp = g.Wa + bmax > Wsub - bmin ? g.Wa + bmax : Wsub - bmin;
  bool tbl;
  if (!wgs_limits(g, tbl)) return false;
  a.tbl = tbl ? 1 : 0;
  a.nblocks = cdiv((long long)g.N * g.Hp * g.Wp, 64);
  // classes in order of decreasing tap count (the long workgroups start first)
  const int ncand = s == 2 ? 4 : 2;
  int order[4] = {0, 1, 2, 3}, cnt[4] = {0, 0, 0, 0};
  for (int t = 0; t < K * K; ++t) ++cnt[tc[t]];
  for (int i = 0; i < ncand; ++i)
    for (int j = i + 1; j < ncand; ++j)
      if (cnt[order[j]] > cnt[order[i]]) { int o = order[i]; order[i] = order[j]; order[j] = o; }
  a.ncls = 0;
  int span = 0;
  for (int i = 0; i < ncand; ++i) {
    const int c = order[i];
    if (!cnt[c]) continue;
    if (cnt[c] != 4 && cnt[c] != 8 && !(k3 && (cnt[c] == 1 || cnt[c] == 2))) return false;
    const int k = a.ncls++;
    a.cls_T[k] = cnt[c]; a.cls_py[k] = s == 2 ? c >> 1 : 0; a.cls_px[k] = s == 2 ? c & 1 : 0;
    int lo = 0, hi = 0, n = 0;
    for (int t = 0; t < K * K; ++t)
      if (tc[t] == c) {
        const int off = ta[t] * g.Wp + tb[t];
        a.toff[k][n] = off; a.wt[k][n] = t; ++n;
        lo = off < lo ? off : lo; hi = off > hi ? off : hi;
      }
    a.cls_hneg[k] = -lo;
    span = 64 + hi - lo > span ? 64 + hi - lo : span;
  }
  if (span > 128) return false;
  nxi = span <= 96 ? 3 : 4;
  // K splits: ~2 workgroups per CU in total, the same number for every class (a block costs a class of 4 taps as much as one of
  // 8: these launches are bound by the DMA round trips of a block, not by its MFMAs)
  const double unit = (S2P_DIAG_SWITCH(16) ? 1.0 : 2.0) * s2p_num_cus() / ((double)a.tiles_per_cls * a.ncls);
  int wg = 0, red = 0;
  size_t fl = 0;
  for (int k = 0; k < a.ncls; ++k) {
    int S = (int)(unit + 0.5);
    if (S > 128) S = 128;
    if (S > a.nblocks) S = a.nblocks;
    if (S < 1) S = 1;
    a.cls_bps[k] = cdiv(a.nblocks, S);
    a.cls_S[k] = cdiv(a.nblocks, a.cls_bps[k]);
    a.cls_wg0[k] = wg; wg += a.tiles_per_cls * a.cls_S[k];
    a.cls_red0[k] = red; red += a.tiles_per_cls * a.cls_T[k];
    a.cls_slab0[k] = (long long)fl; fl += (size_t)a.tiles_per_cls * a.cls_S[k] * 64 * a.cls_T[k] * 64;
  }
  for (int k = a.ncls; k <= SG_MAX_CLS; ++k) { a.cls_wg0[k] = wg; a.cls_red0[k] = red; }
  a.total_wgs = wg;
  ws_floats = fl + (size_t)a.co_tiles * a.cls_S[0] * 64;        // + the bias partials of class 0
  return true;
}

bool s2p_wgrad_slabg_supported(const s2p_conv_desc* d, int cin_real, int cout_real) {
  if (S2P_DIAG_SWITCH(5)) return false;
  WgSlabGArgs a{}; int nxi; size_t fl;
  return sg_plan(d, cin_real, cout_real, a, nxi, fl);
}

size_t s2p_wgrad_slabg_workspace(const s2p_conv_desc* d, int cin_real, int cout_real) {
  WgSlabGArgs a{}; int nxi; size_t fl;
  if (!sg_plan(d, cin_real, cout_real, a, nxi, fl)) return 0;
  return fl * sizeof(float);
}

int s2p_wgrad_slabg(const s2p_conv_desc* d, const void* x, const void* dy, float* dw, float* db, int cin_real, int cout_real,
                    void* workspace, size_t workspace_bytes, hipStream_t st) {
  WgSlabGArgs a{}; int nxi; size_t fl;
  if (!sg_plan(d, cin_real, cout_real, a, nxi, fl)) S2P_FAIL(-2, "s2p_wgrad_slabg: unsupported geometry");
  if (!workspace || workspace_bytes < fl * sizeof(float))
    S2P_FAIL(-1, "s2p_wgrad_slabg: workspace of %zu bytes needed, got %zu", fl * sizeof(float), workspace_bytes);
  a.A = d->transposed ? x : dy; a.B = d->transposed ? dy : x;
  a.dW = dw; a.db = db;
  a.slab = (float*)workspace;
  a.slabb = a.slab + (fl - (size_t)a.co_tiles * a.cls_S[0] * 64);
  if (nxi == 3) hipLaunchKernelGGL(wgrad_slabg_kernel<3>, dim3(a.total_wgs), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(wgrad_slabg_kernel<4>, dim3(a.total_wgs), dim3(256), 0, st, a);
  S2P_CHECK_LAUNCH("wgrad_slabg_kernel");
  hipLaunchKernelGGL(wgrad_slabg_reduce_kernel, dim3(a.cls_red0[a.ncls] * 16), dim3(256), 0, st, a);
  S2P_CHECK_LAUNCH("wgrad_slabg_reduce_kernel");
  return 0;
}
