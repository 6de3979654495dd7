// Batched weight gradient of stride-1 "same" convolutions (ResBlk 3x3 convs, the grouped gamma/beta 3x3 convs) on
// gfx950:   dW[co][t][ci] (+)= sum_p dY[p][co] * X[p + (dy_t, dx_t)][ci],   db[co] (+)= sum_p dY[p][co].
//
// Why a second wgrad kernel.  In the generic implicit GEMM (wgrad_igemm.hip) a 128x128 output tile holds ONE tap, so
// every tap re-streams its own shifted copy of X and every tile re-streams dY: 64 FLOP per L2->LDS byte, and the
// 256x2304 output of a ResBlk conv (36 tiles) only fills the chip through split-K 16 with fp32 atomics (16x write
// amplification, run-to-run last-bit noise).  Here
//   * both operands are addressed on a PADDED RASTER: positions k = (n*Hp + r)*Wp + c with Hp = H + pad, Wp = W + pad;
//     pad rows / columns are zero (the LDS-DMA's out-of-range offset returns zeros), so a tap is a pure row shift
//     k -> k + dy*Wp + dx and image borders need no masks (a shifted read that leaves the image lands on a pad
//     position; a pad position of dY contributes 0).  Cost: (Hp*Wp)/(H*W) = 1.10 more MFMA work at 21x21;
//   * a workgroup (4 waves) owns a 64(co) x 9 taps x 64(ci) output tile: one dY stage (64 positions x 64 co) and one X
//     window (64 positions + halo, 64 ci) feed all nine taps -> 214 FLOP per L2->LDS byte, and each wave keeps
//     9 accumulator tiles (32 co x 32 ci per tap) so an A fragment is reused nine times;
//   * several layers (jobs) share one launch: 12 ResBlk convs x 16 tiles x S K-splits fill the chip with S = 2..4
//     instead of 16, partial tiles go to a slab with plain stores and a second tiny kernel adds them up in a fixed
//     order: no atomics, bitwise reproducible, dW written once.
// Staging, swizzle, fragment reads (`ds_read_b64_tr_b16`), the 3-stage LDS-DMA pipeline with counted vmcnt and the slab stores are
// wgrad_slab_core.h, shared with the 4x4 / parity-class kernel (wgrad_slabg.hip).  This file: the multi-job argument block,
// workgroup -> (job, tile, split), the direct-accumulate epilogue of an unsplit launch, the reduce kernel and the entry points.
#include "wgrad_slab_core.h"

constexpr int WS_MAX_JOBS = 16;
struct WgSlabArgs {
  const void* A[WS_MAX_JOBS]; const void* B[WS_MAX_JOBS]; float* dW[WS_MAX_JOBS]; float* db[WS_MAX_JOBS];
  float* slab; float* slabb;
  WgsRaster g;                                   // Ha x Wa = Hb x Wb = H x W, Hp = H + 1, Wp = W + 1
  int Cin;
  int co_tiles, tiles_per_job;
  int S, blocks_per_split, nblocks;
  int halo;
  int toff[9];
  int total_wgs;
};

// WROWS: rows of the X window (64 positions + halo both sides); TBL: DMA offsets from the tabulated raster (wgrad_slab_core.h).
// The tables sit at LDS address 0, the stages behind them; the (n, row, column) variants reserve no table space.
template <int WROWS, bool TBL>
__global__ __launch_bounds__(256, 2) void wgrad_slab_kernel(const WgSlabArgs a) {
  constexpr int T = 9, NXI = WROWS / 32;
  constexpr int TOFF = TBL ? WGS_TBL_BYTES : 0;
  __shared__ __attribute__((aligned(1024))) char lds_all[TOFF + WGS_NST * wgs_stage_bytes(NXI)];
  // job-major: the tiles of one job stream the same dY / X rows
  const int f = wgs_xcd_spread(blockIdx.x, a.total_wgs);
  const int per_job = a.tiles_per_job * a.S;
  const int job = f / per_job;
  const int rem = f - job * per_job;
  const int split = rem / a.tiles_per_job, tile = rem - split * a.tiles_per_job;
  const int co_t = tile % a.co_tiles, ci_s = tile / a.co_tiles;
  const int b0 = split * a.blocks_per_split;
  int b1 = b0 + a.blocks_per_split; if (b1 > a.nblocks) b1 = a.nblocks;
  const int nblk = b1 - b0;                                   // >= 1 by construction
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool do_bias = a.db[job] != nullptr && ci_s == 0 && (wave & 1) == 0;         // wave-uniform
  // one grid for both operands, stride 1, no parity -- as constants, so that the B address is the A address with another pitch
  const WgsRaster g = {a.g.N, a.g.Ha, a.g.Wa, a.g.Ha, a.g.Wa, a.g.Hp, a.g.Wp, 1, 0, 0, a.g.a_pitch, a.g.b_pitch, a.g.a_bytes, a.g.b_bytes};

  f32x16 acc[T];
  f32x16 accb;
  wgs_accumulate<T, NXI, TBL>(g, a.A[job], a.B[job], a.toff, a.halo, co_t, ci_s, b0, nblk, do_bias, lds_all + TOFF,
                              (unsigned*)lds_all, acc, accb);

  const int tile_g = job * a.tiles_per_job + tile;
  if (a.S == 1) {
    // lanes <-> consecutive ci (contiguous floats), registers <-> co rows; wave tile: co [32wa, +32) x ci [32wb, +32) for every tap
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5, wa = wave >> 1, wb = wave & 1;
    float* dW = a.dW[job];
    const int row_len = T * a.Cin;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int co = co_t * 64 + 32 * wa + (e & 3) + 8 * (e >> 2) + 4 * h;
        float* o = dW + (size_t)co * row_len + t * a.Cin + ci_s * 64 + 32 * wb + r;
        *o += acc[t][e];
      }
    if (do_bias && r == 0) {
      float* db = a.db[job];
#pragma unroll
      for (int e = 0; e < 16; ++e) db[co_t * 64 + 32 * wa + (e & 3) + 8 * (e >> 2) + 4 * h] += accb[e];
    }
  } else {
    wgs_store_slab<T>(a.slab + ((size_t)tile_g * a.S + split) * (64 * T * 64), a.slabb + ((size_t)tile_g * a.S + split) * 64, acc, accb, do_bias);
  }
}

// dW[tile] += sum over the S partial tiles, in split order (fixed order: bitwise reproducible).  One workgroup per
// (tile, tap): 64 rows x 64 ci = 1024 float4, four per thread, all S partial loads of a thread in flight together.
__global__ __launch_bounds__(256) void wgrad_slab_reduce_kernel(const WgSlabArgs a) {
  constexpr int T = 9;
  const int tile_g = blockIdx.x / T, t = blockIdx.x - tile_g * T;
  const int job = tile_g / a.tiles_per_job, tile = tile_g - job * a.tiles_per_job;
  const int co_t = tile % a.co_tiles, ci_s = tile / a.co_tiles;
  const float* sl = a.slab + (size_t)tile_g * a.S * (64 * T * 64);
  float* dW = a.dW[job];
  const int row_len = T * a.Cin;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = threadIdx.x + 256 * u;                       // float4 index inside the [64 rows][16 quads] tap plane
    const int qd = i & 15, row = i >> 4;
    const size_t so = ((size_t)(row * T + t) * 16 + qd) * 4;
    f32x4 s = *(const f32x4*)(sl + so);
    for (int k = 1; k < a.S; ++k) s += *(const f32x4*)(sl + (size_t)k * (64 * T * 64) + so);
    float* o = dW + (size_t)(co_t * 64 + row) * row_len + t * a.Cin + ci_s * 64 + qd * 4;
    *(f32x4*)o = *(const f32x4*)o + s;
  }
  if (t == 0 && a.db[job] != nullptr && ci_s == 0 && threadIdx.x < 64) {
    const float* sb = a.slabb + (size_t)tile_g * a.S * 64;
    float s = sb[threadIdx.x];
    for (int k = 1; k < a.S; ++k) s += sb[k * 64 + threadIdx.x];
    a.db[job][co_t * 64 + threadIdx.x] += s;
  }
}

static int ws_window_rows(int halo) { return (64 + 2 * halo + 31) / 32 * 32; }

// dY and X on the same H x W grid, one pad row / column (a_bytes / b_bytes: wgs_limits)
static WgsRaster ws_raster(const s2p_conv_desc* d) {
  WgsRaster g{};
  g.N = d->N; g.Ha = g.Hb = d->H; g.Wa = g.Wb = d->W; g.Hp = d->H + 1; g.Wp = d->W + 1; g.bs = 1;
  g.a_pitch = d->y_pitch; g.b_pitch = d->x_pitch;
  return g;
}

static bool ws_supported(const s2p_conv_desc* d, int n_jobs, int cin_real, int cout_real) {
  if (d->dtype != S2P_BF16 || d->transposed || d->reflect || d->groups != 1) return false;
  if (d->KH != 3 || d->KW != 3 || d->stride != 1 || d->pad != 1) return false;
  if (d->Ho != d->H || d->Wo != d->W) return false;
  if (d->Cin % 64 || d->Cout % 64 || cin_real != d->Cin || cout_real != d->Cout) return false;
  if (n_jobs < 1 || n_jobs > WS_MAX_JOBS) return false;
  const int halo = (d->W + 1) + 1;
  if (ws_window_rows(halo) > 256) return false;
  WgsRaster g = ws_raster(d); bool tbl;
  return wgs_limits(g, tbl);
}

static int ws_splits(const s2p_conv_desc* d, int n_jobs) {
  const int tiles = n_jobs * (d->Cout / 64) * (d->Cin / 64);
  const int nblocks = cdiv((long long)d->N * (d->H + 1) * (d->W + 1), 64);
  const int forced = s2p_env_int("S2P_WGRAD_SLAB_SPLITS", 0);
  int S = forced > 0 ? forced : cdiv(3 * s2p_num_cus(), tiles);          // ~3 workgroups per CU (two resident, one queued)
  if (S > 8) S = 8;
  if (S > nblocks) S = nblocks;
  if (S < 1) S = 1;
  const int bps = cdiv(nblocks, S);
  return cdiv(nblocks, bps);
}

extern "C" size_t s2p_conv2d_wgrad_batched_workspace(const s2p_conv_desc* d, int n_jobs, int cin_real, int cout_real) {
  if (d && n_jobs >= 1 && s2p_head_wgrad_supported(d, cin_real, cout_real)) return (size_t)n_jobs * s2p_head_wgrad_workspace(d);
  if (!d) return 0;
  if (!ws_supported(d, n_jobs, cin_real, cout_real)) return s2p_conv2d_wgrad_workspace(d, cin_real, cout_real);   // jobs run one after the other
  const int S = ws_splits(d, n_jobs);
  if (S == 1) return 0;
  const size_t tiles = (size_t)n_jobs * (d->Cout / 64) * (d->Cin / 64);
  return tiles * S * (64 * 9 * 64 + 64) * sizeof(float);
}

extern "C" int s2p_conv2d_wgrad_batched(const s2p_conv_desc* d, const s2p_wgrad_job* jobs, int n_jobs, int cin_real,
                                        int cout_real, void* workspace, size_t workspace_bytes, void* stream) {
  if (!d || !jobs || n_jobs < 1) S2P_FAIL(-1, "s2p_conv2d_wgrad_batched: null pointer / no jobs");
  for (int j = 0; j < n_jobs; ++j)
    if (!jobs[j].x || !jobs[j].dy || !jobs[j].dw) S2P_FAIL(-1, "s2p_conv2d_wgrad_batched: job %d has a null pointer", j);
  if (s2p_head_wgrad_supported(d, cin_real, cout_real)) {
    // PatchGAN logit heads (Cout = 1): activation-stationary kernel + fixed-order partial reduce (csrc/wgrad_head.hip)
    const size_t per = s2p_head_wgrad_workspace(d);
    if (!workspace || workspace_bytes < per * n_jobs) S2P_FAIL(-1, "s2p_conv2d_wgrad_batched: workspace of %zu bytes needed", per * n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
      int rc = s2p_head_wgrad(d, jobs[j].x, jobs[j].dy, jobs[j].dw, jobs[j].db, cin_real, (char*)workspace + j * per, per,
                              (hipStream_t)stream);
      if (rc) return rc;
    }
    return 0;
  }
  if (!ws_supported(d, n_jobs, cin_real, cout_real)) {
    // geometry outside the slab kernel's scope (other taps / strides / dtypes): one generic launch per job, stream-ordered
    // on the same workspace
    for (int j = 0; j < n_jobs; ++j) {
      int rc = s2p_conv2d_wgrad_ws(d, jobs[j].x, jobs[j].dy, jobs[j].dw, jobs[j].db, cin_real, cout_real, 0, 0, workspace,
                                   workspace_bytes, stream);
      if (rc) return rc;
    }
    return 0;
  }
  WgSlabArgs a{};
  for (int j = 0; j < n_jobs; ++j) { a.A[j] = jobs[j].dy; a.B[j] = jobs[j].x; a.dW[j] = jobs[j].dw; a.db[j] = jobs[j].db; }
  // tabulated padded raster where it applies (wgs_limits; ws_supported has checked the limits themselves)
  bool tbl;
  a.g = ws_raster(d); wgs_limits(a.g, tbl);
  const int Wp = a.g.Wp;
  a.Cin = d->Cin;
  a.co_tiles = d->Cout / 64; a.tiles_per_job = a.co_tiles * (d->Cin / 64);
  a.nblocks = cdiv((long long)d->N * a.g.Hp * Wp, 64);
  a.S = ws_splits(d, n_jobs);
  a.blocks_per_split = cdiv(a.nblocks, a.S);
  a.halo = Wp + 1;
  const int wrows = ws_window_rows(a.halo);
  for (int ky = 0; ky < 3; ++ky)
    for (int kx = 0; kx < 3; ++kx) a.toff[ky * 3 + kx] = (ky - 1) * Wp + (kx - 1);
  const int tiles = n_jobs * a.tiles_per_job;
  a.total_wgs = tiles * a.S;
  if (a.S > 1) {
    const size_t need = (size_t)tiles * a.S * (64 * 9 * 64 + 64) * sizeof(float);
    if (!workspace || workspace_bytes < need)
      S2P_FAIL(-1, "s2p_conv2d_wgrad_batched: workspace of %zu bytes needed (s2p_conv2d_wgrad_batched_workspace), got %zu", need, workspace_bytes);
    a.slab = (float*)workspace;
    a.slabb = a.slab + (size_t)tiles * a.S * (64 * 9 * 64);
  }
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(a.total_wgs);
  if (wrows <= 128) { if (tbl) hipLaunchKernelGGL((wgrad_slab_kernel<128, true>), grid, dim3(256), 0, st, a); else hipLaunchKernelGGL((wgrad_slab_kernel<128, false>), grid, dim3(256), 0, st, a); }
  else if (wrows <= 192) { if (tbl) hipLaunchKernelGGL((wgrad_slab_kernel<192, true>), grid, dim3(256), 0, st, a); else hipLaunchKernelGGL((wgrad_slab_kernel<192, false>), grid, dim3(256), 0, st, a); }
  else { if (tbl) hipLaunchKernelGGL((wgrad_slab_kernel<256, true>), grid, dim3(256), 0, st, a); else hipLaunchKernelGGL((wgrad_slab_kernel<256, false>), grid, dim3(256), 0, st, a); }
  S2P_CHECK_LAUNCH("wgrad_slab_kernel");
  if (a.S > 1) {
    hipLaunchKernelGGL(wgrad_slab_reduce_kernel, dim3(tiles * 9), dim3(256), 0, st, a);
    S2P_CHECK_LAUNCH("wgrad_slab_reduce_kernel");
  }
  return 0;
}
