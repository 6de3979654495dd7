// The pipeline the two padded-raster weight-gradient kernels share (wgrad_slab.hip: stride-1 3x3 convs, several jobs per launch;
// wgrad_slabg.hip: the PatchGAN 4x4 layers as parity classes).  A workgroup (4 waves) accumulates a 64 (A channels) x T taps x 64
// (B channels) tile over a range of 64-position raster blocks:
//   acc[t][a][b] += sum over positions k of the block range:  A[k][a] * B[k + toff[t]][b],      accb[a] += sum_k A[k][a]
// Both operands are addressed on a PADDED RASTER k = (n*Hp + r)*Wp + c; pad positions read zeros (the LDS-DMA's out-of-range offset),
// so a tap is a pure row shift of ONE resident B window (64 positions + the halo the taps reach) and image borders need no masks.
// [position][channel] staging as the tensors lie in HBM, fragments from `ds_read_b64_tr_b16`; 128-byte LDS rows with the 16-byte
// chunk index XOR-ed by ((row >> 1) & 1) << 2 (on the DMA source address and on the read) are conflict-free for the four rows x 64
// bytes a half-wave touches.  3-stage LDS-DMA pipeline, counted vmcnt, raw barrier.  What differs between the two kernels -- the
// argument block, workgroup -> (tile, split), the final epilogue and the reduce -- stays in their files.
#pragma once
#include "s2p_common.h"

// Geometry of a launch.  A lives on the Ha x Wa grid; raster position (r, c) reads B at pixel (bs*r + py, bs*c + px) of its Hb x Wb
// grid (bs = 2: the parity sub-plane (py, px), the space-to-depth is done by the DMA's per-lane source address).  The stride-1 3x3
// kernel is Ha = Hb, Wa = Wb, bs = 1, py = px = 0.  Pitches in elements, a_bytes / b_bytes: the tensors' sizes (the DMA's range).
struct WgsRaster {
  int N, Ha, Wa, Hb, Wb, Hp, Wp, bs, py, px;
  int a_pitch, b_pitch;
  unsigned a_bytes, b_bytes;
};

// TBL: the padded raster of one image (Hp * Wp <= WGS_TBL_MAX positions) is tabulated in LDS once per workgroup, one table per
// operand -- position -> byte offset of the pixel inside its image, 0xc0000000 where the position is padding -- and a DMA's source
// offset is  table[q] + (image offset + chunk offset):  6 VALU instructions per DMA (advance q with one wrap, one add) and one
// 4-byte LDS read issued a whole block ahead, instead of ~19 for the (n, row, column) state with its bounds tests and two
// multiplies.  Round 5's instruction-mix counters: the kernel spent 3.7 VALU instructions per MFMA, nearly all of them on these
// addresses, and 81 % of its time is VALU + MFMA issue.  A padding position adds up to an offset in [2^31 + 2^29, 2^32 - 2^29) and
// an image index outside [0, N) to one below 0 or beyond the tensor: either way the buffer range check returns zeros (the host
// keeps the tensors below 2^29 bytes on this path).
constexpr int WGS_TBL_MAX = 768;
constexpr int WGS_TBL_BYTES = 2 * WGS_TBL_MAX * 4;            // [A | B], a multiple of 1 KiB
constexpr int WGS_NST = 3;
// one stage: 64 positions x 64 A channels, then the B window of NXI * 32 rows (64 positions + halo) x 64 B channels; 128-byte rows
constexpr int wgs_stage_bytes(int nxi) { return (64 + nxi * 32) * 128; }

// flattened workgroup id, spread so that workgroups b, b+8, ... (one XCD) hold consecutive ids: neighbouring tiles stream the same
// A / B rows and share that XCD's L2
__device__ __forceinline__ int wgs_xcd_spread(int bid, int nw) {
  const int q8 = nw >> 3, r8 = nw & 7, xcd = bid & 7, k = bid >> 3;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + k;
}

// Raster blocks [b0, b0 + nblk) (nblk >= 1) of tile (co_t, ci_s) into acc[T] and, with do_bias (wave-uniform), accb.
// toff[t]: raster offset of tap t; halo: window rows in front of the block's first position (>= -min toff, < Hp * Wp).
// smem: WGS_NST stages; ptab: the two tables (TBL only), at LDS address 0 so that their byte offsets fit a ds_read's immediate.
// Wave w holds A channels [32 (w >> 1), +32) x B channels [32 (w & 1), +32) of every tap.
template <int T, int NXI, bool TBL>
__device__ __forceinline__ void wgs_accumulate(const WgsRaster& g, const void* A, const void* B, const int* toff, const int halo,
                                               const int co_t, const int ci_s, const int b0, const int nblk, const bool do_bias,
                                               char* const smem, unsigned* const ptab, f32x16 (&acc)[T], f32x16& accb) {
  constexpr int RS = 128, NST = WGS_NST;
  constexpr int ASTG = 64 * RS;                 // 8 KiB: 64 positions x 64 A channels
  constexpr int STG = wgs_stage_bytes(NXI);
  constexpr int NDMA = 2 + NXI;                 // DMA instructions per wave per block (8 rows each, 4 waves): 2 of A, NXI of B
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  const unsigned OOB = 0x80000000u;
  const i32x4 ar = s2p_make_rsrc(A, g.a_bytes);
  const i32x4 br = s2p_make_rsrc(B, g.b_bytes);
  const unsigned lds0 = __builtin_amdgcn_readfirstlane(s2p_lds_addr(smem));

  // ---- DMA geometry: a piece = 8 rows x 128 B; lane -> (row in piece, physical chunk).  Every lane keeps the padded-
  //      raster coordinates (n, r, c) of the NDMA rows it stages and advances them by 64 positions per block with a few
  //      branch-free adds / selects (a division per DMA would cost more issue slots than the block's MFMAs).
  const int lrow = lane >> 3, pch = lane & 7;
  const int a_cbyte = (co_t * 64) * 2, b_cbyte = (ci_s * 64) * 2;
  int pn[NDMA], prr[NDMA], pc[NDMA];
  int cb[NDMA];                                                // chunk byte offset (swizzled) + channel base
  // TBL: q4 = 4 * (position inside its image's padded raster), noffc = image offset + chunk offset (bytes), tv = the table entry of q
  unsigned q4[NDMA], noffc[NDMA], tv[NDMA];
  const int HpWp = g.Hp * g.Wp;
  if constexpr (TBL) {
    for (int q = tid; q < HpWp; q += 256) {
      const int r = q / g.Wp, c = q - r * g.Wp;
      ptab[q] = (c < g.Wa && r < g.Ha) ? (unsigned)(r * g.Wa + c) * (unsigned)(g.a_pitch * 2) : 0xc0000000u;
      const int sy = r * g.bs + g.py, sx = c * g.bs + g.px;      // B's pixel in the full-resolution tensor
      ptab[WGS_TBL_MAX + q] = (sy < g.Hb && sx < g.Wb) ? (unsigned)(sy * g.Wb + sx) * (unsigned)(g.b_pitch * 2) : 0xc0000000u;
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < NDMA; ++i) {
    const int row = (4 * (i < 2 ? i : i - 2) + wave) * 8 + lrow;
    int pos = b0 * 64 + row - (i < 2 ? 0 : halo);
    int nadj = 0;
    if (pos < 0) { pos += g.Hp * g.Wp; nadj = -1; }            // pos >= -halo > -Hp*Wp
    cb[i] = (i < 2 ? a_cbyte : b_cbyte) + ((pch ^ (((row >> 1) & 1) << 2)) * 16);
    if constexpr (TBL) {
      const int n = pos / HpWp, q = pos - n * HpWp;
      q4[i] = (unsigned)q * 4u;
      noffc[i] = (unsigned)((n + nadj) * (i < 2 ? g.Ha * g.Wa * g.a_pitch * 2 : g.Hb * g.Wb * g.b_pitch * 2) + cb[i]);
      tv[i] = ptab[(i < 2 ? 0 : WGS_TBL_MAX) + q];
    } else {
      const int q1 = pos / g.Wp;
      pc[i] = pos - q1 * g.Wp;
      const int n = q1 / g.Hp;
      prr[i] = q1 - n * g.Hp;
      pn[i] = n + nadj;
    }
  }
  const int a_pitch2 = g.a_pitch * 2, b_pitch2 = g.b_pitch * 2;
  // 64 positions = adv_n images + adv_r rows + adv_c columns (block-uniform scalars)
  const int adv_q = 64 / g.Wp, adv_c = 64 - adv_q * g.Wp, adv_n = adv_q / g.Hp, adv_r = adv_q - adv_n * g.Hp;
  // TBL: 64 positions = tadv_n images + tadv_q positions; HpWp4 = 4 Hp Wp
  const int tadv_n = 64 / HpWp;
  const unsigned tadv_q4 = (unsigned)(64 - tadv_n * HpWp) * 4u, HpWp4 = (unsigned)HpWp * 4u;
  const unsigned img_a = (unsigned)(g.Ha * g.Wa) * (unsigned)a_pitch2, img_b = (unsigned)(g.Hb * g.Wb) * (unsigned)b_pitch2;
  // one DMA (index i of this wave's NDMA per block) of the block the coordinate state points at, then advance that state
  auto issue_one = [&](auto ic, unsigned base) {
    constexpr int i = decltype(ic)::value;
    if constexpr (TBL) {
      const unsigned off = tv[i] + noffc[i];
      if (i < 2) s2p_dma16(ar, base + (4 * i + wave) * 1024, (int)off);
      else s2p_dma16(br, base + ASTG + (4 * (i - 2) + wave) * 1024, (int)off);
      const unsigned img = i < 2 ? img_a : img_b;
      const unsigned qa = q4[i] + tadv_q4;
      const bool wrap = qa >= HpWp4;
      q4[i] = wrap ? qa - HpWp4 : qa;
      noffc[i] += (unsigned)tadv_n * img + (wrap ? img : 0u);
      tv[i] = *(const unsigned*)((const char*)(ptab + (i < 2 ? 0 : WGS_TBL_MAX)) + q4[i]);      // consumed a whole block later
    } else {
      int off;
      if constexpr (i < 2) {
        const bool ok = pc[i] < g.Wa && prr[i] < g.Ha && (unsigned)pn[i] < (unsigned)g.N;
        const int pix = __mul24(__mul24(pn[i], g.Ha) + prr[i], g.Wa) + pc[i];           // < 2^24 (host-checked)
        off = ok ? __mul24(pix, a_pitch2) + cb[i] : (int)OOB;
        s2p_dma16(ar, base + (4 * i + wave) * 1024, off);
      } else {
        const int sy = prr[i] * g.bs + g.py, sx = pc[i] * g.bs + g.px;                  // B's pixel in the full-resolution tensor
        const bool ok = sy < g.Hb && sx < g.Wb && (unsigned)pn[i] < (unsigned)g.N;
        const int pix = __mul24(__mul24(pn[i], g.Hb) + sy, g.Wb) + sx;
        off = ok ? __mul24(pix, b_pitch2) + cb[i] : (int)OOB;
        s2p_dma16(br, base + ASTG + (4 * (i - 2) + wave) * 1024, off);
      }
      int c = pc[i] + adv_c, r = prr[i] + adv_r, n = pn[i] + adv_n;
      const bool cw = c >= g.Wp;
      c = cw ? c - g.Wp : c; r += cw ? 1 : 0;
      const bool rw = r >= g.Hp;
      r = rw ? r - g.Hp : r; n += rw ? 1 : 0;
      pc[i] = c; prr[i] = r; pn[i] = n;
    }
  };
  auto issue = [&](int stage) {
    const unsigned base = lds0 + stage * STG;
    s2p_static_for<0, NDMA>([&](auto ic) { issue_one(ic, base); });
  };

  // ---- fragment geometry (ds_read_b64_tr_b16): 16-lane group gq: channel block 16*(gq&1), k half gq>>1; inside the
  //      group lane 4q+p supplies row q, columns 4p..4p+3 -------------------------------------------------------------
  const int gq = lane >> 4, gg = gq & 1, hh = gq >> 1, q = (lane >> 2) & 3, p = lane & 3;
  const int wa = wave >> 1, wb = wave & 1;
  const int a_lane = (8 * hh + q) * RS + (((4 * wa + 2 * gg + (p >> 1)) ^ ((q >> 1) << 2)) * 16) + 8 * (p & 1);
  int b_lane[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int r0 = halo + toff[t] + 8 * hh + q;                // window row of this lane for k = 0, half 0
    b_lane[t] = ASTG + r0 * RS + (((4 * wb + 2 * gg + (p >> 1)) ^ (((r0 >> 1) & 1) << 2)) * 16) + 8 * (p & 1);
  }

#pragma unroll
  for (int e = 0; e < 16; ++e) accb[e] = 0.f;
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  const s16x8 ones_s = {0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80};   // bf16 1.0
  const bf16x8 ones = __builtin_bit_cast(bf16x8, ones_s);
  typedef __attribute__((address_space(3))) s16x4* lds_s16x4;

  // ---- 3-stage pipeline over the blocks of this split ----------------------------------------------------------------
  issue(0);
  if (nblk > 1) { issue(1); S2P_WAIT_VMCNT(NDMA); } else { S2P_WAIT_VMCNT(0); }
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  // Inside a block the 4 T (substep, tap) MFMAs of a wave run as one software pipeline: the two transposed reads of the B
  // fragment used LA steps later and, once per substep, the next A fragment are issued right behind each MFMA, so an
  // MFMA never waits on a read issued less than ~LA x 32 cycles earlier; the block's DMAs (for block kb + 2) are spread
  // over the steps instead of being issued as one burst in front of the first read.
  constexpr int NSTEP = 4 * T;
  constexpr int LA = NSTEP < 4 ? NSTEP : 4, RING = LA + 1;
  constexpr int TA = T - 1 - LA >= 0 ? T - 1 - LA : 0;         // tap step behind which the next substep's A fragment is read
  auto read_frag = [&](const char* ptr) {
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(ptr));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(ptr + 4 * RS));
    // (a concatenation, not eight element inserts: the inserts cost four v_mov_b32 per fragment -- 4.7 VALU instructions per MFMA
    // in this loop, round 5's instruction-mix counters)
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
  };
  auto main_loop = [&](auto biasc) {
    constexpr bool BIAS = decltype(biasc)::value;
    int stage = 0;
    for (int kb = 0; kb < nblk; ++kb) {
      int st2 = stage + 2; if (st2 >= NST) st2 -= NST;
      const bool more = kb + 2 < nblk;
      const unsigned dbase = lds0 + st2 * STG;
      const char* sb = smem + stage * STG;
      bf16x8 AF[2], BF[RING];
      AF[0] = read_frag(sb + a_lane);
      s2p_static_for<0, LA>([&](auto vc) {
        constexpr int v = decltype(vc)::value;
        BF[v % RING] = read_frag(sb + b_lane[v % T] + (v / T) * 16 * RS);
      });
      s2p_static_for<0, NSTEP>([&](auto uc) {
        constexpr int u = decltype(uc)::value, s_ = u / T, t = u % T;
        if constexpr (BIAS && t == 0) accb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AF[s_ & 1], ones, accb, 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AF[s_ & 1], BF[u % RING], acc[t], 0, 0, 0);
        constexpr int v = u + LA;
        if constexpr (v < NSTEP) BF[v % RING] = read_frag(sb + b_lane[v % T] + (v / T) * 16 * RS);
        if constexpr (t == TA && s_ < 3) AF[(s_ + 1) & 1] = read_frag(sb + a_lane + (s_ + 1) * 16 * RS);
        // DMA i of block kb + 2 goes out behind step (i * NSTEP) / NDMA + 1 (the last step at the latest)
        s2p_static_for<0, NDMA>([&](auto ic) {
          constexpr int i = decltype(ic)::value;
          constexpr int at = (i * NSTEP) / NDMA + 1 < NSTEP ? (i * NSTEP) / NDMA + 1 : NSTEP - 1;
          if constexpr (u == at) { if (more) issue_one(ic, dbase); }
        });
        __builtin_amdgcn_sched_barrier(0);
      });
      // block kb+1 must have landed (for every wave) before anyone reads it; block kb+2 may stay in flight
      if (more) S2P_WAIT_VMCNT(NDMA); else S2P_WAIT_VMCNT(0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      if (++stage == NST) stage = 0;
    }
  };
  if (do_bias) main_loop(std::integral_constant<bool, true>{});
  else main_loop(std::integral_constant<bool, false>{});
}

// The partial tile of one (tile, split) with plain stores: sl[64 A rows][T][64 B channels], lanes <-> consecutive B channels
// (contiguous floats), registers <-> A rows; slb[64] (bias partials) from the waves that ran the bias MFMA.
template <int T>
__device__ __forceinline__ void wgs_store_slab(float* sl, float* slb, const f32x16 (&acc)[T], const f32x16& accb, const bool do_bias) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wa = wave >> 1, wb = wave & 1, r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = 32 * wa + (e & 3) + 8 * (e >> 2) + 4 * h;
      sl[(row * T + t) * 64 + 32 * wb + r] = acc[t][e];
    }
  if (do_bias && r == 0) {
#pragma unroll
    for (int e = 0; e < 16; ++e) slb[32 * wa + (e & 3) + 8 * (e >> 2) + 4 * h] = accb[e];
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// Fills a_bytes / b_bytes.  false: beyond the kernels' addressing -- pixel and raster position indices go through 24-bit
// multiplies (2^23: exact with a sign), DMA offsets are 31-bit.  tbl: the tabulated raster applies (see WGS_TBL_MAX: images of
// <= WGS_TBL_MAX padded positions, tensors of <= 2^29 bytes so that image offsets stay exact in 32 bits and padding stays out of
// range); switch 18 of the diagnostics build selects the (n, row, column) state everywhere.
static inline bool wgs_limits(WgsRaster& g, bool& tbl) {
  if ((long long)g.N * g.Hp * g.Wp >= (1 << 23) || (long long)g.N * g.Hb * g.Wb >= (1 << 23) || (long long)g.N * g.Ha * g.Wa >= (1 << 23)) return false;
  const long long ab = (long long)g.N * g.Ha * g.Wa * g.a_pitch * 2, bb = (long long)g.N * g.Hb * g.Wb * g.b_pitch * 2;
  if (ab >= (1ll << 31) || bb >= (1ll << 31)) return false;
  g.a_bytes = (unsigned)ab; g.b_bytes = (unsigned)bb;
  tbl = g.Hp * g.Wp <= WGS_TBL_MAX && ab <= (1ll << 29) && bb <= (1ll << 29) && !S2P_DIAG_SWITCH(18);
  return true;
}
