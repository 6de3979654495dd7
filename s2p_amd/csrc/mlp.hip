// Grouped ReLU linear layers forward and backward: every s2p_mlp_linear_* entry point and its kernels, the layer machinery of the
// latent RL trainers (SPEC.md N3d, N3e).  Group = network: qf1, qf2, the targets, vf and the policy are MLPs of one hidden width but
// of unequal input width and row count, so a call carries a table of per-group views (at most MLP_MAX_G, copied into the kernel
// arguments) and one launch serves all of them, grid z = group.  Wide layers run on the wave tiles of ens_tile.h (the tiles of the
// ensemble entry points, here with ReLU or identity); the N = 1 and N = 2 A last layers run on plain dot-product kernels (a 32 x 64
// MFMA tile would be 98 % / 81 % padding there, and with one wave per row the reads are whole contiguous rows).  Three backward
// forms share the tiles, so what they write agrees bit for bit: the full backward; the input gradient alone (the CQL policy loss is
// differentiated THROUGH the critics to the action, and the critics' gradient buffers must stay as they are); the full backward with
// the rows of each weight tile split into chunks.  All fp32, no atomics, a fixed summation order: two identical calls give bitwise
// identical results.  The s2p_mlp_linear_*_bf16 entry points (SPEC.md N3l) are the wide-layer kernels over the tiles of
// ens_tile_bf16.h: the same tensors, tables, grids and checks, both operands of every product rounded to bf16 as a tile loads them.
#include "ens_tile_bf16.h"

#define MLP_MAX_G 8
#define MLP_DOT_MAX_N 16
struct MlpFwdArgs { EnsFwdTile g[MLP_MAX_G]; };
struct MlpBwdArgs { EnsBwdTile g[MLP_MAX_G]; };              // the full backward and the input gradient alone (x, dw, db NULL there)

// ---- wide layers: the MFMA wave tiles, fp32 compute (ens_tile.h) or with BF16 the bf16 compute of ens_tile_bf16.h ---------------------
template <int ACT, bool BF16> __global__ __launch_bounds__(256) void mlp_fwd_kernel(const MlpFwdArgs a) {
  const EnsFwdTile t = a.g[blockIdx.z];
  const int wave = threadIdx.x >> 6, nb = blockIdx.x * 64, mb = blockIdx.y * 128 + wave * 32;
  if (mb >= t.B) return;                                     // (wave-uniform; a group of fewer rows than the widest one ends here)
  if constexpr (BF16) ens_fwd_tile_bf16<ACT>(t, mb, nb);
  else ens_fwd_tile<ACT>(t, mb, nb);
}
// input tile `id` of group view t (four waves = 128 rows per workgroup, row tiles outermost): nothing past the group's last tile.
// tk = the group's tiles along K and the wave index come from the caller, which has both at hand for its weight tiles
template <int ACT, bool BF16> __device__ __forceinline__ void mlp_input_tile(const EnsBwdTile& t, int id, int tk, int wave) {
  const int tm = (t.B + 127) / 128;
  if (id >= tm * tk) return;
  const int mb = (id / tk) * 128 + wave * 32;
  if (mb >= t.B) return;                                     // (wave-uniform)
  if constexpr (BF16) ens_dgrad_tile_bf16<ACT>(t, mb, (id % tk) * 64);
  else ens_dgrad_tile<ACT>(t, mb, (id % tk) * 64);
}
// grid x: the weight tiles of a group (four waves = four tiles per workgroup), then its input tiles; sized for the largest group
template <int ACT, bool BF16> __global__ __launch_bounds__(256) void mlp_bwd_kernel(const MlpBwdArgs a) {
  const EnsBwdTile t = a.g[blockIdx.z];
  const int wave = threadIdx.x >> 6;
  if (t.B == 0) return;
  const int tk = (t.K + 63) / 64, w_tiles = ((t.N + 31) / 32) * tk, w_blocks = (w_tiles + 3) / 4;
  if ((int)blockIdx.x < w_blocks) {
    const int id = blockIdx.x * 4 + wave;
    if (id >= w_tiles) return;                               // (wave-uniform)
    if constexpr (BF16) ens_wgrad_tile_bf16(t, (id / tk) * 32, (id % tk) * 64);
    else ens_wgrad_tile(t, (id / tk) * 32, (id % tk) * 64);
    return;
  }
  if (!t.dprev) return;
  mlp_input_tile<ACT, BF16>(t, blockIdx.x - w_blocks, tk, wave);
}
// the input gradient alone: the input tiles of mlp_bwd_kernel
template <int ACT, bool BF16> __global__ __launch_bounds__(256) void mlp_dgrad_kernel(const MlpBwdArgs a) {
  const EnsBwdTile t = a.g[blockIdx.z];
  if (t.B == 0) return;
  mlp_input_tile<ACT, BF16>(t, blockIdx.x, (t.K + 63) / 64, threadIdx.x >> 6);
}

// ---- the grouped backward with the rows of each weight tile divided into S contiguous chunks: chunk s of a tile is one wave that
//      sums its rows in row order into partial s of a caller-owned workspace ([S][dw [N][K] | db [N]] per group); a second kernel
//      adds the partials in the order s = 0 .. S - 1.  More waves for a launch whose weight tiles alone do not fill the chip, and
//      S shorter summation chains.  The input tiles are those of mlp_bwd_kernel --------------------------------------------------------
struct MlpSplitArgs { EnsBwdTile g[MLP_MAX_G]; float* ws[MLP_MAX_G]; int chunk[MLP_MAX_G]; int S; };
template <int ACT, bool BF16> __global__ __launch_bounds__(256) void mlp_bwd_split_kernel(const MlpSplitArgs a) {
  EnsBwdTile t = a.g[blockIdx.z];
  const int wave = threadIdx.x >> 6;
  if (t.B == 0) return;
  const int tk = (t.K + 63) / 64, w_tiles = ((t.N + 31) / 32) * tk, w_blocks = (w_tiles + 3) / 4;
  if ((int)blockIdx.x < w_blocks * a.S) {
    const int s = blockIdx.x / w_blocks, id = (blockIdx.x % w_blocks) * 4 + wave;
    if (id >= w_tiles) return;                               // (wave-uniform)
    const size_t nk = (size_t)t.N * t.K;
    t.dw = a.ws[blockIdx.z] + (size_t)s * (nk + t.N);
    t.db = t.dw + nk;
    const int mb = s * a.chunk[blockIdx.z];                  // (a chunk past the last row sums nothing and writes zeros)
    if constexpr (BF16) ens_wgrad_tile_bf16(t, (id / tk) * 32, (id % tk) * 64, mb, mb + a.chunk[blockIdx.z]);
    else ens_wgrad_tile(t, (id / tk) * 32, (id % tk) * 64, mb, mb + a.chunk[blockIdx.z]);
    return;
  }
  if (!t.dprev) return;
  mlp_input_tile<ACT, BF16>(t, blockIdx.x - w_blocks * a.S, tk, wave);
}
__global__ __launch_bounds__(256) void mlp_split_sum_kernel(const MlpSplitArgs a) {
  const EnsBwdTile t = a.g[blockIdx.z];
  if (t.B == 0) return;
  const size_t nk = (size_t)t.N * t.K, per = nk + t.N, idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= per) return;
  const float* p = a.ws[blockIdx.z] + idx;
  float s = p[0];                                            // (S = 1 hands the one partial on bit for bit)
  for (int c = 1; c < a.S; ++c) s += p[(size_t)c * per];
  if (idx < nk) t.dw[idx] = s;
  else t.db[idx - nk] = s;
}

// ---- narrow last layers (N <= MLP_DOT_MAX_N): dot products ----------------------------------------------------------------------------
// forward: one wave per row; lane l takes k = 4 l .. 4 l + 3 of every 256, in k order, then the 64 lane sums meet in a butterfly
template <int ACT> __global__ __launch_bounds__(256) void mlp_dot_fwd_kernel(const MlpFwdArgs a) {
  const EnsFwdTile t = a.g[blockIdx.z];
  const int lane = threadIdx.x & 63, m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= t.B) return;                                      // (wave-uniform)
  const float* xr = t.x + (size_t)m * t.xp;
  for (int n = 0; n < t.N; ++n) {
    const float* wr = t.w + (size_t)n * t.K;
    float s = 0.f;
    for (int k = lane * 4; k < t.K; k += 256) {              // K is a multiple of 4: a float4 is in or out
      const f32x4 xv = *(const f32x4*)(xr + k), wv = *(const f32x4*)(wr + k);
#pragma unroll
      for (int c = 0; c < 4; ++c) s += xv[c] * wv[c];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) {
      const float v = s + t.bias[n];
      const size_t o = (size_t)m * t.yp + n;
      if (t.pre) t.pre[o] = v;
      if (t.act) t.act[o] = ens_act<ACT>(v);
    }
  }
}
// backward.  Weight blocks: 64 input columns x 4 row lanes; row lane r sums the rows r, r + 4, ... in row order, then the four
// partial sums are added in lane order through LDS (db from the same loop, by the first block).  Input blocks: one thread per
// (row, column) of dprev, n in order.
template <int ACT> __global__ __launch_bounds__(256) void mlp_dot_bwd_kernel(const MlpBwdArgs a) {
  __shared__ float red[4][MLP_DOT_MAX_N + 1][64];
  const EnsBwdTile t = a.g[blockIdx.z];
  if (t.B == 0) return;
  const int col = threadIdx.x & 63, rl = threadIdx.x >> 6, wb = (t.K + 63) / 64;
  if ((int)blockIdx.x < wb) {
    const int k = blockIdx.x * 64 + col;
    const bool kok = k < t.K, bias_lane = blockIdx.x == 0 && col < t.N;
    float acc[MLP_DOT_MAX_N] = {}, bs = 0.f;
    for (int m = rl; m < t.B; m += 4) {
      const float xv = kok ? t.x[(size_t)m * t.xp + k] : 0.f;
      const float* dr = t.dpre + (size_t)m * t.dp;
#pragma unroll
      for (int n = 0; n < MLP_DOT_MAX_N; ++n)
        if (n < t.N) acc[n] += dr[n] * xv;
      if (bias_lane) bs += dr[col];
    }
#pragma unroll
    for (int n = 0; n < MLP_DOT_MAX_N; ++n) red[rl][n][col] = acc[n];
    red[rl][MLP_DOT_MAX_N][col] = bs;
    __syncthreads();
    if (rl != 0) return;
#pragma unroll
    for (int n = 0; n < MLP_DOT_MAX_N; ++n)
      if (n < t.N && kok) t.dw[(size_t)n * t.K + k] = ((red[0][n][col] + red[1][n][col]) + red[2][n][col]) + red[3][n][col];
    if (bias_lane)
      t.db[col] = ((red[0][MLP_DOT_MAX_N][col] + red[1][MLP_DOT_MAX_N][col]) + red[2][MLP_DOT_MAX_N][col]) + red[3][MLP_DOT_MAX_N][col];
    return;
  }
  if (!t.dprev) return;
  ens_dot_dgrad_elem<ACT>(t, (long long)(blockIdx.x - wb) * 256 + threadIdx.x);
}
// the input gradient alone: the input blocks of mlp_dot_bwd_kernel
template <int ACT> __global__ __launch_bounds__(256) void mlp_dot_dgrad_kernel(const MlpBwdArgs a) {
  const EnsBwdTile t = a.g[blockIdx.z];
  if (t.B == 0) return;
  ens_dot_dgrad_elem<ACT>(t, (long long)blockIdx.x * 256 + threadIdx.x);
}

// ---- entry points -------------------------------------------------------------------------------------------------------------------
// launch kernel<ReLU> or kernel<identity> on 256-thread workgroups
#define MLP_LAUNCH_ACT(kernel, act, grid, st, args) do { \
    if ((act) == S2P_ACT_RELU) hipLaunchKernelGGL(kernel<ENS_ACT_RELU>, grid, dim3(256), 0, st, args); \
    else hipLaunchKernelGGL(kernel<ENS_ACT_NONE>, grid, dim3(256), 0, st, args); \
    S2P_CHECK_LAUNCH(#kernel); } while (0)
// the same for a wide-layer kernel, on the fp32 tiles or (bf16 != 0) the bf16 tiles
#define MLP_LAUNCH_TILE(kernel, bf16, act, grid, st, args) do { \
    if (bf16) { \
      if ((act) == S2P_ACT_RELU) hipLaunchKernelGGL((kernel<ENS_ACT_RELU, true>), grid, dim3(256), 0, st, args); \
      else hipLaunchKernelGGL((kernel<ENS_ACT_NONE, true>), grid, dim3(256), 0, st, args); \
    } else if ((act) == S2P_ACT_RELU) hipLaunchKernelGGL((kernel<ENS_ACT_RELU, false>), grid, dim3(256), 0, st, args); \
    else hipLaunchKernelGGL((kernel<ENS_ACT_NONE, false>), grid, dim3(256), 0, st, args); \
    S2P_CHECK_LAUNCH(#kernel); } while (0)

// the head of a group table: 1 = go on, 0 = nothing to do, below 0 = refused
static int mlp_header(const char* who, const void* groups, int G, int N, int act) {
  if (G < 0 || N < 0) S2P_FAIL(-1, "%s: negative size", who);
  if (G == 0 || N == 0) return 0;
  if (!groups) S2P_FAIL(-1, "%s: null group table", who);
  if (G > MLP_MAX_G) S2P_FAIL(-1, "%s: at most %d groups (G %d)", who, MLP_MAX_G, G);
  if (act != S2P_ACT_NONE && act != S2P_ACT_RELU) S2P_FAIL(-1, "%s: activation %d (none and relu only)", who, act);
  return 1;
}
// the bf16 entry points have the MFMA-tile form only
static int mlp_bf16_wide(const char* who, int N) {
  if (N <= MLP_DOT_MAX_N) S2P_FAIL(-1, "%s: the MFMA-tile form only: N above %d (N %d); narrow layers run on the fp32 entry point", who, MLP_DOT_MAX_N, N);
  return 0;
}
// group g of a backward table -> its tile view; an empty group leaves *t as it is (B = 0: the kernels skip it).  `weights`: the
// caller writes dw / db (x, dw, db required, dprev optional), else the input gradient alone (dprev required, x not looked at);
// `wide`: the MFMA tiles read dpre in 16-byte groups
static int mlp_bwd_group(const char* who, int g, const s2p_mlp_bwd_group& s, int N, int act_prev, bool weights, bool wide, EnsBwdTile* t) {
  if (s.rows < 0 || s.K < 0) S2P_FAIL(-1, "%s: group %d: negative size", who, g);
  if (s.rows == 0 || s.K == 0) return 0;
  const bool prev_ok = s.w && (act_prev == S2P_ACT_NONE || s.pre_prev);
  if (weights) {
    if (!s.x || !s.dpre || !s.dw || !s.db) S2P_FAIL(-1, "%s: group %d: null tensor (x, dpre, dw, db are required)", who, g);
    if (s.dprev && !prev_ok) S2P_FAIL(-1, "%s: group %d: dprev needs w (and pre_prev with relu)", who, g);
  } else if (!s.dpre || !s.dprev || !prev_ok) {
    S2P_FAIL(-1, "%s: group %d: null tensor (dpre, w, dprev are required, and pre_prev with relu)", who, g);
  }
  if (wide && (s.dpre_pitch % 4 || !s2p_al16(s.dpre)))
    S2P_FAIL(-1, "%s: group %d: dpre_pitch must be a multiple of 4 floats, dpre 16-byte aligned", who, g);
  if ((weights && s.x_pitch < s.K) || s.dpre_pitch < N || (s.dprev && s.prev_pitch < s.K)) S2P_FAIL(-1, "%s: group %d: pitch shorter than the row", who, g);
  if ((int64_t)s.rows * s.K >= ((int64_t)1 << 31)) S2P_FAIL(-1, "%s: group %d: rows * K must stay below 2^31", who, g);
  *t = weights ? EnsBwdTile{s.x, s.dpre, s.w, s.dw, s.db, s.pre_prev, s.dprev, s.x_pitch, s.dpre_pitch, s.prev_pitch, s.rows, s.K, N}
               : EnsBwdTile{nullptr, s.dpre, s.w, nullptr, nullptr, s.pre_prev, s.dprev, 0, s.dpre_pitch, s.prev_pitch, s.rows, s.K, N};
  return 0;
}

// every entry point below is one function for both compute modes: `bf16` selects the tiles and refuses the narrow form
static int mlp_fwd(const char* who, bool bf16, const s2p_mlp_fwd_group* groups, int G, int N, int act, void* stream) {
  if (const int h = mlp_header(who, groups, G, N, act); h <= 0) return h;
  if (bf16) if (int rc = mlp_bf16_wide(who, N)) return rc;
  MlpFwdArgs a{};
  int rows = 0;
  for (int g = 0; g < G; ++g) {
    const s2p_mlp_fwd_group& s = groups[g];
    if (s.rows < 0 || s.K < 0) S2P_FAIL(-1, "%s: group %d: negative size", who, g);
    if (s.rows == 0) continue;                               // (an empty group: B = 0 in the table, no pointer looked at)
    if (!s.x || !s.w || !s.bias || (!s.pre && !s.act)) S2P_FAIL(-1, "%s: group %d: null tensor (x, w, bias and one of pre / act are required)", who, g);
    if (s.K == 0 || s.K % 4 || s.x_pitch % 4 || !s2p_al16(s.x) || !s2p_al16(s.w))
      S2P_FAIL(-1, "%s: group %d: K, x_pitch must be multiples of 4 floats (K > 0), x and w 16-byte aligned", who, g);
    if (s.x_pitch < s.K || s.y_pitch < N) S2P_FAIL(-1, "%s: group %d: pitch shorter than the row", who, g);
    a.g[g] = EnsFwdTile{s.x, s.w, s.bias, s.pre, s.act, s.x_pitch, s.y_pitch, s.rows, s.K, N};
    rows = s.rows > rows ? s.rows : rows;
  }
  if (rows == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  if (N <= MLP_DOT_MAX_N) MLP_LAUNCH_ACT(mlp_dot_fwd_kernel, act, dim3(cdiv(rows, 4), 1, G), st, a);
  else MLP_LAUNCH_TILE(mlp_fwd_kernel, bf16, act, dim3(cdiv(N, 64), cdiv(rows, 128), G), st, a);
  return 0;
}
extern "C" int s2p_mlp_linear_fwd(const s2p_mlp_fwd_group* groups, int G, int N, int act, void* stream) {
  return mlp_fwd("s2p_mlp_linear_fwd", false, groups, G, N, act, stream);
}
extern "C" int s2p_mlp_linear_fwd_bf16(const s2p_mlp_fwd_group* groups, int G, int N, int act, void* stream) {
  return mlp_fwd("s2p_mlp_linear_fwd_bf16", true, groups, G, N, act, stream);
}

static int mlp_bwd(const char* who, bool bf16, const s2p_mlp_bwd_group* groups, int G, int N, int act_prev, void* stream) {
  if (const int h = mlp_header(who, groups, G, N, act_prev); h <= 0) return h;
  if (bf16) if (int rc = mlp_bf16_wide(who, N)) return rc;
  const bool dot = N <= MLP_DOT_MAX_N;
  if (!dot && N % 4) S2P_FAIL(-1, "%s: N above %d must be a multiple of 4 (N %d)", who, MLP_DOT_MAX_N, N);
  MlpBwdArgs a{};
  int blocks = 0;
  for (int g = 0; g < G; ++g) {
    const s2p_mlp_bwd_group& s = groups[g];
    if (int rc = mlp_bwd_group(who, g, s, N, act_prev, true, !dot, &a.g[g])) return rc;
    if (a.g[g].B == 0) continue;
    const int tk = cdiv(s.K, 64);
    const int b = dot ? tk + (s.dprev ? cdiv((int64_t)s.rows * s.K, 256) : 0)
                      : cdiv((int64_t)cdiv(N, 32) * tk, 4) + (s.dprev ? cdiv(s.rows, 128) * tk : 0);
    blocks = b > blocks ? b : blocks;
  }
  if (blocks == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  if (dot) MLP_LAUNCH_ACT(mlp_dot_bwd_kernel, act_prev, dim3(blocks, 1, G), st, a);
  else MLP_LAUNCH_TILE(mlp_bwd_kernel, bf16, act_prev, dim3(blocks, 1, G), st, a);
  return 0;
}
extern "C" int s2p_mlp_linear_bwd(const s2p_mlp_bwd_group* groups, int G, int N, int act_prev, void* stream) {
  return mlp_bwd("s2p_mlp_linear_bwd", false, groups, G, N, act_prev, stream);
}
extern "C" int s2p_mlp_linear_bwd_bf16(const s2p_mlp_bwd_group* groups, int G, int N, int act_prev, void* stream) {
  return mlp_bwd("s2p_mlp_linear_bwd_bf16", true, groups, G, N, act_prev, stream);
}

static int mlp_dgrad(const char* who, bool bf16, const s2p_mlp_bwd_group* groups, int G, int N, int act_prev, void* stream) {
  if (const int h = mlp_header(who, groups, G, N, act_prev); h <= 0) return h;
  if (bf16) if (int rc = mlp_bf16_wide(who, N)) return rc;
  const bool dot = N <= MLP_DOT_MAX_N;
  if (!dot && N % 4) S2P_FAIL(-1, "%s: N above %d must be a multiple of 4 (N %d)", who, MLP_DOT_MAX_N, N);
  MlpBwdArgs a{};
  int blocks = 0;
  for (int g = 0; g < G; ++g) {
    const s2p_mlp_bwd_group& s = groups[g];
    if (int rc = mlp_bwd_group(who, g, s, N, act_prev, false, !dot, &a.g[g])) return rc;
    if (a.g[g].B == 0) continue;
    const int b = dot ? cdiv((int64_t)s.rows * s.K, 256) : cdiv(s.rows, 128) * cdiv(s.K, 64);
    blocks = b > blocks ? b : blocks;
  }
  if (blocks == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  if (dot) MLP_LAUNCH_ACT(mlp_dot_dgrad_kernel, act_prev, dim3(blocks, 1, G), st, a);
  else MLP_LAUNCH_TILE(mlp_dgrad_kernel, bf16, act_prev, dim3(blocks, 1, G), st, a);
  return 0;
}
extern "C" int s2p_mlp_linear_dgrad(const s2p_mlp_bwd_group* groups, int G, int N, int act_prev, void* stream) {
  return mlp_dgrad("s2p_mlp_linear_dgrad", false, groups, G, N, act_prev, stream);
}
extern "C" int s2p_mlp_linear_dgrad_bf16(const s2p_mlp_bwd_group* groups, int G, int N, int act_prev, void* stream) {
  return mlp_dgrad("s2p_mlp_linear_dgrad_bf16", true, groups, G, N, act_prev, stream);
}

static inline size_t mlp_split_floats(const s2p_mlp_bwd_group& s, int N, int S) {
  return (s.rows <= 0 || s.K <= 0) ? 0 : (size_t)S * ((size_t)N * s.K + N);
}
extern "C" size_t s2p_mlp_linear_bwd_split_workspace(const s2p_mlp_bwd_group* groups, int G, int N, int S) {
  if (!groups || G <= 0 || G > MLP_MAX_G || N <= MLP_DOT_MAX_N || N % 4 || S < 1 || S > 64) return 0;
  size_t n = 0;
  for (int g = 0; g < G; ++g) n += mlp_split_floats(groups[g], N, S);
  return n * sizeof(float);
}
static int mlp_bwd_split(const char* who, bool bf16, const s2p_mlp_bwd_group* groups, int G, int N, int act_prev, int S, void* workspace,
                         size_t workspace_bytes, void* stream) {
  if (const int h = mlp_header(who, groups, G, N, act_prev); h <= 0) return h;
  if (S < 1 || S > 64) S2P_FAIL(-1, "%s: S must be in [1, 64] (S %d)", who, S);
  if (N <= MLP_DOT_MAX_N || N % 4) S2P_FAIL(-1, "%s: the MFMA-tile form only: N above %d and a multiple of 4 (N %d)", who, MLP_DOT_MAX_N, N);
  MlpSplitArgs a{};
  a.S = S;
  int blocks = 0, sum_blocks = 0;
  size_t off = 0;
  for (int g = 0; g < G; ++g) {
    const s2p_mlp_bwd_group& s = groups[g];
    if (int rc = mlp_bwd_group(who, g, s, N, act_prev, true, true, &a.g[g])) return rc;
    if (a.g[g].B == 0) continue;
    if (!workspace) S2P_FAIL(-1, "%s: null workspace", who);
    a.ws[g] = (float*)workspace + off;
    a.chunk[g] = cdiv(cdiv(s.rows, S), 16) * 16;             // a multiple of the tile's row step; the last chunk is the shorter one
    off += mlp_split_floats(s, N, S);
    const int tk = cdiv(s.K, 64);
    const int b = cdiv((int64_t)cdiv(N, 32) * tk, 4) * S + (s.dprev ? cdiv(s.rows, 128) * tk : 0);
    blocks = b > blocks ? b : blocks;
    const int sb = cdiv((int64_t)N * s.K + N, 256);
    sum_blocks = sb > sum_blocks ? sb : sum_blocks;
  }
  if (blocks == 0) return 0;
  if (workspace_bytes < off * sizeof(float))
    S2P_FAIL(-1, "%s: workspace of %zu bytes, %zu needed (s2p_mlp_linear_bwd_split_workspace)", who, workspace_bytes, off * sizeof(float));
  const hipStream_t st = (hipStream_t)stream;
  MLP_LAUNCH_TILE(mlp_bwd_split_kernel, bf16, act_prev, dim3(blocks, 1, G), st, a);
  hipLaunchKernelGGL(mlp_split_sum_kernel, dim3(sum_blocks, 1, G), dim3(256), 0, st, a);
  S2P_CHECK_LAUNCH("mlp_split_sum_kernel");
  return 0;
}
extern "C" int s2p_mlp_linear_bwd_split(const s2p_mlp_bwd_group* groups, int G, int N, int act_prev, int S, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  return mlp_bwd_split("s2p_mlp_linear_bwd_split", false, groups, G, N, act_prev, S, workspace, workspace_bytes, stream);
}
extern "C" int s2p_mlp_linear_bwd_split_bf16(const s2p_mlp_bwd_group* groups, int G, int N, int act_prev, int S, void* workspace,
                                             size_t workspace_bytes, void* stream) {
  return mlp_bwd_split("s2p_mlp_linear_bwd_split_bf16", true, groups, G, N, act_prev, S, workspace, workspace_bytes, stream);
}
