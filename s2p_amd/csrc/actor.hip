// The acting step of a SLAC policy (SPEC.md N3f): the three kernels between an environment's uint8 frame and the policy's action.
//   s2p_u8_chw_to_nhwc01     the frames an environment hands out ([N][C][H][W] uint8) -> the encoder's NHWC input, u8 / 255
//   s2p_feature_action_push  the policy-input rows ARE the observation state: shift one feature and one action in, or reset
//   s2p_mlp_linear_fwd_skinny  the grouped linear layer for rows <= 16: one wave per output column, weights read once
// All fp32 (the first writes bf16 too), no atomics, a fixed summation order.
#include "ens_tile.h"

#define ACTOR_REQUIRE(cond, ...) do { if (!(cond)) S2P_FAIL(-1, __VA_ARGS__); } while (0)
#define ACTOR_MAX_G 8                                        // (MLP_MAX_G of mlp.hip: the same group table)
#define ACTOR_MAX_ROWS 16

// ---- uint8 CHW -> NHWC in [0, 1] ------------------------------------------------------------------------------------------------
// One thread per V consecutive pixels of one frame (blockIdx.y = frame): channel plane c is read as V contiguous bytes (one dword
// for V = 4), the pixel's `pitch` elements leave as one contiguous run.  v / 255.0f is a true division: 255 -> exactly 1.0.
template <typename T, int V>
__global__ __launch_bounds__(256) void u8_chw_to_nhwc01_kernel(const unsigned char* x, int C, int HW, T* y, int pitch) {
  const int p0 = (blockIdx.x * 256 + threadIdx.x) * V;
  if (p0 >= HW) return;
  const unsigned char* xf = x + (size_t)blockIdx.y * C * HW;
  T* yf = y + ((size_t)blockIdx.y * HW + p0) * pitch;
  for (int c = 0; c < C; ++c) {
    unsigned d;
    if constexpr (V == 4) d = *(const unsigned*)(xf + (size_t)c * HW + p0);      // HW % 4 == 0, x 4-byte aligned: a dword is in or out
    else d = xf[(size_t)c * HW + p0];
#pragma unroll
    for (int v = 0; v < V; ++v) yf[(size_t)v * pitch + c] = from_f32<T>((float)((d >> (8 * v)) & 0xffu) / 255.0f);
  }
#pragma unroll
  for (int v = 0; v < V; ++v)
    for (int c = C; c < pitch; ++c) yf[(size_t)v * pitch + c] = from_f32<T>(0.f);
}

template <typename T>
static void launch_u8_chw(const void* x, int N, int C, int HW, void* y, int pitch, hipStream_t st) {
  const bool v4 = HW % 4 == 0 && ((uintptr_t)x & 3) == 0;     // (every frame then starts on a dword: C * HW is a multiple of 4)
  if (v4)
    hipLaunchKernelGGL((u8_chw_to_nhwc01_kernel<T, 4>), dim3(cdiv(HW / 4, 256), N), dim3(256), 0, st, (const unsigned char*)x, C, HW, (T*)y, pitch);
  else
    hipLaunchKernelGGL((u8_chw_to_nhwc01_kernel<T, 1>), dim3(cdiv(HW, 256), N), dim3(256), 0, st, (const unsigned char*)x, C, HW, (T*)y, pitch);
}

extern "C" int s2p_u8_chw_to_nhwc01(int dtype, const void* x, int N, int C, int H, int W, void* y, int y_pitch, void* stream) {
  const char* who = "s2p_u8_chw_to_nhwc01";
  ACTOR_REQUIRE(s2p_is_dtype(dtype), "%s: bad dtype", who);
  ACTOR_REQUIRE(N >= 0 && C >= 0 && H >= 0 && W >= 0 && y_pitch >= 0, "%s: negative size", who);
  if (N == 0 || H == 0 || W == 0 || (C == 0 && y_pitch == 0)) return 0;         // nothing to write: no pointer is looked at
  ACTOR_REQUIRE(y_pitch >= C, "%s: pitch shorter than the row (C %d, y_pitch %d)", who, C, y_pitch);
  ACTOR_REQUIRE((C == 0 || x) && y, "%s: null pointer", who);
  ACTOR_REQUIRE(N <= 65535 && (int64_t)H * W < ((int64_t)1 << 29), "%s: at most 65535 frames of fewer than 2^29 pixels", who);
  s2p_with_dtype(dtype, [&](auto tag) { launch_u8_chw<decltype(tag)>(x, N, C, H * W, y, y_pitch, (hipStream_t)stream); });
  S2P_CHECK_LAUNCH("u8_chw_to_nhwc01_kernel");
  return 0;
}

// ---- the policy-input rows as the observation state -----------------------------------------------------------------------------
// Row n = [f_0 .. f_{S-1} | a_0 .. a_{S-2} | 0 pad].  One thread per column of dst (blockIdx.y = row): every column has exactly one
// source -- a column of src one slot to the right, the new feature / action, the fill vector or zero -- chosen by the row's reset
// code, which is block-uniform.  An unknown code is treated as 0 (append).
__global__ __launch_bounds__(256) void feature_action_push_kernel(const float* src, float* dst, int pitch, int S, int F, int A,
                                                                  const float* feat, int fp, const float* action, int ap,
                                                                  const int* reset, const float* fill) {
  const int n = blockIdx.y, col = blockIdx.x * 256 + threadIdx.x;
  if (col >= pitch) return;
  const int code = reset ? reset[n] : 0, SF = S * F, P = SF + (S - 1) * A;
  const float* sr = src + (size_t)n * pitch;
  const float* fr = feat + (size_t)n * fp;
  float v = 0.f;
  if (col < SF) {
    const int f = col % F;
    if (col >= SF - F) v = fr[f];
    else if (code == 1) v = fill[f];
    else if (code == 2) v = fr[f];
    else v = sr[col + F];
  } else if (col < P && code != 1 && code != 2) {
    v = col >= P - A ? action[(size_t)n * ap + (col - (P - A))] : sr[col + A];
  }
  dst[(size_t)n * pitch + col] = v;
}

extern "C" int s2p_feature_action_push(const float* src, float* dst, int pitch, int N, int S, int F, int A, const float* feat,
                                       int feat_pitch, const float* action, int action_pitch, const int32_t* reset,
                                       const float* fill, void* stream) {
  const char* who = "s2p_feature_action_push";
  ACTOR_REQUIRE(pitch >= 0 && N >= 0 && S >= 0 && F >= 0 && A >= 0 && feat_pitch >= 0 && action_pitch >= 0, "%s: negative size", who);
  if (N == 0 || pitch == 0) return 0;                        // nothing to write: no pointer is looked at
  ACTOR_REQUIRE(S >= 1, "%s: a window holds at least one frame (S %d)", who, S);
  const int64_t P = (int64_t)S * F + (int64_t)(S - 1) * A;
  ACTOR_REQUIRE(P <= pitch && feat_pitch >= F && action_pitch >= A, "%s: pitch shorter than the row", who);
  ACTOR_REQUIRE(pitch % 4 == 0, "%s: pitch must be a multiple of 4 floats (the policy's first layer reads 16-byte groups)", who);
  ACTOR_REQUIRE(N <= 65535, "%s: at most 65535 rows", who);
  const bool need_action = S > 1 && A > 0;
  ACTOR_REQUIRE(src && dst && (F == 0 || feat) && (!need_action || action), "%s: null pointer (src, dst, feat and action are required)", who);
  ACTOR_REQUIRE(F == 0 || S == 1 || !reset || fill, "%s: reset codes need the fill vector", who);
  ACTOR_REQUIRE(s2p_al16(src) && s2p_al16(dst), "%s: src and dst must be 16-byte aligned", who);
  const float* s_end = src + (size_t)N * pitch;
  const float* d_end = dst + (size_t)N * pitch;
  ACTOR_REQUIRE(s_end <= dst || d_end <= src, "%s: src and dst overlap (the caller ping-pongs two buffers)", who);
  hipLaunchKernelGGL(feature_action_push_kernel, dim3(cdiv(pitch, 256), N), dim3(256), 0, (hipStream_t)stream, src, dst, pitch, S, F, A,
                     feat, feat_pitch, action, action_pitch, (const int*)reset, fill);
  S2P_CHECK_LAUNCH("feature_action_push_kernel");
  return 0;
}

// ---- the grouped linear layer for at most 16 rows: weight-stationary dot products -----------------------------------------------
// One wave per output column n (four per workgroup), grid z = group.  The wave reads w[n][:] ONCE: lane l takes k = 4 l .. 4 l + 3 of
// every 256, in k order (the split of mlp_dot_fwd_kernel), and keeps one accumulator per row; every accumulator then goes through
// the same 64-lane butterfly.  A row's value is a chain of fused multiply-adds over ITS x row and the weight row alone, in an
// order that does not involve the row count: the R = 1, 4 and 16 instantiations, and any row count inside one, give a row the same
// bits.  The weights never touch LDS; the x rows (at most 16 K floats) come out of L2 for every wave after the first.
struct SkinnyArgs { EnsFwdTile g[ACTOR_MAX_G]; };
template <int ACT, int R> __global__ __launch_bounds__(256) void mlp_skinny_fwd_kernel(const SkinnyArgs a) {
  const EnsFwdTile t = a.g[blockIdx.z];
  const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= t.N || t.B == 0) return;                          // (wave-uniform)
  const float* wr = t.w + (size_t)n * t.K;
  float s[R];
#pragma unroll
  for (int r = 0; r < R; ++r) s[r] = 0.f;
  for (int k = lane * 4; k < t.K; k += 256) {                // K is a multiple of 4: a float4 is in or out
    const f32x4 wv = *(const f32x4*)(wr + k);
    f32x4 xv[R];                                             // an accumulator past the group's last row reads row 0 and is never stored:
#pragma unroll                                               // no branch between the R loads, so they are all in flight together
    for (int r = 0; r < R; ++r) xv[r] = *(const f32x4*)(t.x + (size_t)(r < t.B ? r : 0) * t.xp + k);
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) s[r] = __builtin_fmaf(xv[r][c], wv[c], s[r]);
  }
  const float b = t.bias[n];
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s[r] += __shfl_xor(s[r], o, 64);
    if (lane == r && r < t.B) {                              // (every lane holds the sum: lane r stores row r)
      const float v = s[r] + b;
      const size_t o = (size_t)r * t.yp + n;
      if (t.pre) t.pre[o] = v;
      if (t.act) t.act[o] = ens_act<ACT>(v);
    }
  }
}

template <int R> static void launch_skinny(int act, dim3 grid, hipStream_t st, const SkinnyArgs& a) {
  if (act == S2P_ACT_RELU) hipLaunchKernelGGL((mlp_skinny_fwd_kernel<ENS_ACT_RELU, R>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((mlp_skinny_fwd_kernel<ENS_ACT_NONE, R>), grid, dim3(256), 0, st, a);
}

extern "C" int s2p_mlp_linear_fwd_skinny(const s2p_mlp_fwd_group* groups, int G, int N, int act, void* stream) {
  const char* who = "s2p_mlp_linear_fwd_skinny";
  ACTOR_REQUIRE(G >= 0 && N >= 0, "%s: negative size", who);
  if (G == 0 || N == 0) return 0;
  ACTOR_REQUIRE(groups, "%s: null group table", who);
  ACTOR_REQUIRE(G <= ACTOR_MAX_G, "%s: at most %d groups (G %d)", who, ACTOR_MAX_G, G);
  ACTOR_REQUIRE(act == S2P_ACT_NONE || act == S2P_ACT_RELU, "%s: activation %d (none and relu only)", who, act);
  SkinnyArgs a{};
  int rows = 0;
  for (int g = 0; g < G; ++g) {
    const s2p_mlp_fwd_group& s = groups[g];
    ACTOR_REQUIRE(s.rows >= 0 && s.K >= 0, "%s: group %d: negative size", who, g);
    ACTOR_REQUIRE(s.rows <= ACTOR_MAX_ROWS, "%s: group %d: %d rows (at most %d: s2p_mlp_linear_fwd takes more)", who, g, s.rows, ACTOR_MAX_ROWS);
    if (s.rows == 0) continue;                               // (an empty group: B = 0 in the table, no pointer looked at)
    ACTOR_REQUIRE(s.x && s.w && s.bias && (s.pre || s.act), "%s: group %d: null tensor (x, w, bias and one of pre / act are required)", who, g);
    ACTOR_REQUIRE(s.K > 0 && s.K % 4 == 0 && s.x_pitch % 4 == 0 && s2p_al16(s.x) && s2p_al16(s.w),
                  "%s: group %d: K, x_pitch must be multiples of 4 floats (K > 0), x and w 16-byte aligned", who, g);
    ACTOR_REQUIRE(s.x_pitch >= s.K && s.y_pitch >= N, "%s: group %d: pitch shorter than the row", who, g);
    a.g[g] = EnsFwdTile{s.x, s.w, s.bias, s.pre, s.act, s.x_pitch, s.y_pitch, s.rows, s.K, N};
    rows = s.rows > rows ? s.rows : rows;
  }
  if (rows == 0) return 0;
  const dim3 grid(cdiv(N, 4), 1, G);
  const hipStream_t st = (hipStream_t)stream;
  if (rows == 1) launch_skinny<1>(act, grid, st, a);
  else if (rows <= 4) launch_skinny<4>(act, grid, st, a);
  else launch_skinny<ACTOR_MAX_ROWS>(act, grid, st, a);
  S2P_CHECK_LAUNCH("mlp_skinny_fwd_kernel");
  return 0;
}
