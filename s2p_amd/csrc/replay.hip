// SLAC sequence replay buffer: sampled window ids -> the frames of those windows, straight out of a device-resident uint8 frame pool
// (SPEC.md N3c).  One launch reads every source byte once and writes both forms the latent model consumes: the encoder's NHWC input
// in the compute dtype (u8 / 255, zero-padded pitch) and the uint8 frames the image loss takes as its target.
#include "s2p_common.h"

// Frame (b, t) of the output is block-uniform: blockIdx.y = t, blockIdx.z strides over b, so the window id, the table entry and the
// slot check are scalar work once per workgroup and a thread's only index is its position inside the frame (no division anywhere).
// A slot outside [0, n_slots) is never dereferenced: the frame reads as zeros.  All byte offsets are 64-bit (a production pool of
// 100 k frames of 30 000 B is 3 GB).

// C == 3, frame_pixels % 4 == 0, pool / u8_out 4-byte aligned, pitch a whole number of 16-byte chunks: a thread step moves 4 pixels =
// 3 dwords in, 3 dwords (u8_out) and 4 * chunks 16-byte stores (x) out.  Every frame starts on a dword: slot * frame_pixels * 3 is a
// multiple of 12.
template <typename T>
__global__ __launch_bounds__(256) void window_gather_rgb4_kernel(const unsigned char* pool, long long n_slots, long long quads,
                                                                 const int* table, int Tn, const long long* win, int B, T* x,
                                                                 int chunks, unsigned char* u8o) {
  constexpr int CE = DT<T>::CE;
  const int t = blockIdx.y;
  for (int b = blockIdx.z; b < B; b += gridDim.z) {
    const long long slot = table[win[b] * Tn + t];
    const bool ok = slot >= 0 && slot < n_slots;
    const size_t f = (size_t)b * Tn + t;
    const unsigned* src = (const unsigned*)(pool + (size_t)(ok ? slot : 0) * (size_t)quads * 12);
    unsigned* d8 = (unsigned*)(u8o + f * (size_t)quads * 12);
    T* dx = x + f * (size_t)quads * 4 * chunks * CE;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long long)gridDim.x * 256) {
      unsigned d[3] = {0u, 0u, 0u};
      if (ok) { d[0] = src[3 * q]; d[1] = src[3 * q + 1]; d[2] = src[3 * q + 2]; }
      if (u8o) { d8[3 * q] = d[0]; d8[3 * q + 1] = d[1]; d8[3 * q + 2] = d[2]; }
      if (x) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {                         // pixel k: bytes 3k .. 3k+2 of the 12
          float v[CE];
#pragma unroll
          for (int e = 0; e < CE; ++e) v[e] = 0.f;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int byte = 3 * k + c;
            v[c] = (float)((d[byte >> 2] >> (8 * (byte & 3))) & 0xffu) / 255.0f;      // true division: 255 -> exactly 1.0
          }
          Chunk<T> o; o.pack(v);
          T* px = dx + (size_t)(4 * q + k) * chunks * CE;
          *(u32x4*)px = o.raw;
          for (int ch = 1; ch < chunks; ++ch) *(u32x4*)(px + ch * CE) = (u32x4){0u, 0u, 0u, 0u};
        }
      }
    }
  }
}

// any C, any frame size, any alignment of a frame inside the pool: one thread per pixel, bytes in, elements out
template <typename T>
__global__ __launch_bounds__(256) void window_gather_kernel(const unsigned char* pool, long long n_slots, long long fp, int C,
                                                            const int* table, int Tn, const long long* win, int B, T* x, int pitch,
                                                            unsigned char* u8o) {
  const int t = blockIdx.y;
  for (int b = blockIdx.z; b < B; b += gridDim.z) {
    const long long slot = table[win[b] * Tn + t];
    const bool ok = slot >= 0 && slot < n_slots;
    const size_t f = (size_t)b * Tn + t;
    const unsigned char* src = pool + (size_t)(ok ? slot : 0) * (size_t)fp * C;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < fp; p += (long long)gridDim.x * 256) {
      const size_t op = f * (size_t)fp + p;
      for (int c = 0; c < C; ++c) {
        const unsigned char v = ok ? src[(size_t)p * C + c] : (unsigned char)0;
        if (u8o) u8o[op * C + c] = v;
        if (x) x[op * pitch + c] = from_f32<T>((float)v / 255.0f);
      }
      if (x) for (int c = C; c < pitch; ++c) x[op * pitch + c] = from_f32<T>(0.f);
    }
  }
}

template <typename T>
static void launch_gather(const void* pool, int64_t n_slots, int64_t fp, int C, const int32_t* table, int T_, const int64_t* win, int B,
                          void* x, int x_pitch, void* u8_out, hipStream_t st) {
  constexpr int CE = DT<T>::CE;
  const bool fast = C == 3 && fp % 4 == 0 && (!x || x_pitch % CE == 0) && (((uintptr_t)pool | (uintptr_t)u8_out) & 3) == 0;
  const long long items = fast ? fp / 4 : fp;                 // thread steps per frame
  long long gx = (items + 255) / 256; if (gx > 64) gx = 64;
  const dim3 grid((unsigned)gx, (unsigned)T_, (unsigned)(B < 65535 ? B : 65535));
  if (fast)
    hipLaunchKernelGGL(window_gather_rgb4_kernel<T>, grid, dim3(256), 0, st, (const unsigned char*)pool, (long long)n_slots, items, table,
                       T_, (const long long*)win, B, (T*)x, x_pitch / CE, (unsigned char*)u8_out);
  else
    hipLaunchKernelGGL(window_gather_kernel<T>, grid, dim3(256), 0, st, (const unsigned char*)pool, (long long)n_slots, (long long)fp, C,
                       table, T_, (const long long*)win, B, (T*)x, x_pitch, (unsigned char*)u8_out);
}

extern "C" int s2p_window_gather_u8(int dtype, const void* pool, int64_t n_slots, int64_t frame_pixels, int C, const int32_t* table, int T,
                                    const int64_t* win, int B, void* x, int x_pitch, void* u8_out, void* stream) {
  S2P_REQUIRE(s2p_is_dtype(dtype), "s2p_window_gather_u8: bad dtype");
  S2P_REQUIRE(n_slots >= 0 && frame_pixels >= 0 && C >= 0 && T >= 0 && B >= 0 && x_pitch >= 0, "s2p_window_gather_u8: negative size");
  S2P_REQUIRE(T <= 65535, "s2p_window_gather_u8: at most 65535 frames per window");
  if ((long long)B * T == 0 || frame_pixels == 0) return 0;            // nothing to gather: no pointer is looked at
  S2P_REQUIRE(x || u8_out, "s2p_window_gather_u8: both outputs are null");
  S2P_REQUIRE(!x || C <= x_pitch, "s2p_window_gather_u8: channels exceed pitch");
  if ((x ? x_pitch : C) == 0) return 0;
  S2P_REQUIRE(pool && table && win, "s2p_window_gather_u8: null pointer");
  S2P_REQUIRE(s2p_al16(x), "s2p_window_gather_u8: x must be 16-byte aligned");
  s2p_with_dtype(dtype, [&](auto tag) {
    launch_gather<decltype(tag)>(pool, n_slots, frame_pixels, C, table, T, win, B, x, x_pitch, u8_out, (hipStream_t)stream); });
  S2P_CHECK_LAUNCH("window_gather_kernel");
  return 0;
}

// Decoded frame -> observed frame (SPEC.md N3o): the decoder's NHWC output becomes the frame an environment would have handed out, in
// the two forms the gather above writes -- the encoder's NHWC input and the uint8 frame -- so an imagined frame reaches the encoder
// with the bits the same frame has coming out of the replay buffer.  One value: the byte is clamp(rintf(v * 255), 0, 255) (one fp32
// multiply, ties to even; NaN and -0.0 give byte 0), x holds that byte / 255.0f as the gather forms it or, clamp-only, min(max(v, 0), 1)
// with NaN and -0.0 as +0.
__device__ __forceinline__ unsigned decoded_byte(float v) {
  const float r = rintf(v * 255.0f);
  const float lo = r > 0.f ? r : 0.f;                         // (NaN compares false: 0)
  return (unsigned)(lo < 255.f ? lo : 255.f);
}
__device__ __forceinline__ float decoded_value(float v, unsigned q, bool quantize) {
  if (quantize) return (float)q / 255.0f;                     // true division: 255 -> exactly 1.0
  const float lo = v > 0.f ? v : 0.f;
  return lo < 1.f ? lo : 1.f;
}

// C == 3, pixels % 4 == 0, both pitches whole numbers of 16-byte chunks, y / x 16-byte and u8_out 4-byte aligned: a thread step moves
// 4 pixels = 4 16-byte loads (the chunk that holds the three channels), 4 * chunks 16-byte stores (x) and 3 dwords (u8_out).
template <typename T>
__global__ __launch_bounds__(256) void decoded_frames_rgb4_kernel(const T* y, int ychunks, long long quads, int quantize, T* x, int xchunks,
                                                                  unsigned char* u8o) {
  constexpr int CE = DT<T>::CE;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long long)gridDim.x * 256) {
    Chunk<T> in[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) in[k].raw = *(const u32x4*)(y + (size_t)(4 * q + k) * ychunks * CE);
    unsigned d[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; ++k) {                             // pixel k: bytes 3k .. 3k+2 of the 12
      float v[CE];
#pragma unroll
      for (int e = 0; e < CE; ++e) v[e] = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float s = in[k].get(c);
        const unsigned b = decoded_byte(s);
        const int byte = 3 * k + c;
        d[byte >> 2] |= b << (8 * (byte & 3));
        v[c] = decoded_value(s, b, quantize != 0);
      }
      if (x) {
        Chunk<T> o; o.pack(v);
        T* px = x + (size_t)(4 * q + k) * xchunks * CE;
        *(u32x4*)px = o.raw;
        for (int ch = 1; ch < xchunks; ++ch) *(u32x4*)(px + ch * CE) = (u32x4){0u, 0u, 0u, 0u};
      }
    }
    if (u8o) {
      unsigned* d8 = (unsigned*)(u8o + (size_t)q * 12);
      d8[0] = d[0]; d8[1] = d[1]; d8[2] = d[2];
    }
  }
}

// any C, any pixel count, any pitches, any alignment of u8_out: one thread per pixel, elements in, elements and bytes out
template <typename T>
__global__ __launch_bounds__(256) void decoded_frames_kernel(const T* y, int y_pitch, long long pixels, int C, int quantize, T* x,
                                                             int x_pitch, unsigned char* u8o) {
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < pixels; p += (long long)gridDim.x * 256) {
    for (int c = 0; c < C; ++c) {
      const float s = to_f32(y[(size_t)p * y_pitch + c]);
      const unsigned b = decoded_byte(s);
      if (u8o) u8o[(size_t)p * C + c] = (unsigned char)b;
      if (x) x[(size_t)p * x_pitch + c] = from_f32<T>(decoded_value(s, b, quantize != 0));
    }
    if (x) for (int c = C; c < x_pitch; ++c) x[(size_t)p * x_pitch + c] = from_f32<T>(0.f);
  }
}

extern "C" int s2p_decoded_to_frames(int dtype, const void* y, int y_pitch, int64_t pixels_total, int C, int quantize, void* x,
                                     int x_pitch, void* u8_out, void* stream) {
  S2P_REQUIRE(s2p_is_dtype(dtype), "s2p_decoded_to_frames: bad dtype");
  S2P_REQUIRE(y_pitch >= 0 && pixels_total >= 0 && x_pitch >= 0, "s2p_decoded_to_frames: negative size");
  S2P_REQUIRE(C >= 1, "s2p_decoded_to_frames: C < 1");
  if (pixels_total == 0) return 0;                                     // nothing to convert: no pointer is looked at
  S2P_REQUIRE(y, "s2p_decoded_to_frames: null y");
  S2P_REQUIRE(x || u8_out, "s2p_decoded_to_frames: both outputs are null");
  S2P_REQUIRE(C <= y_pitch && (!x || C <= x_pitch), "s2p_decoded_to_frames: channels exceed pitch");
  S2P_REQUIRE(s2p_al16(x), "s2p_decoded_to_frames: x must be 16-byte aligned");
  const int ce = s2p_chunk_elems(dtype);
  S2P_REQUIRE(((uintptr_t)y & (uintptr_t)(16 / ce - 1)) == 0, "s2p_decoded_to_frames: y must be aligned to its element size");
  const bool fast = C == 3 && pixels_total % 4 == 0 && y_pitch % ce == 0 && (!x || x_pitch % ce == 0) && s2p_al16(y) &&
                    ((uintptr_t)u8_out & 3) == 0;
  const long long items = fast ? pixels_total / 4 : pixels_total;     // thread steps
  long long gx = (items + 255) / 256; if (gx > (1 << 20)) gx = 1 << 20;
  hipStream_t st = (hipStream_t)stream;
  s2p_with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    if (fast)
      hipLaunchKernelGGL(decoded_frames_rgb4_kernel<T>, dim3((unsigned)gx), dim3(256), 0, st, (const T*)y, y_pitch / ce, items, quantize,
                         (T*)x, x_pitch / ce, (unsigned char*)u8_out);
    else
      hipLaunchKernelGGL(decoded_frames_kernel<T>, dim3((unsigned)gx), dim3(256), 0, st, (const T*)y, y_pitch, (long long)pixels_total, C,
                         quantize, (T*)x, x_pitch, (unsigned char*)u8_out);
  });
  S2P_CHECK_LAUNCH("decoded_frames_kernel");
  return 0;
}

// Cached encoder features (SPEC.md N3g): sampled window ids -> everything a frozen-encoder RL step reads, out of a feature table
// that holds one row of F floats per pool slot.  Row (b, t) is block-uniform as above (blockIdx.y = t, blockIdx.z strides over b):
// the table lookup and the slot check are scalar work, a lane owns one 16-byte chunk of the row, reads it once and stores it to up
// to three places: feature_[b][t], fa[b] at feature t (t <= T-2) and next_fa[b] at feature t-1 (t >= 1).  The first block of t == 0
// also copies the window's actions (action_seq, the action columns of fa / next_fa, action_last), zeroes the pad columns and picks
// the last reward / terminal.  No division in the per-thread path; a slot outside [0, n_slots) reads as a zero row.
__global__ __launch_bounds__(64) void feature_window_gather_kernel(const float* feat, long long n_slots, int feat_pitch, int F4,
                                                                   const int* table, int Tn, const long long* win, int B,
                                                                   const float* action_, const float* reward_, const float* done_,
                                                                   int A, float* feature_, float* fa, float* next_fa, int fa_pitch,
                                                                   float* action_seq, float* action_last, int action_last_pitch,
                                                                   float* reward, float* terminal) {
  const int t = blockIdx.y;
  const int F = 4 * F4;
  for (int b = blockIdx.z; b < B; b += gridDim.z) {
    const long long w = win[b];
    const long long slot = table[w * Tn + t];
    const bool ok = slot >= 0 && slot < n_slots;
    const u32x4* src = (const u32x4*)(feat + (size_t)(ok ? slot : 0) * (size_t)feat_pitch);
    u32x4* d0 = feature_ ? (u32x4*)(feature_ + ((size_t)b * Tn + t) * (size_t)F) : nullptr;
    u32x4* d1 = fa && t < Tn - 1 ? (u32x4*)(fa + (size_t)b * fa_pitch + (size_t)t * F) : nullptr;
    u32x4* d2 = next_fa && t > 0 ? (u32x4*)(next_fa + (size_t)b * fa_pitch + (size_t)(t - 1) * F) : nullptr;
    for (int q = blockIdx.x * 64 + threadIdx.x; q < F4; q += gridDim.x * 64) {
      const u32x4 v = ok ? src[q] : (u32x4){0u, 0u, 0u, 0u};
      if (d0) d0[q] = v;
      if (d1) d1[q] = v;
      if (d2) d2[q] = v;
    }
    if (t == 0 && blockIdx.x == 0) {
      const int S = Tn - 1;                                   // actions per window; the policy input holds S - 1 of them
      const int na = S * A, nfa = na - A;
      const float* a = action_ + (size_t)w * na;              // (never formed into a load when action_ is null: the launcher checks)
      const size_t cols = (size_t)S * F;                      // feature columns of fa / next_fa
      if (action_)
        for (int j = threadIdx.x; j < na; j += 64) {
          const float v = a[j];
          if (action_seq) action_seq[(size_t)b * na + j] = v;
          if (fa && j < nfa) fa[(size_t)b * fa_pitch + cols + j] = v;
          if (next_fa && j >= A) next_fa[(size_t)b * fa_pitch + cols + (j - A)] = v;
        }
      if (fa || next_fa)
        for (size_t j = cols + nfa + threadIdx.x; j < (size_t)fa_pitch; j += 64) {
          if (fa) fa[(size_t)b * fa_pitch + j] = 0.f;
          if (next_fa) next_fa[(size_t)b * fa_pitch + j] = 0.f;
        }
      if (action_last)
        for (int j = threadIdx.x; j < action_last_pitch; j += 64) action_last[(size_t)b * action_last_pitch + j] = j < A ? a[nfa + j] : 0.f;
      if (threadIdx.x == 0) {
        if (reward) reward[b] = reward_[(size_t)w * S + (S - 1)];
        if (terminal) terminal[b] = done_[(size_t)w * S + (S - 1)];
      }
    }
  }
}

extern "C" int s2p_feature_window_gather(const float* feat, int64_t n_slots, int feat_pitch, int F, const int32_t* table, int T,
                                         const int64_t* win, int B, const float* action_, const float* reward_, const float* done_,
                                         int A, float* feature_, float* fa, float* next_fa, int fa_pitch, float* action_seq,
                                         float* action_last, int action_last_pitch, float* reward, float* terminal, void* stream) {
  S2P_REQUIRE(n_slots >= 0 && feat_pitch >= 0 && F >= 0 && T >= 0 && B >= 0 && A >= 0 && fa_pitch >= 0 && action_last_pitch >= 0,
              "s2p_feature_window_gather: negative size");
  S2P_REQUIRE(T <= 65535, "s2p_feature_window_gather: at most 65535 frames per window");
  if ((long long)B * T == 0) return 0;                                 // nothing to gather: no pointer is looked at
  S2P_REQUIRE(feature_ || fa || next_fa || action_seq || action_last || reward || terminal, "s2p_feature_window_gather: every output is null");
  S2P_REQUIRE(T >= 2, "s2p_feature_window_gather: a window holds at least 2 frames (T = S + 1)");
  S2P_REQUIRE(F % 4 == 0 && feat_pitch % 4 == 0 && feat_pitch >= F, "s2p_feature_window_gather: F and feat_pitch are multiples of 4, feat_pitch >= F");
  S2P_REQUIRE(table && win, "s2p_feature_window_gather: null pointer");
  const bool rows = feature_ || fa || next_fa;
  S2P_REQUIRE(!rows || F == 0 || feat, "s2p_feature_window_gather: null feature table");
  S2P_REQUIRE(s2p_al16(feat, feature_, fa, next_fa),
              "s2p_feature_window_gather: feat, feature_, fa and next_fa must be 16-byte aligned");
  if (fa || next_fa)
    S2P_REQUIRE(fa_pitch % 4 == 0 && (long long)(T - 1) * F + (long long)(T - 2) * A <= fa_pitch,
                "s2p_feature_window_gather: fa_pitch is a multiple of 4 and at least (T-1) F + (T-2) A");
  S2P_REQUIRE(!action_last || A <= action_last_pitch, "s2p_feature_window_gather: A exceeds action_last_pitch");
  S2P_REQUIRE((long long)(T - 1) * A <= 0x7fffffffLL, "s2p_feature_window_gather: (T-1) A exceeds 2^31");
  const bool acts = A > 0 && (action_seq || action_last || ((fa || next_fa) && T > 2));
  S2P_REQUIRE(!acts || action_, "s2p_feature_window_gather: null action_");
  S2P_REQUIRE((!reward || reward_) && (!terminal || done_), "s2p_feature_window_gather: null reward_ / done_");
  const int F4 = F / 4;
  int gx = (F4 + 63) / 64; if (gx > 64) gx = 64; if (gx < 1) gx = 1;
  const dim3 grid((unsigned)gx, (unsigned)T, (unsigned)(B < 65535 ? B : 65535));
  hipLaunchKernelGGL(feature_window_gather_kernel, grid, dim3(64), 0, (hipStream_t)stream, feat, (long long)n_slots, feat_pitch, F4, table, T,
                     (const long long*)win, B, action_, reward_, done_, A, feature_, fa, next_fa, fa_pitch, action_seq, action_last,
                     action_last_pitch, reward, terminal);
  S2P_CHECK_LAUNCH("feature_window_gather_kernel");
  return 0;
}

// S2P training set (SPEC.md N1d): frame numbers t -> the (previous image, next image, next state) triples of those frames, out of the
// dataset's uint8 NHWC frames and fp32 states as stored, in the form the generator's train step takes: fp32 NCHW in [-1,1], nearest-
// resized to out_h x out_w.  This is S2PDataset.__getitem__ + the default collate, bit for bit.  Output frame (b, which) is block-uniform:
// blockIdx.y = which (0: frame t -> prev, 1: frame t+1 -> image), blockIdx.z strides over b, so the index load and its range check are
// scalar work once per workgroup.  A row with t < 0 or t + 1 >= n_frames is never dereferenced: all its outputs are zeros.

// (float)u8 / 127.5f - 1.0f with the quotient and the difference rounded on their own, as torch's `.float() / 127.5 - 1.0` does: the
// quotient passes through a register the compiler cannot see through, so it can neither fold the division into the subtraction nor
// replace it by a multiplication
__device__ __forceinline__ float pair_value(unsigned byte) {
  float q = (float)byte / 127.5f;
  asm volatile("" : "+v"(q));
  return q - 1.0f;
}
// torch's `nearest` source index: min((int)floorf(dst * scale), size - 1), scale = (float)in / (float)out formed by the launcher
__device__ __forceinline__ int pair_nearest(int dst, float scale, int size) {
  const int s = (int)floorf((float)dst * scale);
  return s < size - 1 ? s : size - 1;
}
__device__ __forceinline__ void pair_copy_state(const float* states, int S, long long t, bool ok, float* state, int b) {
  for (int j = threadIdx.x; j < S; j += 256) state[(size_t)b * S + j] = ok ? states[(size_t)(t + 1) * S + j] : 0.f;
}

// C == 3, out_w % 4 == 0, a frame a whole number of dwords in a 4-byte aligned pool, 16-byte aligned outputs, frames below 2^31 bytes:
// a thread step makes 4 neighbouring output pixels of a row = one 16-byte store into each of the three planes.  RESIZE false (out ==
// source size): the 12 source bytes are 3 whole dwords and the quad number is both offsets, no division.  RESIZE true: a pixel's 3
// bytes are cut out of the 2 dwords that hold them (the second index is clamped to the frame: it is then not needed).
template <bool RESIZE>
__global__ __launch_bounds__(256) void frame_pair_rgb4_kernel(const unsigned char* pool, long long n_frames, int H, int W,
                                                              const float* states, int S, const long long* idx, int B, int oh, int ow,
                                                              float sh, float sw, float* prev, float* image, float* state) {
  const int which = blockIdx.y;
  const unsigned quads = (unsigned)oh * (unsigned)ow / 4u, qw = (unsigned)ow / 4u;
  const size_t plane = (size_t)oh * ow;
  const unsigned frame_dwords = (unsigned)H * (unsigned)W * 3u / 4u;
  for (int b = blockIdx.z; b < B; b += gridDim.z) {
    const long long t = idx[b];
    const bool ok = t >= 0 && t < n_frames - 1;                   // (t + 1 could overflow)
    if (state && which == 0 && blockIdx.x == 0) pair_copy_state(states, S, t, ok, state, b);
    const unsigned* src = (const unsigned*)(pool + (size_t)(ok ? t + which : 0) * (size_t)frame_dwords * 4);
    float* dst = (which ? image : prev) + (size_t)b * 3 * plane;
    for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < quads; q += gridDim.x * 256u) {
      f32x4 o[3];
      if (!ok) {
        o[0] = o[1] = o[2] = (f32x4){0.f, 0.f, 0.f, 0.f};
      } else if (!RESIZE) {
        const unsigned d[3] = {src[3 * q], src[3 * q + 1], src[3 * q + 2]};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int byte = 3 * k + c;
            o[c][k] = pair_value((d[byte >> 2] >> (8 * (byte & 3))) & 0xffu);
          }
      } else {
        const unsigned y = q / qw, x0 = (q - y * qw) * 4u;
        const unsigned row = (unsigned)pair_nearest((int)y, sh, H) * (unsigned)W;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned at = (row + (unsigned)pair_nearest((int)(x0 + k), sw, W)) * 3u;      // first byte of the source pixel
          const unsigned i0 = at >> 2, i1 = i0 + 1 < frame_dwords ? i0 + 1 : frame_dwords - 1;
          const unsigned long long two = ((unsigned long long)src[i1] << 32) | src[i0];
          const unsigned px = (unsigned)(two >> (8 * (at & 3u)));
#pragma unroll
          for (int c = 0; c < 3; ++c) o[c][k] = pair_value((px >> (8 * c)) & 0xffu);
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) *(f32x4*)(dst + c * plane + (size_t)q * 4) = o[c];
    }
  }
}

// any C, any sizes, any alignment of the pool, 4-byte aligned outputs: one thread per output pixel, bytes in, one float per plane out
__global__ __launch_bounds__(256) void frame_pair_kernel(const unsigned char* pool, long long n_frames, int H, int W, int C,
                                                         const float* states, int S, const long long* idx, int B, int oh, int ow,
                                                         float sh, float sw, float* prev, float* image, float* state) {
  const int which = blockIdx.y;
  const long long plane = (long long)oh * ow;
  for (int b = blockIdx.z; b < B; b += gridDim.z) {
    const long long t = idx[b];
    const bool ok = t >= 0 && t < n_frames - 1;                   // (t + 1 could overflow)
    if (state && which == 0 && blockIdx.x == 0) pair_copy_state(states, S, t, ok, state, b);
    const unsigned char* src = pool + (size_t)(ok ? t + which : 0) * (size_t)H * (size_t)W * (size_t)C;
    float* dst = (which ? image : prev) + (size_t)b * (size_t)C * (size_t)plane;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < plane; p += (long long)gridDim.x * 256) {
      const int y = (int)(p / ow), x = (int)(p - (long long)y * ow);
      const size_t at = ((size_t)pair_nearest(y, sh, H) * (size_t)W + (size_t)pair_nearest(x, sw, W)) * (size_t)C;
      for (int c = 0; c < C; ++c) dst[(size_t)c * plane + p] = ok ? pair_value(src[at + c]) : 0.f;
    }
  }
}

extern "C" int s2p_frame_pair_gather(const void* pool, int64_t n_frames, int H, int W, int C, const float* states, int S,
                                     const int64_t* idx, int B, int out_h, int out_w, float* prev, float* image, float* state,
                                     void* stream) {
  S2P_REQUIRE(n_frames >= 0 && H >= 0 && W >= 0 && S >= 0 && B >= 0 && out_h >= 0 && out_w >= 0, "s2p_frame_pair_gather: negative size");
  S2P_REQUIRE(C >= 1, "s2p_frame_pair_gather: C < 1");
  if (B == 0) return 0;                                                // nothing to gather: no pointer is looked at
  S2P_REQUIRE(H >= 1 && W >= 1 && out_h >= 1 && out_w >= 1, "s2p_frame_pair_gather: empty frame");
  S2P_REQUIRE(pool && idx && prev, "s2p_frame_pair_gather: null pointer (pool, idx and prev are required)");
  if (S == 0) state = nullptr;
  S2P_REQUIRE(!state || states, "s2p_frame_pair_gather: null states");
  S2P_REQUIRE((((uintptr_t)prev | (uintptr_t)image | (uintptr_t)state | (uintptr_t)states) & 3) == 0,
              "s2p_frame_pair_gather: prev, image, state and states must be 4-byte aligned");
  const long long frame_bytes = (long long)H * W * C, plane = (long long)out_h * out_w;
  const bool same = out_h == H && out_w == W;
  const bool fast = C == 3 && out_w % 4 == 0 && frame_bytes % 4 == 0 && frame_bytes < 0x7fffffffLL && plane < 0x7fffffffLL &&
                    ((uintptr_t)pool & 3) == 0 && s2p_al16(prev, image);
  const float sh = (float)H / (float)out_h, sw = (float)W / (float)out_w;       // torch's scales: fp32 quotients
  const long long items = fast ? plane / 4 : plane;                   // thread steps per frame
  long long gx = (items + 255) / 256; if (gx > 64) gx = 64;
  const dim3 grid((unsigned)gx, image ? 2u : 1u, (unsigned)(B < 65535 ? B : 65535));
  const unsigned char* p8 = (const unsigned char*)pool;
  const long long* ix = (const long long*)idx;
  hipStream_t st = (hipStream_t)stream;
  if (fast && same)
    hipLaunchKernelGGL(frame_pair_rgb4_kernel<false>, grid, dim3(256), 0, st, p8, (long long)n_frames, H, W, states, S, ix, B, out_h, out_w,
                       sh, sw, prev, image, state);
  else if (fast)
    hipLaunchKernelGGL(frame_pair_rgb4_kernel<true>, grid, dim3(256), 0, st, p8, (long long)n_frames, H, W, states, S, ix, B, out_h, out_w,
                       sh, sw, prev, image, state);
  else
    hipLaunchKernelGGL(frame_pair_kernel, grid, dim3(256), 0, st, p8, (long long)n_frames, H, W, C, states, S, ix, B, out_h, out_w, sh, sw,
                       prev, image, state);
  S2P_CHECK_LAUNCH("frame_pair_kernel");
  return 0;
}
