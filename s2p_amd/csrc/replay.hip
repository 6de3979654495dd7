// SLAC sequence replay buffer: sampled window ids -> the frames of those windows, straight out of a device-resident uint8 frame pool
// (SPEC.md N3c).  One launch reads every source byte once and writes both forms the latent model consumes: the encoder's NHWC input
// in the compute dtype (u8 / 255, zero-padded pitch) and the uint8 frames the image loss takes as its target.
#include "s2p_common.h"

#define S2P_REQUIRE(cond, ...) do { if (!(cond)) S2P_FAIL(-1, __VA_ARGS__); } while (0)

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
  S2P_REQUIRE(dtype == S2P_F32 || dtype == S2P_BF16, "s2p_window_gather_u8: bad dtype");
  S2P_REQUIRE(n_slots >= 0 && frame_pixels >= 0 && C >= 0 && T >= 0 && B >= 0 && x_pitch >= 0, "s2p_window_gather_u8: negative size");
  S2P_REQUIRE(T <= 65535, "s2p_window_gather_u8: at most 65535 frames per window");
  if ((long long)B * T == 0 || frame_pixels == 0) return 0;            // nothing to gather: no pointer is looked at
  S2P_REQUIRE(x || u8_out, "s2p_window_gather_u8: both outputs are null");
  S2P_REQUIRE(!x || C <= x_pitch, "s2p_window_gather_u8: channels exceed pitch");
  if ((x ? x_pitch : C) == 0) return 0;
  S2P_REQUIRE(pool && table && win, "s2p_window_gather_u8: null pointer");
  S2P_REQUIRE(((uintptr_t)x & 15) == 0, "s2p_window_gather_u8: x must be 16-byte aligned");
  if (dtype == S2P_F32) launch_gather<float>(pool, n_slots, frame_pixels, C, table, T, win, B, x, x_pitch, u8_out, (hipStream_t)stream);
  else launch_gather<__bf16>(pool, n_slots, frame_pixels, C, table, T, win, B, x, x_pitch, u8_out, (hipStream_t)stream);
  S2P_CHECK_LAUNCH("window_gather_kernel");
  return 0;
}
