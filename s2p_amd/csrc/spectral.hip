// Spectral normalization (torch.nn.utils.spectral_norm semantics, n_power_iterations = 1; SPEC.md section D5s): the power iteration
// that refreshes u, v and sigma of every SN weight of a network, and the projection of dL/dW_sn onto dL/dW.  Each launch covers
// every SN layer of a network through a DEVICE job table (capture-safe, like s2p_pack_weights).
//
// W is the fp32 master [R][T][C] viewed as an R x K matrix, K = T*C (columns in the master's (tap, channel) order; the checkpoint
// code permutes v to torch's (channel, tap) order).  Deterministic: no atomics; every reduction has a fixed shape and order that
// depends only on the job's own R and K, so a job's result does not depend on the other jobs of the launch or on the grid.
//   1. sn_wtu_kernel     (training)  per 64-column chunk: a = W^T u over all R rows (16 row lanes, summed in lane order) -> ws.a,
//                                    and the chunk's sum of a^2 -> ws.pa
//   2. sn_wv_kernel                  per 8-row block: b = W v (training: v = a / max(|a|, eps), |a| summed from ws.pa by every
//                                    workgroup in the same order; the block also writes its share of v) -> ws.b, and the block's
//                                    sum of b^2 (training) or of u*b (eval) -> ws.pb
//   3. sn_finalize_kernel            one workgroup per job: training u = b / max(|b|, eps), sigma = u . b;  eval sigma = sum ws.pb
// The scaled repack (s2p_pack_weights_scaled, misc.hip) then packs W / sigma.  Projection: sn_proj_dot_kernel (per 8-row block
// sum of G*W -> ws.pg), sn_proj_apply_kernel (G = (G - (sum G*W / sigma) u v^T) / sigma, one row per workgroup).
#include "s2p_common.h"

namespace {

constexpr int SN_CB = 64;       // columns per chunk of kernel 1
constexpr int SN_RB = 8;        // rows per block of kernels 2 and the projection's dot

struct SnWs {                   // the job's workspace, carved in this order (s2p_sn_workspace_floats)
  float *a, *pa, *b, *pb, *pg;
};

__device__ __forceinline__ int sn_nck(int K) { return (K + SN_CB - 1) / SN_CB; }
__device__ __forceinline__ int sn_nrb(int R) { return (R + SN_RB - 1) / SN_RB; }

__device__ __forceinline__ SnWs sn_ws(const s2p_sn_job& j) {
  SnWs w;
  w.a = j.ws;
  w.pa = w.a + j.K;
  w.b = w.pa + sn_nck(j.K);
  w.pb = w.b + j.R;
  w.pg = w.pb + sn_nrb(j.R);
  return w;
}

__device__ __forceinline__ bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ float sn_den(float sumsq) { return fmaxf(sqrtf(sumsq), 1e-12f); }

__device__ __forceinline__ float wave_sum(float x) {           // fixed butterfly: same order on every call
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// sum over j < n of p[j], left to right (every caller that needs the same total computes it the same way)
__device__ __forceinline__ float seq_sum(const float* p, int n) {
  float s = 0.f;
  for (int i = 0; i < n; ++i) s += p[i];
  return s;
}

// ---- 1: a = W^T u ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sn_wtu_kernel(const s2p_sn_job* jobs) {
  __shared__ float red[16][SN_CB + 1];
  const s2p_sn_job j = jobs[blockIdx.y];
  const int chunk = blockIdx.x;
  if (chunk >= sn_nck(j.K)) return;
  const SnWs w = sn_ws(j);
  const int t = threadIdx.x, q = t & 15, rl = t >> 4;
  const int k0 = chunk * SN_CB + 4 * q;
  const bool vec = (j.K & 3) == 0 && al16(j.w);    // rows start 16-byte aligned and k0 < K implies k0 + 3 < K
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (k0 < j.K) {
    for (int r = rl; r < j.R; r += 16) {
      const float ur = j.u[r];
      const float* wp = j.w + (long long)r * j.K + k0;
      if (vec) {
        const f32x4 x = *(const f32x4*)wp;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += x[e] * ur;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (k0 + e < j.K) acc[e] += wp[e] * ur;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) red[rl][4 * q + e] = acc[e];
  __syncthreads();
  if (t < SN_CB) {                                 // wave 0: one column per lane
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += red[i][t];
    const int k = chunk * SN_CB + t;
    if (k < j.K) w.a[k] = s;
    const float sq = wave_sum(k < j.K ? s * s : 0.f);
    if (t == 0) w.pa[chunk] = sq;
  }
}

// ---- 2: b = W v --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sn_wv_kernel(const s2p_sn_job* jobs, int training) {
  __shared__ float part[SN_RB];
  const s2p_sn_job j = jobs[blockIdx.y];
  const int nrb = sn_nrb(j.R), rb = blockIdx.x;
  if (rb >= nrb) return;
  const SnWs w = sn_ws(j);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const float den = training ? sn_den(seq_sum(w.pa, sn_nck(j.K))) : 1.f;
  const float* vsrc = training ? w.a : j.v;
  const bool vec = (j.K & 3) == 0 && al16(j.w) && al16(vsrc);
  for (int i = wv; i < SN_RB; i += 4) {
    const int r = rb * SN_RB + i;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (r < j.R) {
      const float* wp = j.w + (long long)r * j.K;
      for (int k = 4 * lane; k < j.K; k += 256) {
        if (vec) {
          const f32x4 x = *(const f32x4*)(wp + k);
          const f32x4 y = *(const f32x4*)(vsrc + k);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] += x[e] * (training ? y[e] / den : y[e]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (k + e < j.K) acc[e] += wp[k + e] * (training ? vsrc[k + e] / den : vsrc[k + e]);
        }
      }
    }
    const float b = wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
    if (lane == 0) {
      float p = 0.f;
      if (r < j.R) {
        if (training) { w.b[r] = b; p = b * b; }
        else p = j.u[r] * b;
      }
      part[i] = p;
    }
  }
  __syncthreads();
  if (t == 0) w.pb[rb] = seq_sum(part, SN_RB);
  if (training) {                                  // this block's share of v = a / |a| (kernel 2 reads a, never v, in training)
    const int share = (j.K + nrb - 1) / nrb;
    const int lo = rb * share, hi = min(j.K, lo + share);
    for (int k = lo + t; k < hi; k += 256) j.v[k] = w.a[k] / den;
  }
}

// ---- 3: u and sigma ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sn_finalize_kernel(const s2p_sn_job* jobs, int training) {
  __shared__ float red[256];
  const s2p_sn_job j = jobs[blockIdx.y];
  const SnWs w = sn_ws(j);
  const int t = threadIdx.x;
  const float s = seq_sum(w.pb, sn_nrb(j.R));
  if (!training) {
    if (t == 0) *j.sigma = s;
    return;
  }
  const float den = sn_den(s);
  float p = 0.f;
  for (int r = t; r < j.R; r += 256) {
    const float u = w.b[r] / den;
    j.u[r] = u;
    p += u * w.b[r];
  }
  red[t] = p;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (t < h) red[t] += red[t + h];
    __syncthreads();
  }
  if (t == 0) *j.sigma = red[0];
}

// ---- projection of the gradient -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sn_proj_dot_kernel(const s2p_sn_job* jobs) {
  __shared__ float part[SN_RB];
  const s2p_sn_job j = jobs[blockIdx.y];
  const int rb = blockIdx.x;
  if (rb >= sn_nrb(j.R)) return;
  const SnWs w = sn_ws(j);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const bool vec = (j.K & 3) == 0 && al16(j.w) && al16(j.grad);
  for (int i = wv; i < SN_RB; i += 4) {
    const int r = rb * SN_RB + i;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (r < j.R) {
      const float* wp = j.w + (long long)r * j.K;
      const float* gp = j.grad + (long long)r * j.K;
      for (int k = 4 * lane; k < j.K; k += 256) {
        if (vec) {
          const f32x4 x = *(const f32x4*)(wp + k);
          const f32x4 g = *(const f32x4*)(gp + k);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] += x[e] * g[e];
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) if (k + e < j.K) acc[e] += wp[k + e] * gp[k + e];
        }
      }
    }
    const float d = wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
    if (lane == 0) part[i] = r < j.R ? d : 0.f;
  }
  __syncthreads();
  if (t == 0) w.pg[rb] = seq_sum(part, SN_RB);
}

__global__ __launch_bounds__(256) void sn_proj_apply_kernel(const s2p_sn_job* jobs) {
  const s2p_sn_job j = jobs[blockIdx.y];
  const SnWs w = sn_ws(j);
  const float sigma = *j.sigma;
  const float c = seq_sum(w.pg, sn_nrb(j.R)) / sigma;        // <G, W / sigma>
  for (int r = blockIdx.x; r < j.R; r += gridDim.x) {
    const float cu = c * j.u[r];
    float* gp = j.grad + (long long)r * j.K;
    for (int k = threadIdx.x; k < j.K; k += 256) gp[k] = (gp[k] - cu * j.v[k]) / sigma;
  }
}

}  // namespace

extern "C" int64_t s2p_sn_workspace_floats(int R, int K) {
  if (R <= 0 || K <= 0) return 0;
  const int64_t n = (int64_t)K + (K + SN_CB - 1) / SN_CB + R + 2 * ((R + SN_RB - 1) / SN_RB);
  return (n + 3) & ~(int64_t)3;                    // whole 16-byte chunks: consecutive workspaces stay aligned
}

extern "C" int s2p_sn_power_iter(const s2p_sn_job* jobs, int n_jobs, int max_R, int max_K, int training, void* stream) {
  if (!jobs || n_jobs <= 0 || max_R <= 0 || max_K <= 0) S2P_FAIL(-1, "s2p_sn_power_iter: bad argument");
  hipStream_t s = (hipStream_t)stream;
  if (training) {
    hipLaunchKernelGGL(sn_wtu_kernel, dim3((max_K + SN_CB - 1) / SN_CB, n_jobs), dim3(256), 0, s, jobs);
    S2P_CHECK_LAUNCH("sn_wtu_kernel");
  }
  hipLaunchKernelGGL(sn_wv_kernel, dim3((max_R + SN_RB - 1) / SN_RB, n_jobs), dim3(256), 0, s, jobs, training ? 1 : 0);
  S2P_CHECK_LAUNCH("sn_wv_kernel");
  hipLaunchKernelGGL(sn_finalize_kernel, dim3(1, n_jobs), dim3(256), 0, s, jobs, training ? 1 : 0);
  S2P_CHECK_LAUNCH("sn_finalize_kernel");
  return 0;
}

extern "C" int s2p_sn_project_grad(const s2p_sn_job* jobs, int n_jobs, int max_R, int max_K, void* stream) {
  if (!jobs || n_jobs <= 0 || max_R <= 0 || max_K <= 0) S2P_FAIL(-1, "s2p_sn_project_grad: bad argument");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sn_proj_dot_kernel, dim3((max_R + SN_RB - 1) / SN_RB, n_jobs), dim3(256), 0, s, jobs);
  S2P_CHECK_LAUNCH("sn_proj_dot_kernel");
  hipLaunchKernelGGL(sn_proj_apply_kernel, dim3(max_R, n_jobs), dim3(256), 0, s, jobs);
  S2P_CHECK_LAUNCH("sn_proj_apply_kernel");
  return 0;
}
