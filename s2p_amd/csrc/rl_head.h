// What the loss heads of the latent RL trainers (iql.hip, cql.hip) share.
#pragma once
#include "s2p_common.h"

// softplus without overflow on either side (SPEC.md N3b)
__device__ __forceinline__ float head_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// S sums over one workgroup of 1024 threads: red[s][t] holds thread t's share, red[s][0] the total afterwards.  A halving tree
// through LDS (a fixed order), as ens_nll_kernel adds its own.
template <int S> __device__ __forceinline__ void head_tree_sum(float (&red)[S][1024], int t) {
  for (int w = 512; w > 0; w >>= 1) {
    __syncthreads();
    if (t < w)
#pragma unroll
      for (int s = 0; s < S; ++s) red[s][t] += red[s][t + w];
  }
  __syncthreads();
}
