// loss_helpers.h — device helpers shared by the loss-phase files (loss.hip, nce.hip, maps.hip): one copy of each.  They are not in common.h because
// every conv / wgrad file includes that header and none of them resizes, selects or reduces this way.
#pragma once
#include "common.h"

// bilinear source index and scale, align_corners=True (head.hip and affinity.hip keep their own forms: their arithmetic differs, see there)
__device__ __forceinline__ void src_index(int o, float scale, int in_size, int& i0, int& i1, float& f) {
  const float s = scale * o;
  i0 = (int)s;
  if (i0 > in_size - 1) i0 = in_size - 1;
  i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
  f = s - i0;
}
__device__ __forceinline__ float ac_scale(int in_size, int out_size) {
  return out_size > 1 ? (float)(in_size - 1) / (out_size - 1) : 0.f;
}

// sum of v over the workgroup (any multiple of 64 threads), returned to every thread; red: one float per wave
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < nw; ++i) t += red[i];
  return t;
}

// floats as order-preserving unsigned keys (radix select)
__device__ __forceinline__ unsigned f2key(float f) { unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float key2f(unsigned k) { unsigned u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k; return __uint_as_float(u); }
