// aug_resize.h — Pillow's two-pass 8-bit resampler on the device, shared by augment.hip (wseg_augment_batch) and seg_data.hip
// (wseg_seg_data_batch): integer coefficients of 22 fractional bits made on the host in float64 exactly as Resample.c makes them
// (wseg_amd/augment.py pil_bicubic_coeffs), rounding constant, clip, uint8 intermediate.  Integer arithmetic only: the bytes do not depend on
// the translation unit that instantiates it.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ unsigned char clip8i(long long v) { return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// one pass of Pillow's ImagingResampleHorizontal_8bpc / Vertical_8bpc: out = clip8((2^21 + sum_j in[min + j] * k[j]) >> 22)
template <int VERTICAL>
__global__ void aug_resize_kernel(const wseg_aug_desc* __restrict__ descs) {
  const wseg_aug_desc d = descs[blockIdx.y];
  const int ow = d.rw, oh = VERTICAL ? d.rh : d.H;           // this pass's output size
  const long total = (long)ow * oh;
  const unsigned char* in = VERTICAL ? d.tmp : d.src;
  unsigned char* out = VERTICAL ? d.img : d.tmp;
  const int in_w = VERTICAL ? d.rw : d.W;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int y = (int)(idx / ow), x = (int)(idx - (long)y * ow);
    const int o = VERTICAL ? y : x;
    const int* b = (VERTICAL ? d.yb : d.xb) + 2 * o;
    const int ks = VERTICAL ? d.yks : d.xks;
    const int* k = (VERTICAL ? d.yk : d.xk) + (long)o * ks;
    const int lo = b[0], cnt = b[1];
    long long s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
    for (int j = 0; j < cnt; ++j) {
      const unsigned char* p = VERTICAL ? in + ((long)(lo + j) * in_w + x) * 3 : in + ((long)y * in_w + lo + j) * 3;
      const long long kk = k[j];
      s0 += p[0] * kk; s1 += p[1] * kk; s2 += p[2] * kk;
    }
    unsigned char* q = out + idx * 3;
    q[0] = clip8i(s0 >> 22); q[1] = clip8i(s1 >> 22); q[2] = clip8i(s2 >> 22);
  }
}

}  // namespace
