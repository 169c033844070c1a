// seg_geo.h — the align_corners=True bilinear source-index arithmetic of the DeepLab stage, shared by seg.hip (the test-time fusion) and
// seg_loss.hip (the training loss and its gather-form gradient): one copy, so that a fine pixel's taps and weights are the same f32 values
// wherever they are computed.  Not in common.h: every conv / wgrad file includes that header and none of them resamples.
#pragma once
#include "common.h"

namespace {

// ATen's align_corners source index (area_pixel_compute_source_index + guard_index_and_lambda): s = scale * o in f32, i0 = min(floor(s), n - 1),
// i1 = i0 + (i0 < n - 1), f = s - i0
__device__ __forceinline__ void seg_src(int o, float scale, int n, int& i0, int& i1, float& f) {
  const float s = scale * (float)o;
  i0 = min((int)s, n - 1);
  i1 = i0 + (i0 < n - 1 ? 1 : 0);
  f = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
}
__host__ __device__ inline float seg_scale(int n_in, int n_out) { return n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f; }

// one bilinear sample, each product and sum rounded to f32 on its own (no contraction: the value does not depend on the compiler's fusing)
__device__ __forceinline__ float seg_lerp2(float a, float b, float c, float d, float fy, float fx) {
#pragma clang fp contract(off)
  return (1.f - fy) * ((1.f - fx) * a + fx * b) + fy * ((1.f - fx) * c + fx * d);
}

}  // namespace
