// seg_data.hip — DeepLab-v1 training data on the device: the chain of segmentation/lib/datasets/BaseDataset.py:88-98 (__weak_augment__) with
// the transforms of lib/datasets/transform.py, for a batch of decoded uint8 images and their uint8 label maps (blockIdx.y = image):
//   RandomHSV -> RandomFlip (before the rescale) -> RandomScale (image cubic, label nearest) -> ImageNorm -> RandomCrop (0 / 255) -> CHW
// in four launches:
//   seg_hsv_kernel        pixelwise, out of place: the jittered pixel goes to column W-1-x where the flip bit is set, so the resampler below
//                         reads a flipped source and nothing after it knows about the flip.  A thread owns 4 consecutive DESTINATION pixels
//                         (12 bytes = three 4-byte stores); unflipped it reads its 12 source bytes as three words too
//   aug_resize_kernel x 2 Pillow's two-pass 8-bit bicubic (aug_resize.h, the device code wseg_augment_batch runs)
//   seg_finish_kernel     ONE launch for both outputs: the image through the float32 normalise table into [3][crop][crop] f32 with +0.0
//                         outside the pasted rectangle, and the label — nearest resample, flip and crop fused into one gather through the
//                         host's index tables — with 255 outside.  A thread owns 4 container pixels of a row: three 16-byte stores and one
//                         4-byte store (crop % 4 == 0; the scalar instantiation otherwise).  No grid-stride loop.
// Every stage reproduces the host chain of wseg_amd/data.py (RandomHSV ... SegRandomCrop) BIT FOR BIT: tests/test_gpu_seg_data.py.  The
// 8-bit HSV arithmetic is OpenCV's definition as include/wseg_hip.h states it; cv2 itself is not available to pin it.
// No atomics, no float64, no LDS: the bytes are the same from run to run.
#include <algorithm>
#include <cstdint>
#include "common.h"
#include "aug_resize.h"

// The inverse HSV rounds every product and every difference on its own (V * (1 - S * f) is three roundings).  hipcc contracts a multiply and
// the add or subtract that follows it into one fused multiply-add by default, and __fmul_rn / __fsub_rn do not prevent it: contraction is
// switched off for this file, as in augment.hip.
#pragma clang fp contract(off)

namespace {

constexpr int HSV_PIX = 4;            // destination pixels per thread of seg_hsv_kernel
constexpr int BLOCK = 256;
constexpr int MAX_GRID_X = 1024;      // the grid-stride launches (hsv, resize): as wseg_augment_batch

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// RGB -> HSV (8 bits, H in [0, 180)) -> offsets -> HSV -> RGB of one pixel
__device__ __forceinline__ void hsv_jitter(int& r, int& g, int& b, int dh, int ds, int dv, const int* __restrict__ sdiv,
                                           const int* __restrict__ hdiv) {
  int v = max(r, max(g, b));
  const int mn = min(r, min(g, b)), diff = v - mn;
  int s = (diff * sdiv[v] + 2048) >> 12;
  const int hn = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
  int h = (hn * hdiv[diff] + 2048) >> 12;                   // arithmetic shift of a signed int
  if (h < 0) h += 180;
  h = (h + dh) % 180;
  if (h < 0) h += 180;                                      // Python's non-negative modulo
  s = clampi(s + ds, 0, 255);
  v = clampi(v + dv, 0, 255);
  const float S = __fdiv_rn((float)s, 255.f), V = __fdiv_rn((float)v, 255.f);
  float hh = (float)h * (6.f / 180.f);                      // the constant is the float32 quotient of 6 and 180
  while (hh < 0.f) hh += 6.f;
  while (hh >= 6.f) hh -= 6.f;
  const float fl = floorf(hh);
  int sec = (int)fl;
  float f = hh - fl;
  if ((unsigned)sec >= 6u) { sec = 0; f = 0.f; }
  const float t0 = V, t1 = V * (1.f - S), t2 = V * (1.f - S * f), t3 = V * (1.f - S * (1.f - f));
  float fb, fg, fr;
  switch (sec) {                                            // (b, g, r) = tab[{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}]
    case 0: fb = t1; fg = t3; fr = t0; break;
    case 1: fb = t1; fg = t0; fr = t2; break;
    case 2: fb = t3; fg = t0; fr = t1; break;
    case 3: fb = t0; fg = t2; fr = t1; break;
    case 4: fb = t0; fg = t1; fr = t3; break;
    default: fb = t2; fg = t1; fr = t0; break;
  }
  if (s == 0) fb = fg = fr = V;
  r = clampi((int)rintf(fr * 255.f), 0, 255);               // rintf: half to even
  g = clampi((int)rintf(fg * 255.f), 0, 255);
  b = clampi((int)rintf(fb * 255.f), 0, 255);
}

__global__ __launch_bounds__(BLOCK) void seg_hsv_kernel(const wseg_aug_desc* __restrict__ aug, const wseg_seg_data_desc* __restrict__ seg,
                                                        const int* __restrict__ hsv_div) {
  const wseg_aug_desc a = aug[blockIdx.y];
  const wseg_seg_data_desc d = seg[blockIdx.y];
  const int W = a.W;
  const long total = (long)a.H * W, groups = (total + HSV_PIX - 1) / HSV_PIX;
  unsigned char* dst = const_cast<unsigned char*>(a.src);   // the resampler's source is this launch's output
  const int* sdiv = hsv_div;
  const int* hdiv = hsv_div + 256;
  for (long grp = (long)blockIdx.x * BLOCK + threadIdx.x; grp < groups; grp += (long)gridDim.x * BLOCK) {
    const long q0 = grp * HSV_PIX;
    const bool full = q0 + HSV_PIX <= total;
    int c[3 * HSV_PIX];
    if (full && !a.flip) {                                  // (raw and src are 4-byte aligned: the entry point refuses others)
      const unsigned* p = reinterpret_cast<const unsigned*>(d.raw + q0 * 3);
#pragma unroll
      for (int w = 0; w < 3; ++w) {
        const unsigned u = p[w];
#pragma unroll
        for (int k = 0; k < 4; ++k) c[4 * w + k] = (int)((u >> (8 * k)) & 255u);
      }
    } else {
#pragma unroll
      for (int j = 0; j < HSV_PIX; ++j) {
        const long q = min(q0 + j, total - 1);              // (pixels past the end repeat the last one and are not stored)
        const int y = (int)(q / W), x = (int)(q - (long)y * W);
        const unsigned char* p = d.raw + ((long)y * W + (a.flip ? W - 1 - x : x)) * 3;
        c[3 * j] = p[0]; c[3 * j + 1] = p[1]; c[3 * j + 2] = p[2];
      }
    }
#pragma unroll
    for (int j = 0; j < HSV_PIX; ++j) hsv_jitter(c[3 * j], c[3 * j + 1], c[3 * j + 2], d.dh, d.ds, d.dv, sdiv, hdiv);
    if (full) {
      unsigned* o = reinterpret_cast<unsigned*>(dst + q0 * 3);
#pragma unroll
      for (int w = 0; w < 3; ++w)
        o[w] = (unsigned)c[4 * w] | ((unsigned)c[4 * w + 1] << 8) | ((unsigned)c[4 * w + 2] << 16) | ((unsigned)c[4 * w + 3] << 24);
    } else {
#pragma unroll
      for (int j = 0; j < HSV_PIX; ++j)
        if (q0 + j < total) {
          unsigned char* o = dst + (q0 + j) * 3;
          o[0] = (unsigned char)c[3 * j]; o[1] = (unsigned char)c[3 * j + 1]; o[2] = (unsigned char)c[3 * j + 2];
        }
    }
  }
}

// normalise + crop placement of the image, gather + crop placement of the label: VEC container pixels of one row per thread
template <int VEC>
__global__ __launch_bounds__(BLOCK) void seg_finish_kernel(const wseg_aug_desc* __restrict__ aug, const wseg_seg_data_desc* __restrict__ seg,
                                                           const float* __restrict__ lut, int crop) {
  const wseg_aug_desc a = aug[blockIdx.y];
  const wseg_seg_data_desc d = seg[blockIdx.y];
  const int per_row = crop / VEC;
  const long groups = (long)per_row * crop, grp = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (grp >= groups) return;
  const int y = (int)(grp / per_row), x0 = (int)(grp - (long)y * per_row) * VEC;
  const int cy = y - a.cont_top;
  const bool row_in = cy >= 0 && cy < a.ch;
  const int ry = row_in ? cy + a.img_top : 0;
  const unsigned char* irow = a.img + (long)ry * a.rw * 3;
  const unsigned char* lrow = d.lab;
  if (row_in) lrow += (long)clampi(d.yi[ry], 0, a.H - 1) * a.W;
  float v[3][VEC];
  unsigned char l[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const int cx = x0 + j - a.cont_left;
    v[0][j] = v[1][j] = v[2][j] = 0.f;                      // +0.0: the container is np.zeros, not normalize(0)
    l[j] = 255;
    if (row_in && cx >= 0 && cx < a.cw) {
      const int rx = cx + a.img_left;
      const unsigned char* p = irow + (long)rx * 3;
      v[0][j] = lut[p[0]]; v[1][j] = lut[256 + p[1]]; v[2][j] = lut[512 + p[2]];
      l[j] = lrow[clampi(d.xi[rx], 0, a.W - 1)];
    }
  }
  const long plane = (long)crop * crop, idx = (long)y * crop + x0;
  if constexpr (VEC == 4) {
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(a.out + c * plane + idx) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
    *reinterpret_cast<unsigned*>(d.lab_out + idx) = (unsigned)l[0] | ((unsigned)l[1] << 8) | ((unsigned)l[2] << 16) | ((unsigned)l[3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      a.out[idx + j] = v[0][j]; a.out[plane + idx + j] = v[1][j]; a.out[2 * plane + idx + j] = v[2][j];
      d.lab_out[idx + j] = l[j];
    }
  }
}

unsigned stride_grid(long items) { return (unsigned)std::min<long>(MAX_GRID_X, std::max<long>(1, (items + BLOCK - 1) / BLOCK)); }
unsigned finish_grid(int crop, int vec) { return (unsigned)(((long)(crop / vec) * crop + BLOCK - 1) / BLOCK); }

}  // namespace

extern "C" size_t wseg_sizeof_seg_data_desc(void) { return sizeof(wseg_seg_data_desc); }

extern "C" int wseg_seg_data_geometry(int max_pixels, int crop, int* out4) {
  WSEG_CHECK(out4 && max_pixels > 0 && crop > 0, "seg_data_geometry: bad arguments");
  const int vec = crop % 4 == 0 ? 4 : 1;
  out4[0] = (int)stride_grid(((long)max_pixels + HSV_PIX - 1) / HSV_PIX);
  out4[1] = (int)stride_grid(max_pixels);
  out4[2] = (int)finish_grid(crop, vec);
  out4[3] = vec;
  return 0;
}

extern "C" int wseg_seg_data_batch(const wseg_aug_desc* aug_host, const wseg_seg_data_desc* seg_host, const wseg_aug_desc* aug_dev,
                                   const wseg_seg_data_desc* seg_dev, int n, int crop, const float* lut, const int32_t* hsv_div, int stages,
                                   void* stream) {
  WSEG_CHECK(n > 0 && n <= 65535, "seg_data_batch: n = %d is outside [1, 65535]", n);
  WSEG_CHECK(crop > 0 && crop <= 32768, "seg_data_batch: crop = %d is outside [1, 32768]", crop);
  WSEG_CHECK(aug_host && seg_host && aug_dev && seg_dev, "seg_data_batch: a descriptor array is null");
  WSEG_CHECK(stages > 0 && stages <= 7, "seg_data_batch: stages = %d selects no launch", stages);
  const bool hsv = stages & WSEG_SEG_DATA_HSV, resize = stages & WSEG_SEG_DATA_RESIZE, finish = stages & WSEG_SEG_DATA_FINISH;
  WSEG_CHECK(!hsv || hsv_div, "seg_data_batch: the HSV division tables are null");
  WSEG_CHECK(!finish || lut, "seg_data_batch: the normalise table is null");
  long max_src = 1, max_res = 1;
  const bool wide = crop % 4 == 0;
  for (int i = 0; i < n; ++i) {
    const wseg_aug_desc& a = aug_host[i];
    const wseg_seg_data_desc& d = seg_host[i];
    WSEG_CHECK(a.H > 0 && a.W > 0 && a.rh > 0 && a.rw > 0, "seg_data_batch: image %d has the sizes %d x %d -> %d x %d", i, a.H, a.W, a.rh, a.rw);
    WSEG_CHECK(a.flip == 0 || a.flip == 1, "seg_data_batch: image %d has the flip bit %d", i, a.flip);
    WSEG_CHECK(a.src, "seg_data_batch: image %d has no buffer for the jittered image", i);
    WSEG_CHECK(!hsv || d.raw, "seg_data_batch: image %d has no decoded image", i);
    WSEG_CHECK(!hsv || (((uintptr_t)d.raw | (uintptr_t)a.src) & 3) == 0, "seg_data_batch: image %d is not 4-byte aligned", i);
    WSEG_CHECK(!resize || (a.tmp && a.img && a.xb && a.xk && a.yb && a.yk && a.xks > 0 && a.yks > 0),
               "seg_data_batch: image %d lacks a resize buffer or table", i);
    if (finish) {
      WSEG_CHECK(a.img && a.out && d.lab && d.yi && d.xi && d.lab_out, "seg_data_batch: image %d has a null pointer", i);
      WSEG_CHECK(a.ch > 0 && a.ch <= crop && a.cw > 0 && a.cw <= crop, "seg_data_batch: image %d pastes %d x %d into a crop of %d", i, a.ch, a.cw, crop);
      WSEG_CHECK(a.cont_top >= 0 && a.cont_top <= crop - a.ch && a.cont_left >= 0 && a.cont_left <= crop - a.cw,
                 "seg_data_batch: image %d pastes at (%d, %d), outside the container", i, a.cont_top, a.cont_left);
      WSEG_CHECK(a.img_top >= 0 && a.ch <= a.rh && a.img_top <= a.rh - a.ch && a.img_left >= 0 && a.cw <= a.rw && a.img_left <= a.rw - a.cw,
                 "seg_data_batch: image %d reads %d x %d from (%d, %d) of a %d x %d image", i, a.ch, a.cw, a.img_top, a.img_left, a.rh, a.rw);
      WSEG_CHECK(!wide || ((((uintptr_t)a.out & 15) == 0 && ((uintptr_t)d.lab_out & 3) == 0)),
                 "seg_data_batch: image %d has outputs off the 16-byte / 4-byte alignment of a crop that is a multiple of 4", i);
    }
    max_src = std::max(max_src, (long)a.H * a.W);
    max_res = std::max({max_res, (long)a.H * a.rw, (long)a.rh * a.rw});
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(BLOCK);
  if (hsv) hipLaunchKernelGGL(seg_hsv_kernel, dim3(stride_grid((max_src + HSV_PIX - 1) / HSV_PIX), n), blk, 0, s, aug_dev, seg_dev, hsv_div);
  if (resize) {
    const dim3 grid(stride_grid(max_res), n);
    hipLaunchKernelGGL(aug_resize_kernel<0>, grid, blk, 0, s, aug_dev);
    hipLaunchKernelGGL(aug_resize_kernel<1>, grid, blk, 0, s, aug_dev);
  }
  if (finish) {
    if (wide) hipLaunchKernelGGL(seg_finish_kernel<4>, dim3(finish_grid(crop, 4), n), blk, 0, s, aug_dev, seg_dev, lut, crop);
    else hipLaunchKernelGGL(seg_finish_kernel<1>, dim3(finish_grid(crop, 1), n), blk, 0, s, aug_dev, seg_dev, lut, crop);
  }
  WSEG_LAUNCH_CHECK();
  return 0;
}
