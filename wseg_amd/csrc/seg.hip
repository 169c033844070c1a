// seg.hip — DeepLab multi-scale test fusion (wseg_seg_fuse, include/wseg_hip.h): both bilinear resamples of every pass, the un-flip, the mean over the
// passes, the softmax and the arg-max in one launch, from the stride-8 cls_conv pixel rows.  One thread per output pixel (x fastest: the planar
// stores are full lines), the class sums in registers, the pass loop outermost; the coarse rows (24 contiguous elements) are read with 16-byte loads
// and stay in L2 (at most 770 KB per pass).  No LDS, no atomics.  The source-index arithmetic (seg_src, seg_scale, seg_lerp2) is seg_geo.h's.
#include "seg_geo.h"

namespace {

struct SegArgs {
  wseg_seg_pass p[WSEG_SEG_MAX_PASSES];
  int n_pass, H, W, n_cls;
  float* mean; float* prob; unsigned char* amax; float* margin;
};

struct SegTap { size_t r00, r01, r10, r11; float fy, fx; };   // element offsets of the four coarse rows of one intermediate pixel

template <int DT>
__device__ __forceinline__ void seg_tap8(const void* rows, const SegTap& t, int c0, float (&m)[8]) {
  float a[8], b[8], c[8], d[8];
  load8<DT>(rows, t.r00 + c0, a);
  load8<DT>(rows, t.r01 + c0, b);
  load8<DT>(rows, t.r10 + c0, c);
  load8<DT>(rows, t.r11 + c0, d);
#pragma unroll
  for (int e = 0; e < 8; ++e) m[e] = seg_lerp2(a[e], b[e], c[e], d[e], t.fy, t.fx);
}

// NC8: chunks of 8 classes (n_cls rounded up)
template <int NC8>
__global__ __launch_bounds__(256) void seg_fuse_kernel(SegArgs a) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long npix = (long)a.H * a.W;
  if (idx >= npix) return;
  const int y = (int)(idx / a.W), x = (int)(idx - (long)y * a.W);
  float acc[NC8 * 8];
#pragma unroll
  for (int c = 0; c < NC8 * 8; ++c) acc[c] = 0.f;

  for (int ip = 0; ip < a.n_pass; ++ip) {
    const wseg_seg_pass& p = a.p[ip];
    const int xs = p.flip ? a.W - 1 - x : x;
    // stage 2: (ih, iw) -> (H, W)
    int Y[2], X[2];
    float fy2, fx2;
    seg_src(y, seg_scale(p.ih, a.H), p.ih, Y[0], Y[1], fy2);
    seg_src(xs, seg_scale(p.iw, a.W), p.iw, X[0], X[1], fx2);
    // stage 1: (fh, fw) -> (ih, iw), for the two rows and the two columns of the stage-2 taps
    const float s1y = seg_scale(p.fh, p.ih), s1x = seg_scale(p.fw, p.iw);
    int y0[2], y1[2], x0[2], x1[2];
    float fy1[2], fx1[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      seg_src(Y[j], s1y, p.fh, y0[j], y1[j], fy1[j]);
      seg_src(X[j], s1x, p.fw, x0[j], x1[j], fx1[j]);
    }
    const size_t base = (size_t)p.img * p.fh * p.fw;
    SegTap t[2][2];
#pragma unroll
    for (int jy = 0; jy < 2; ++jy)
#pragma unroll
      for (int jx = 0; jx < 2; ++jx) {
        t[jy][jx].r00 = (base + (size_t)y0[jy] * p.fw + x0[jx]) * p.ld;
        t[jy][jx].r01 = (base + (size_t)y0[jy] * p.fw + x1[jx]) * p.ld;
        t[jy][jx].r10 = (base + (size_t)y1[jy] * p.fw + x0[jx]) * p.ld;
        t[jy][jx].r11 = (base + (size_t)y1[jy] * p.fw + x1[jx]) * p.ld;
        t[jy][jx].fy = fy1[jy];
        t[jy][jx].fx = fx1[jx];
      }
    const bool bf = p.dtype == WSEG_BF16;                    // (uniform: a launch argument)
#pragma unroll
    for (int k = 0; k < NC8; ++k) {
      float m00[8], m01[8], m10[8], m11[8];
      if (bf) {
        seg_tap8<WSEG_BF16>(p.rows, t[0][0], k * 8, m00);
        seg_tap8<WSEG_BF16>(p.rows, t[0][1], k * 8, m01);
        seg_tap8<WSEG_BF16>(p.rows, t[1][0], k * 8, m10);
        seg_tap8<WSEG_BF16>(p.rows, t[1][1], k * 8, m11);
      } else {
        seg_tap8<WSEG_F32>(p.rows, t[0][0], k * 8, m00);
        seg_tap8<WSEG_F32>(p.rows, t[0][1], k * 8, m01);
        seg_tap8<WSEG_F32>(p.rows, t[1][0], k * 8, m10);
        seg_tap8<WSEG_F32>(p.rows, t[1][1], k * 8, m11);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[k * 8 + e] += seg_lerp2(m00[e], m01[e], m10[e], m11[e], fy2, fx2);
    }
  }

  const float cnt = (float)a.n_pass;
  float mx = -INFINITY, second = -INFINITY;
  int arg = 0;
#pragma unroll
  for (int c = 0; c < NC8 * 8; ++c) {
    if (c < a.n_cls) {
      const float v = acc[c] / cnt;
      acc[c] = v;
      if (v > mx) { second = mx; mx = v; arg = c; }
      else if (v > second) second = v;
      if (a.mean) a.mean[(size_t)c * npix + idx] = v;
    }
  }
  a.amax[idx] = (unsigned char)arg;
  if (a.margin) a.margin[idx] = mx - second;
  if (a.prob) {
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < NC8 * 8; ++c)
      if (c < a.n_cls) { acc[c] = expf(acc[c] - mx); sum += acc[c]; }
#pragma unroll
    for (int c = 0; c < NC8 * 8; ++c)
      if (c < a.n_cls) a.prob[(size_t)c * npix + idx] = acc[c] / sum;
  }
}

}  // namespace

extern "C" size_t wseg_sizeof_seg_pass(void) { return sizeof(wseg_seg_pass); }

extern "C" int wseg_seg_fuse(const wseg_seg_pass* passes, int n_pass, int H, int W, int n_cls, float* mean_logits, float* prob,
                             unsigned char* amax, float* margin, void* stream) {
  WSEG_CHECK(passes && amax, "seg_fuse: null pointer (the arg-max output is required)");
  WSEG_CHECK(n_pass >= 1 && n_pass <= WSEG_SEG_MAX_PASSES, "seg_fuse: %d passes outside [1, %d]", n_pass, WSEG_SEG_MAX_PASSES);
  WSEG_CHECK(n_cls >= 2 && n_cls <= WSEG_SEG_MAX_CLASSES, "seg_fuse: n_cls=%d outside [2, %d]", n_cls, WSEG_SEG_MAX_CLASSES);
  WSEG_CHECK(H > 0 && W > 0 && (long)H * W < (1L << 31), "seg_fuse: bad output size %dx%d", H, W);
  const int nc8 = (n_cls + 7) / 8;
  SegArgs a;
  for (int i = 0; i < n_pass; ++i) {
    const wseg_seg_pass& p = passes[i];
    WSEG_CHECK(p.rows && ((uintptr_t)p.rows & 15) == 0, "seg_fuse: pass %d: rows null or not 16-byte aligned", i);
    WSEG_CHECK(p.dtype == WSEG_F32 || p.dtype == WSEG_BF16, "seg_fuse: pass %d: dtype %d (f32 or bf16)", i, p.dtype);
    WSEG_CHECK(p.ld % 8 == 0 && p.ld >= nc8 * 8, "seg_fuse: pass %d: ld=%d must be a multiple of 8 and >= %d", i, p.ld, nc8 * 8);
    WSEG_CHECK(p.fh > 0 && p.fw > 0 && p.ih > 0 && p.iw > 0 && p.img >= 0, "seg_fuse: pass %d: bad dims", i);
    WSEG_CHECK((long)(p.img + 1) * p.fh * p.fw * p.ld < (1L << 40) && p.ih < (1 << 24) && p.iw < (1 << 24), "seg_fuse: pass %d: too large", i);
    a.p[i] = p;
  }
  a.n_pass = n_pass; a.H = H; a.W = W; a.n_cls = n_cls;
  a.mean = mean_logits; a.prob = prob; a.amax = amax; a.margin = margin;
  const dim3 grid((unsigned)(((long)H * W + 255) / 256));
  hipStream_t s = (hipStream_t)stream;
  switch (nc8) {
    case 1: hipLaunchKernelGGL(seg_fuse_kernel<1>, grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL(seg_fuse_kernel<2>, grid, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL(seg_fuse_kernel<3>, grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL(seg_fuse_kernel<4>, grid, dim3(256), 0, s, a); break;
  }
  WSEG_LAUNCH_CHECK();
  return 0;
}
