// seg_loss.hip — the DeepLab-v1 training loss (segmentation/lib/net/deeplabv1.py:50 + experiment/SEAM_deeplabv1_resnet38/train.py:85,97):
// cross-entropy (ignore_index 255, mean over the valid pixels of the batch) of the stride-8 logits resampled bilinearly (align_corners=True)
// to the label size, and its gradient on the coarse cls_conv rows.  The full-size [N][n_cls][H][W] logits are never written:
//   seg_ce_forward   one thread per label pixel (x fastest, as seg_fuse): the pixel's bilinear sample of its image's coarse rows in
//                    registers, log-sum-exp, nll = lse - z[label]; lse is kept ([N][H][W] f32); the nll sum and the two integer counts are
//                    reduced per workgroup in a fixed order into a [blocks][3] workspace (no atomics)
//   seg_ce_finish    one workgroup adds the partials in a fixed order (the sum in f64, the counts as integers) -> out[4]
//   seg_ce_backward  one wave per coarse cell in GATHER form: the lanes stride over the fine pixels whose taps include the cell, recompute the
//                    softmax from the four coarse rows and the saved lse, and add w_y * w_x * (softmax_c - [c == label]); one fixed butterfly
//                    over the lanes, one multiplication by gscale / count, one store of the row (no atomics, no scatter)
// Which pixels touch a cell, and with what weight, is decided by seg_src (seg_geo.h) — the function the forward sampled with — on every pixel
// of a conservative range; the scale is never inverted to decide membership, so a pixel whose f32 coordinate lands a hair under an integer
// goes to the cell the forward read.  Nothing is accumulated in an order that depends on scheduling.
#include "seg_geo.h"

namespace {

struct SegCeArgs {
  const void* rows; const unsigned char* label;
  int ld, N, fh, fw, H, W, n_cls;
  float sy, sx;                                                  // seg_scale(fh, H), seg_scale(fw, W)
};

// z[e] = the bilinear sample of columns [c0, c0 + 8) of the four coarse rows (element offsets r00 .. r11); columns >= n_cls are loaded with
// their chunk and never used by a caller
template <int DT>
__device__ __forceinline__ void seg_ce_sample8(const void* rows, size_t r00, size_t r01, size_t r10, size_t r11, int c0, float fy, float fx,
                                               float* z) {
  float a[8], b[8], c[8], d[8];
  load8<DT>(rows, r00 + c0, a);
  load8<DT>(rows, r01 + c0, b);
  load8<DT>(rows, r10 + c0, c);
  load8<DT>(rows, r11 + c0, d);
#pragma unroll
  for (int e = 0; e < 8; ++e) z[e] = seg_lerp2(a[e], b[e], c[e], d[e], fy, fx);
}

template <int DT, int NC8>
__global__ __launch_bounds__(256) void seg_ce_forward_kernel(SegCeArgs a, float* __restrict__ lse_out, float* __restrict__ ws) {
  __shared__ float red_s[4];
  __shared__ int red_c[4][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long npix = (long)a.H * a.W;
  float nll = 0.f;
  int valid = 0, oor = 0;
  if (idx < (long)a.N * npix) {
    const int n = (int)(idx / npix), rem = (int)(idx - (long)n * npix);
    const int y = rem / a.W, x = rem - y * a.W;
    int y0, y1, x0, x1;
    float fy, fx;
    seg_src(y, a.sy, a.fh, y0, y1, fy);
    seg_src(x, a.sx, a.fw, x0, x1, fx);
    const size_t base = (size_t)n * a.fh * a.fw;
    float z[NC8 * 8];
    const size_t r00 = (base + (size_t)y0 * a.fw + x0) * a.ld, r01 = (base + (size_t)y0 * a.fw + x1) * a.ld;
    const size_t r10 = (base + (size_t)y1 * a.fw + x0) * a.ld, r11 = (base + (size_t)y1 * a.fw + x1) * a.ld;
#pragma unroll
    for (int k = 0; k < NC8; ++k) seg_ce_sample8<DT>(a.rows, r00, r01, r10, r11, k * 8, fy, fx, z + k * 8);
    const unsigned lab = a.label[idx];
    float mx = -INFINITY, zl = 0.f;
#pragma unroll
    for (int c = 0; c < NC8 * 8; ++c)
      if (c < a.n_cls) {
        mx = fmaxf(mx, z[c]);
        zl = (unsigned)c == lab ? z[c] : zl;
      }
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < NC8 * 8; ++c)
      if (c < a.n_cls) sum += expf(z[c] - mx);
    const float lse = mx + logf(sum);
    if (lse_out) lse_out[idx] = lse;
    if (lab < (unsigned)a.n_cls) { nll = lse - zl; valid = 1; }
    else if (lab != 255u) oor = 1;                               // a value in [n_cls, 255): ignored, counted, never an index
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nll += __shfl_xor(nll, o, 64);
    valid += __shfl_xor(valid, o, 64);
    oor += __shfl_xor(oor, o, 64);
  }
  if (lane == 0) { red_s[wave] = nll; red_c[wave][0] = valid; red_c[wave][1] = oor; }
  __syncthreads();
  if (threadIdx.x == 0) {
    ws[(long)blockIdx.x * 3] = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
    ws[(long)blockIdx.x * 3 + 1] = __int_as_float(red_c[0][0] + red_c[1][0] + red_c[2][0] + red_c[3][0]);
    ws[(long)blockIdx.x * 3 + 2] = __int_as_float(red_c[0][1] + red_c[1][1] + red_c[2][1] + red_c[3][1]);
  }
}

// thread t adds the partials of blocks t, t + 256, ... in that order, then a fixed LDS tree: the order never depends on scheduling
__global__ __launch_bounds__(256) void seg_ce_finish_kernel(const float* __restrict__ ws, int blocks, float* __restrict__ out) {
  __shared__ double red_s[256];
  __shared__ long long red_c[256][2];
  const int t = threadIdx.x;
  double s = 0.;
  long long c[2] = {0, 0};
  for (int b = t; b < blocks; b += 256) {
    s += (double)ws[(long)b * 3];
    c[0] += __float_as_int(ws[(long)b * 3 + 1]);
    c[1] += __float_as_int(ws[(long)b * 3 + 2]);
  }
  red_s[t] = s; red_c[t][0] = c[0]; red_c[t][1] = c[1];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) { red_s[t] += red_s[t + o]; red_c[t][0] += red_c[t + o][0]; red_c[t][1] += red_c[t + o][1]; }
    __syncthreads();
  }
  if (t == 0) {
    out[0] = (float)(red_s[0] / (double)red_c[0][0]);             // no valid pixel: 0 / 0 = NaN, the mean of an empty set as torch gives it
    out[1] = (float)red_c[0][0];
    out[2] = (float)red_s[0];
    out[3] = (float)red_c[0][1];
  }
}

// does the output position o of an axis read the input position c (as i0 or as i1)?
__device__ __forceinline__ bool seg_reads(int o, float scale, int n_in, int c) {
  int i0, i1;
  float f;
  seg_src(o, scale, n_in, i0, i1, f);
  return i0 == c || i1 == c;
}

// [lo, hi]: the output positions of an axis that read input position c; empty (lo > hi) when none does.  The range starts conservative —
// positions o with scale * o in (c - 1, c + 1), two positions wider on either side: the f32 product's error is below one position for
// o < 2^24 — and is narrowed from both ends with seg_reads itself.  The caller still tests every position inside it.
__device__ __forceinline__ void seg_support(int c, float scale, int n_in, int n_out, int& lo, int& hi) {
  lo = 0;
  hi = n_out - 1;
  if (scale > 0.f) {                                             // (scale == 0: one input or one output position, everything reads position 0)
    const double inv = 1.0 / (double)scale;
    lo = (int)fmin(fmax(floor((double)(c - 1) * inv) - 2.0, 0.0), (double)n_out);      // (clamped as doubles: the quotient may exceed an int)
    hi = (int)fmin(ceil((double)(c + 1) * inv) + 2.0, (double)(n_out - 1));
  }
  while (lo <= hi && !seg_reads(lo, scale, n_in, c)) ++lo;
  while (hi >= lo && !seg_reads(hi, scale, n_in, c)) --hi;
}

// the weight input position c has in the sample (i0, i1, f): 1 - f as i0, f as i1 (both where the two coincide at the last position)
__device__ __forceinline__ float seg_weight(int c, int i0, int i1, float f) { return (i0 == c ? 1.f - f : 0.f) + (i1 == c ? f : 0.f); }

template <int DT, int DD, int NC8>
__global__ __launch_bounds__(256) void seg_ce_backward_kernel(SegCeArgs a, const float* __restrict__ lse, const float* __restrict__ out4,
                                                              const float* __restrict__ gscale, void* __restrict__ d_rows, int ld_d) {
  const int lane = threadIdx.x & 63;
  const int area = a.fh * a.fw;
  const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= (long)a.N * area) return;                           // (wave-uniform; no barrier below)
  const int n = (int)(item / area), q = (int)(item - (long)n * area);
  const int cy = q / a.fw, cx = q - cy * a.fw;
  int ylo, yhi, xlo, xhi;
  seg_support(cy, a.sy, a.fh, a.H, ylo, yhi);
  seg_support(cx, a.sx, a.fw, a.W, xlo, xhi);
  float acc[NC8 * 8];
#pragma unroll
  for (int c = 0; c < NC8 * 8; ++c) acc[c] = 0.f;
  if (ylo <= yhi && xlo <= xhi) {
    const int nx = xhi - xlo + 1;
    const int cnt = (yhi - ylo + 1) * nx;                         // <= H * W < 2^31
    const size_t base = (size_t)n * area;
    const long pix0 = (long)n * a.H * a.W;
    for (int i = lane; i < cnt; i += 64) {
      const int dy = i / nx;
      const int y = ylo + dy, x = xlo + (i - dy * nx);
      const long pix = pix0 + (long)y * a.W + x;
      const unsigned lab = a.label[pix];
      if (lab >= (unsigned)a.n_cls) continue;                      // ignored (255 or out of range): no gradient
      int y0, y1, x0, x1;
      float fy, fx;
      seg_src(y, a.sy, a.fh, y0, y1, fy);
      seg_src(x, a.sx, a.fw, x0, x1, fx);
      const float w = seg_weight(cy, y0, y1, fy) * seg_weight(cx, x0, x1, fx);
      if (w == 0.f) continue;                                     // not a tap of this cell, or a tap of weight zero
      const size_t r00 = (base + (size_t)y0 * a.fw + x0) * a.ld, r01 = (base + (size_t)y0 * a.fw + x1) * a.ld;
      const size_t r10 = (base + (size_t)y1 * a.fw + x0) * a.ld, r11 = (base + (size_t)y1 * a.fw + x1) * a.ld;
      const float l = lse[pix];
#pragma unroll
      for (int k = 0; k < NC8; ++k) {                              // chunk by chunk: the saved lse makes every class independent of the others
        float z[8];
        seg_ce_sample8<DT>(a.rows, r00, r01, r10, r11, k * 8, fy, fx, z);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (k * 8 + e < a.n_cls) acc[k * 8 + e] += w * (expf(z[e] - l) - ((unsigned)(k * 8 + e) == lab ? 1.f : 0.f));
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NC8 * 8; ++c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o, 64);
  }
  if (lane == 0) {
    const float count = out4[1];
    const float k = count > 0.f ? (gscale ? gscale[0] : 1.f) / count : 0.f;      // no valid pixel in the batch: every sum is zero and stays zero
#pragma unroll
    for (int j = 0; j < NC8; ++j) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = acc[j * 8 + e] * k;      // (columns >= n_cls: 0 * k = 0)
      store8<DD>(d_rows, (size_t)item * ld_d + j * 8, v);
    }
  }
}

int seg_ce_check(const char* what, const void* rows, int ld, int dtype, int N, int fh, int fw, int H, int W, int n_cls) {
  WSEG_CHECK(n_cls >= 2 && n_cls <= WSEG_SEG_MAX_CLASSES, "%s: n_cls=%d outside [2, %d]", what, n_cls, WSEG_SEG_MAX_CLASSES);
  const int nc8 = (n_cls + 7) / 8 * 8;
  WSEG_CHECK(rows && ((uintptr_t)rows & 15) == 0, "%s: rows null or not 16-byte aligned", what);
  WSEG_CHECK(dtype == WSEG_F32 || dtype == WSEG_BF16, "%s: dtype %d (f32 or bf16)", what, dtype);
  WSEG_CHECK(ld % 8 == 0 && ld >= nc8, "%s: ld=%d must be a multiple of 8 and >= %d", what, ld, nc8);
  WSEG_CHECK(N > 0 && fh > 0 && fw > 0 && H > 0 && W > 0, "%s: bad dims N=%d coarse %dx%d label %dx%d", what, N, fh, fw, H, W);
  WSEG_CHECK(fh < (1 << 24) && fw < (1 << 24) && H < (1 << 24) && W < (1 << 24), "%s: a side of 2^24 or more (coarse %dx%d label %dx%d)", what, fh, fw, H, W);
  WSEG_CHECK((long)N * H * W < (1L << 31), "%s: N*H*W = %ld must stay below 2^31", what, (long)N * H * W);
  WSEG_CHECK((long)N * fh * fw < (1L << 31) && (long)N * fh * fw * ld < (1L << 40), "%s: coarse rows too large", what);
  return 0;
}

long seg_ce_blocks(int N, int H, int W) { return ((long)N * H * W + 255) / 256; }

SegCeArgs seg_ce_args(const void* rows, int ld, const unsigned char* label, int N, int fh, int fw, int H, int W, int n_cls) {
  SegCeArgs a;
  a.rows = rows; a.label = label; a.ld = ld; a.N = N; a.fh = fh; a.fw = fw; a.H = H; a.W = W; a.n_cls = n_cls;
  a.sy = seg_scale(fh, H); a.sx = seg_scale(fw, W);
  return a;
}

}  // namespace

extern "C" long wseg_seg_ce_workspace_bytes(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0 || (long)N * H * W >= (1L << 31)) {
    wseg_set_error("seg_ce_workspace_bytes: bad size N=%d label %dx%d (N*H*W must stay below 2^31)", N, H, W);
    return -1;
  }
  return seg_ce_blocks(N, H, W) * 3 * (long)sizeof(float);
}

extern "C" int wseg_seg_ce_forward(const void* rows, int ld, int dtype, const unsigned char* label, float* lse, void* workspace, float* out4,
                                   int N, int fh, int fw, int H, int W, int n_cls, void* stream) {
  if (int rc = seg_ce_check("seg_ce_forward", rows, ld, dtype, N, fh, fw, H, W, n_cls)) return rc;
  WSEG_CHECK(label && workspace && out4, "seg_ce_forward: null pointer");
  const long blocks = seg_ce_blocks(N, H, W);
  const SegCeArgs a = seg_ce_args(rows, ld, label, N, fh, fw, H, W, n_cls);
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  with_const<2>(dtype, [&](auto dt) {
    with_const<4>((n_cls + 7) / 8 - 1, [&](auto k) {
      hipLaunchKernelGGL((seg_ce_forward_kernel<decltype(dt)::value, decltype(k)::value + 1>), dim3((unsigned)blocks), dim3(256), 0, s, a, lse, ws);
    });
  });
  WSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL(seg_ce_finish_kernel, dim3(1), dim3(256), 0, s, ws, (int)blocks, out4);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_seg_ce_backward(const void* rows, int ld, int dtype, const unsigned char* label, const float* lse, const float* out4,
                                    const float* gscale, void* d_rows, int ld_d, int d_dtype, int N, int fh, int fw, int H, int W, int n_cls,
                                    void* stream) {
  if (int rc = seg_ce_check("seg_ce_backward", rows, ld, dtype, N, fh, fw, H, W, n_cls)) return rc;
  WSEG_CHECK(label && lse && out4, "seg_ce_backward: null pointer (the forward must have kept lse)");
  WSEG_CHECK(d_rows && ((uintptr_t)d_rows & 15) == 0, "seg_ce_backward: d_rows null or not 16-byte aligned");
  WSEG_CHECK(d_dtype == WSEG_F32 || d_dtype == WSEG_BF16, "seg_ce_backward: d_dtype %d (f32 or bf16)", d_dtype);
  const int nc8 = (n_cls + 7) / 8 * 8;
  WSEG_CHECK(ld_d % 8 == 0 && ld_d >= nc8, "seg_ce_backward: ld_d=%d must be a multiple of 8 and >= %d", ld_d, nc8);
  WSEG_CHECK((long)N * fh * fw * ld_d < (1L << 40), "seg_ce_backward: gradient rows too large");
  const long blocks = ((long)N * fh * fw + 3) / 4;
  const SegCeArgs a = seg_ce_args(rows, ld, label, N, fh, fw, H, W, n_cls);
  hipStream_t s = (hipStream_t)stream;
  with_const<2>(dtype, [&](auto dt) {
    with_const<2>(d_dtype, [&](auto dd) {
      with_const<4>(nc8 / 8 - 1, [&](auto k) {
        hipLaunchKernelGGL((seg_ce_backward_kernel<decltype(dt)::value, decltype(dd)::value, decltype(k)::value + 1>), dim3((unsigned)blocks),
                           dim3(256), 0, s, a, lse, out4, gscale, d_rows, ld_d);
      });
    });
  });
  WSEG_LAUNCH_CHECK();
  return 0;
}
