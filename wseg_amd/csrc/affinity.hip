// affinity.hip — AffinityNet inference (network/resnet38_aff.py, aff_infer.py:14-141) without the dense matrix.
//
// The reference gathers pair features on the device, builds the [area][area] affinity matrix on the host
// (sparse -> dense), raises it to the power beta, normalises its columns and squares it logt times (6 dense
// f32 GEMMs of area^3 each: 3.1e11 FLOP at 47x63), then multiplies the 21 pooled CAM planes by it.  The matrix
// is a fixed stencil (<= 2P + 1 non-zeros per column), so here:
//   aff_pairs     the P affinities of every "from" pixel, one wave per pixel, the 448-channel |diff| sum in f32
//   aff_to_dense  the dense matrix itself, for forward(x, to_dense=True) only
//   rw_prepare    stencil weights A^beta per (slot, column) and the reciprocal column sums
//   random_walk   2^logt stencil applications per CAM plane, one workgroup per plane, the plane ping-ponged in LDS
//   rw_pool       bg plane + class planes + zero padding + 8x8 average pooling
//   rw_finish     bilinear upsample (align_corners=False) + arg-max + crop, written as uint8
#include "aff_geo.h"

namespace {

// one wave per (image, from pixel): the from row stays in registers (8 channels per lane), every to row is one coalesced load
template <int DT>
__global__ __launch_bounds__(256) void aff_pairs_kernel(const void* __restrict__ feat, int ld, int C, float* __restrict__ aff, int N, AffGeo g) {
  const int lane = threadIdx.x & 63;
  const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= (long)N * g.n_from) return;
  const int n = (int)(item / g.n_from), f = (int)(item - (long)n * g.n_from);
  const int fy = f / g.cw, fx = f - fy * g.cw + g.r - 1;
  const long base = (long)n * g.h * g.w;
  const int groups = C >> 3;                                    // <= 64 (C <= 512, host-checked)
  const bool act = lane < groups;
  const int c0 = act ? lane * 8 : 0;
  float a[8];
  load8<DT>(feat, (size_t)(base + (long)fy * g.w + fx) * ld + c0, a);
  const float fc = (float)C;
  for (int p = 0; p < g.P; ++p) {
    const long to = base + (long)(fy + g.dy[p]) * g.w + fx + g.dx[p];
    float b[8];
    load8<DT>(feat, (size_t)to * ld + c0, b);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s += fabsf(b[e] - a[e]);
    s = act ? s : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) aff[((long)n * g.P + p) * g.n_from + f] = expf(-(s / fc));
  }
}

__global__ __launch_bounds__(256) void aff_dense_kernel(const float* __restrict__ aff, float* __restrict__ dense, AffGeo g) {
  const long area = (long)g.h * g.w;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long npairs = (long)g.P * g.n_from;
  if (i < npairs) {
    const int p = (int)(i / g.n_from), f = (int)(i - (long)p * g.n_from);
    const int fy = f / g.cw, fx = f - fy * g.cw + g.r - 1;
    const long from = (long)fy * g.w + fx, to = (long)(fy + g.dy[p]) * g.w + fx + g.dx[p];
    const float v = aff[i];
    dense[from * area + to] = v;
    dense[to * area + from] = v;
  } else if (i < npairs + area) {
    const long j = i - npairs;
    dense[j * area + j] = 1.f;
  }
}

// one thread per (image, column j): the 2P slots of j and its column sum (diagonal first, then the slots in order)
__global__ __launch_bounds__(256) void rw_prepare_kernel(const float* __restrict__ aff, float* __restrict__ wgt, float* __restrict__ rsum,
                                                         int N, int beta, AffGeo g) {
  const int area = g.h * g.w;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)N * area) return;
  const int n = (int)(t / area), j = (int)(t - (long)n * area);
  const int y = j / g.w, x = j - y * g.w;
  const int ch = g.h - g.r + 1, x_lo = g.r - 1, x_hi = g.w - g.r + 1;
  const bool j_from = y < ch && x >= x_lo && x < x_hi;
  const float* an = aff + (long)n * g.P * g.n_from;
  float* wn = wgt + (long)n * 2 * g.P * area;
  const float fb = (float)beta;
  float s = 1.f;
  for (int q = 0; q < g.P; ++q) {                                 // j = from, i = j + offset
    float v = 0.f;
    if (j_from) v = powf(an[(long)q * g.n_from + y * g.cw + (x - x_lo)], fb);
    wn[(long)q * area + j] = v;
    s += v;
  }
  for (int q = 0; q < g.P; ++q) {                                 // j = to, i = j - offset
    const int iy = y - g.dy[q], ix = x - g.dx[q];
    float v = 0.f;
    if (iy >= 0 && iy < ch && ix >= x_lo && ix < x_hi) v = powf(an[(long)q * g.n_from + iy * g.cw + (ix - x_lo)], fb);
    wn[(long)(g.P + q) * area + j] = v;
    s += v;
  }
  rsum[(long)n * area + j] = 1.f / s;
}

// one workgroup per (image, plane); 2^logt steps with one barrier each.  Out-of-range neighbours carry weight 0 and read a clamped
// (in-plane) LDS address, so the step has no divergent branch.
__global__ __launch_bounds__(1024) void random_walk_kernel(const float* __restrict__ wgt, const float* __restrict__ rsum,
                                                           const float* v_in, float* v_out, int planes, int steps, AffGeo g) {
  extern __shared__ float lds[];
  const int area = g.h * g.w;
  const int n = blockIdx.x / planes;
  float* cur = lds;
  float* nxt = lds + area;
  const long pbase = (long)blockIdx.x * area;
  for (int j = threadIdx.x; j < area; j += blockDim.x) cur[j] = v_in[pbase + j];
  __syncthreads();
  const float* wn = wgt + (long)n * 2 * g.P * area;
  const float* rn = rsum + (long)n * area;
  for (int it = 0; it < steps; ++it) {
    for (int j = threadIdx.x; j < area; j += blockDim.x) {
      float acc = cur[j];
      for (int q = 0; q < g.P; ++q) {
        const int o = g.dy[q] * g.w + g.dx[q];
        const int i1 = min(j + o, area - 1), i2 = max(j - o, 0);
        acc = fmaf(cur[i1], wn[(long)q * area + j], acc);
        acc = fmaf(cur[i2], wn[(long)(g.P + q) * area + j], acc);
      }
      nxt[j] = acc * rn[j];
    }
    __syncthreads();
    float* t = cur; cur = nxt; nxt = t;
  }
  for (int j = threadIdx.x; j < area; j += blockDim.x) v_out[pbase + j] = cur[j];
}

struct PlaneSrc { int src[21]; };

__global__ __launch_bounds__(256) void rw_pool_kernel(const float* __restrict__ cams, PlaneSrc ps, float bg, float* __restrict__ pooled,
                                                      int H, int W, int dh, int dw) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long per = (long)dh * dw;
  if (t >= 21 * per) return;
  const int c = (int)(t / per), k = (int)(t - (long)c * per);
  const int py = k / dw, px = k - py * dw;
  const int s = ps.src[c];
  float acc = 0.f;
  for (int ky = 0; ky < 8; ++ky) {
    const int y = py * 8 + ky;
    for (int kx = 0; kx < 8; ++kx) {
      const int x = px * 8 + kx;
      float v = 0.f;
      if (y < H && x < W) v = c == 0 ? bg : (s >= 0 ? cams[((long)s * H + y) * W + x] : 0.f);
      acc += v;
    }
  }
  pooled[t] = acc / 64.f;
}

// nn.Upsample(mode='bilinear') source index (align_corners=False): max(scale*(o+0.5)-0.5, 0), scale = in/out
// (differs from loss_helpers.h src_index: half-pixel centres, and no clamp of i0, which cannot exceed in_size - 1 here)
__device__ __forceinline__ void src_index(int o, float scale, int in_size, int& i0, int& i1, float& l1) {
  float s = scale * (o + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l1 = s - i0;
}

__global__ __launch_bounds__(256) void rw_finish_kernel(const float* __restrict__ cam, unsigned char* __restrict__ pred, int planes,
                                                        int dh, int dw, int H, int W) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)H * W) return;
  const int y = (int)(t / W), x = (int)(t - (long)y * W);
  int y0, y1, x0, x1; float ly, lx;
  src_index(y, (float)dh / (8 * dh), dh, y0, y1, ly);
  src_index(x, (float)dw / (8 * dw), dw, x0, x1, lx);
  const float hy = 1.f - ly, hx = 1.f - lx;
  const long per = (long)dh * dw;
  float best = 0.f;
  int arg = 0;
  for (int c = 0; c < planes; ++c) {
    const float* p = cam + c * per;
    // explicit fmas: left to the compiler's contraction, the peeled plane 0 and the loop body were fused differently, so a plane >= 1
    // that is a bitwise copy of plane 0 could come out one ulp higher and win the tie that belongs to the lower index
    const float top = fmaf(lx, p[y0 * dw + x1], hx * p[y0 * dw + x0]), bot = fmaf(lx, p[y1 * dw + x1], hx * p[y1 * dw + x0]);
    const float v = fmaf(ly, bot, hy * top);
    if (c == 0 || v > best) { best = v; arg = c; }
  }
  pred[t] = (unsigned char)arg;
}

}  // namespace

extern "C" int wseg_aff_num_offsets(int radius) { return aff_offsets(radius, nullptr, nullptr); }

extern "C" int wseg_aff_pairs(const void* feat, int ld, int C, float* aff, int N, int h, int w, int radius, int dtype, void* stream) {
  AffGeo g;
  if (int rc = aff_geo(h, w, radius, g)) return rc;
  WSEG_CHECK(feat && aff && N > 0, "aff_pairs: null pointer / empty batch");
  WSEG_CHECK(C > 0 && C % 8 == 0 && C <= 512 && ld >= C && ld % 8 == 0, "aff_pairs: C=%d ld=%d (C %% 8 == 0, C <= 512, ld >= C, ld %% 8 == 0)", C, ld);
  WSEG_CHECK(dtype == WSEG_F32 || dtype == WSEG_BF16 || dtype == WSEG_F32X3, "aff_pairs: bad dtype %d", dtype);
  const long items = (long)N * g.n_from;
  const int nwg = (int)((items + 3) / 4);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == WSEG_BF16) hipLaunchKernelGGL(aff_pairs_kernel<WSEG_BF16>, dim3(nwg), dim3(256), 0, s, feat, ld, C, aff, N, g);
  else hipLaunchKernelGGL(aff_pairs_kernel<WSEG_F32>, dim3(nwg), dim3(256), 0, s, feat, ld, C, aff, N, g);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_aff_to_dense(const float* aff, float* dense, int h, int w, int radius, void* stream) {
  AffGeo g;
  if (int rc = aff_geo(h, w, radius, g)) return rc;
  WSEG_CHECK(aff && dense, "aff_to_dense: null pointer");
  const long area = (long)h * w;
  WSEG_CHECK(area <= 65536, "aff_to_dense: a %ldx%ld dense matrix is too large", area, area);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(dense, 0, (size_t)area * area * sizeof(float), s) != hipSuccess) {
    wseg_set_error("aff_to_dense: memset failed");
    return -2;
  }
  const long total = (long)g.P * g.n_from + area;
  hipLaunchKernelGGL(aff_dense_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, aff, dense, g);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_rw_prepare(const float* aff, float* wgt, float* rsum, int N, int h, int w, int radius, int beta, void* stream) {
  AffGeo g;
  if (int rc = aff_geo(h, w, radius, g)) return rc;
  WSEG_CHECK(aff && wgt && rsum && N > 0, "rw_prepare: null pointer / empty batch");
  WSEG_CHECK(beta >= 0, "rw_prepare: beta=%d", beta);
  const long total = (long)N * h * w;
  hipLaunchKernelGGL(rw_prepare_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, aff, wgt, rsum, N, beta, g);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_random_walk(const float* wgt, const float* rsum, const float* v_in, float* v_out, int N, int planes, int h, int w, int radius,
                                int logt, void* stream) {
  AffGeo g;
  if (int rc = aff_geo(h, w, radius, g)) return rc;
  WSEG_CHECK(wgt && rsum && v_in && v_out && N > 0 && planes > 0, "random_walk: null pointer / empty batch");
  WSEG_CHECK(h * w <= WSEG_RW_MAX_PLANE, "random_walk: a %dx%d map (%d pixels) exceeds the LDS plane limit of %d pixels", h, w, h * w,
             WSEG_RW_MAX_PLANE);
  WSEG_CHECK(logt >= 0 && logt <= 20, "random_walk: logt=%d outside [0, 20]", logt);
  const size_t lds = (size_t)2 * h * w * sizeof(float);
  hipLaunchKernelGGL(random_walk_kernel, dim3(N * planes), dim3(1024), lds, (hipStream_t)stream, wgt, rsum, v_in, v_out, planes, 1 << logt, g);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_rw_pool(const float* cams, const int* src, float bg, float* pooled, int H, int W, int dh, int dw, void* stream) {
  WSEG_CHECK(src && pooled && H > 0 && W > 0, "rw_pool: null pointer / empty image");
  WSEG_CHECK(dh * 8 >= H && dw * 8 >= W && (dh - 1) * 8 < H && (dw - 1) * 8 < W, "rw_pool: %dx%d is not the pooled size of %dx%d", dh, dw, H, W);
  PlaneSrc ps;
  bool any = false;
  for (int c = 0; c < 21; ++c) { ps.src[c] = c == 0 ? -1 : src[c]; any = any || (c > 0 && src[c] >= 0); }
  WSEG_CHECK(cams || !any, "rw_pool: class planes without a CAM buffer");
  const long total = 21L * dh * dw;
  hipLaunchKernelGGL(rw_pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cams, ps, bg, pooled, H, W, dh, dw);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_rw_finish(const float* cam_rw, unsigned char* pred, int planes, int dh, int dw, int H, int W, void* stream) {
  WSEG_CHECK(cam_rw && pred && planes > 0 && planes <= 32 && H > 0 && W > 0, "rw_finish: bad arguments");
  WSEG_CHECK(dh * 8 >= H && dw * 8 >= W, "rw_finish: %dx%d upsampled x8 does not cover %dx%d", dh, dw, H, W);
  const long total = (long)H * W;
  hipLaunchKernelGGL(rw_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cam_rw, pred, planes, dh, dw, H, W);
  WSEG_LAUNCH_CHECK();
  return 0;
}
