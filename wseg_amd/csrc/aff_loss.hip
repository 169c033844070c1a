// aff_loss.hip — the AffinityNet training loss (aff_train.py:111-119 on network/resnet38_aff.py:57-63) and its gradient on the feature rows.
//
// The reference gathers two [N, C, P, n_from] tensors, reduces them to aff = exp(-mean|ft - ff|), multiplies by three [N, P, n_from] float
// label tensors built on the host (voc12/data.py:170-199) and back-propagates through the gathers as scatter-adds.  Here the labels are one
// uint8 map [N, h, w] (0 background, 1..20 a class, 255 ignore) and the three indicators of a pair are computed from its two label bytes:
//   aff_loss_forward   one wave per (image, from pixel) as aff_pairs: P affinities, the three f32 term sums and the three integer pair
//                      counts of the wave, reduced per workgroup through LDS into a [blocks][6] workspace (no atomics)
//   aff_loss_finish    one workgroup adds the partials in a fixed order (sums in f64, counts as integers) -> out[7]
//   aff_loss_backward  one wave per (image, pixel) in gather form: every pair the pixel belongs to (as "from" with its P partners, as "to" of
//                      the from pixels q - offset) adds k * sign(.) to the pixel's row, in a fixed order (no atomics, no scatter)
//   aff_pairs_backward the same row walk with the coefficient of a plain d_aff [N, P, n_from]: the backward of wseg_aff_pairs
// Nothing here is accumulated in an order that depends on scheduling: out[7] and d_feat are bit-identical from run to run.
#include "aff_geo.h"

namespace {

constexpr float kEps = 1e-5f;          // log(aff + 1e-5)
constexpr float kOnePlusEps = 1.00001f;   // log(1. + 1e-5 - aff): the reference folds the two Python floats before the tensor op

// the three indicators of voc12/data.py:191-197 from the two label bytes: 0 bg, 1 fg, 2 neg, -1 none
__device__ __forceinline__ int pair_kind(unsigned lf, unsigned lt) {
  if (lf == 255u || lt == 255u) return -1;
  if (lf != lt) return 2;
  return lf == 0u ? 0 : 1;
}

template <int DT>
__global__ __launch_bounds__(256) void aff_loss_forward_kernel(const void* __restrict__ feat, int ld, int C, const unsigned char* __restrict__ label,
                                                               float* __restrict__ aff, float* __restrict__ ws, int N, AffGeo g) {
  __shared__ float red_s[4][3];
  __shared__ int red_c[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long item = (long)blockIdx.x * 4 + wave;
  float sum[3] = {0.f, 0.f, 0.f};
  int cnt[3] = {0, 0, 0};
  if (item < (long)N * g.n_from) {                                // (wave-uniform)
    const int n = (int)(item / g.n_from), f = (int)(item - (long)n * g.n_from);
    const int fy = f / g.cw, fx = f - fy * g.cw + g.r - 1;
    const long base = (long)n * g.h * g.w;
    const long from = base + (long)fy * g.w + fx;
    const int groups = C >> 3;                                    // <= 64 (C <= 512, host-checked)
    const bool act = lane < groups;
    const int c0 = act ? lane * 8 : 0;
    float a[8];
    load8<DT>(feat, (size_t)from * ld + c0, a);
    const unsigned lf = label[from];
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
      const float v = expf(-(s / fc));
      if (aff && lane == 0) aff[((long)n * g.P + p) * g.n_from + f] = v;
      const int kind = pair_kind(lf, label[to]);
      if (kind >= 0) {
        const float t = kind == 2 ? -logf(kOnePlusEps - v) : -logf(v + kEps);
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (kind == j) { sum[j] += t; cnt[j] += 1; }
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) { red_s[wave][j] = sum[j]; red_c[wave][j] = cnt[j]; }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int j = threadIdx.x;
    float s = red_s[0][j];
    int c = red_c[0][j];
    for (int w = 1; w < 4; ++w) { s += red_s[w][j]; c += red_c[w][j]; }
    ws[(long)blockIdx.x * 6 + j] = s;
    ws[(long)blockIdx.x * 6 + 3 + j] = __int_as_float(c);
  }
}

// thread t adds the partials of blocks t, t + 256, ... in that order, then a fixed LDS tree: the order never depends on scheduling
__global__ __launch_bounds__(256) void aff_loss_finish_kernel(const float* __restrict__ ws, int blocks, float* __restrict__ out) {
  __shared__ double red_s[256][3];
  __shared__ long long red_c[256][3];
  const int t = threadIdx.x;
  double s[3] = {0., 0., 0.};
  long long c[3] = {0, 0, 0};
  for (int b = t; b < blocks; b += 256) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      s[j] += (double)ws[(long)b * 6 + j];
      c[j] += __float_as_int(ws[(long)b * 6 + 3 + j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) { red_s[t][j] = s[j]; red_c[t][j] = c[j]; }
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int j = 0; j < 3; ++j) { red_s[t][j] += red_s[t + o][j]; red_c[t][j] += red_c[t + o][j]; }
    }
    __syncthreads();
  }
  if (t == 0) {
    float loss[3], fcnt[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      fcnt[j] = (float)red_c[0][j] + kEps;                        // torch.sum(label) + 1e-5 in f32
      loss[j] = (float)(red_s[0][j] / (double)fcnt[j]);           // an empty kind: 0 / 1e-5 = 0
    }
    out[0] = loss[0] / 4.f + loss[1] / 4.f + loss[2] / 2.f;
    out[1] = loss[0]; out[2] = loss[1]; out[3] = loss[2];
    out[4] = fcnt[0]; out[5] = fcnt[1]; out[6] = fcnt[2];
  }
}

// dL/d aff of one pair times d aff / d s (s = the |diff| sum): the factor of sign(f_to - f_from) in the two rows' gradients
__device__ __forceinline__ float pair_coef(int kind, float v, const float (&w)[3], float fc) {
  const float d = kind == 2 ? w[2] / (kOnePlusEps - v) : -(kind == 0 ? w[0] : w[1]) / (v + kEps);
  return d * (-v / fc);
}

__device__ __forceinline__ float sign0(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }   // sign(0) = 0: torch's abs backward

// The row walk of the two gather-form backward kernels: the wave of pixel q = (n, y, x) visits, offset by offset, the pair q forms as "from" with
// q + offset and the pair it forms as "to" of the from pixel q - offset, and adds k * sign(f_to - f_from) to (to) / subtracts it from (from) its
// row, in that fixed order; `coef` says whether a pair counts and supplies its k.  Every row is written once (zeros where q is in no pair).
//   coef.live(pix)                         false: the pixel is in no pair that counts (its row is zero)
//   coef(n, p, f, from, to, k) -> bool     the pair (offset p, from index f) of image n between the pixel rows `from` and `to`
template <int DT, class Coef>
__device__ __forceinline__ void aff_pair_row_walk(const void* __restrict__ feat, int ld, int C, float* __restrict__ d_feat, int ld_d, int N,
                                                  const AffGeo& g, const Coef& coef) {
  const int lane = threadIdx.x & 63;
  const int area = g.h * g.w;
  const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= (long)N * area) return;
  const int n = (int)(item / area), q = (int)(item - (long)n * area);
  const int y = q / g.w, x = q - y * g.w;
  const int ch = g.h - g.r + 1, x_lo = g.r - 1, x_hi = g.w - g.r + 1;
  const long base = (long)n * area;
  const int groups = C >> 3;
  const bool act = lane < groups;
  const int c0 = act ? lane * 8 : 0;
  const bool q_from = y < ch && x >= x_lo && x < x_hi;
  float a[8], acc[8];
  load8<DT>(feat, (size_t)(base + q) * ld + c0, a);
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  if (coef.live(base + q)) {
    for (int p = 0; p < g.P; ++p) {
      float k;
      if (q_from) {                                               // q = from, partner q + offset: d f_from -= k * sign(f_to - f_from)
        const long to = base + (long)(y + g.dy[p]) * g.w + x + g.dx[p];
        if (coef(n, p, y * g.cw + (x - x_lo), base + q, to, k)) { // (wave-uniform)
          float b[8];
          load8<DT>(feat, (size_t)to * ld + c0, b);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] -= k * sign0(b[e] - a[e]);
        }
      }
      const int iy = y - g.dy[p], ix = x - g.dx[p];
      if (iy >= 0 && iy < ch && ix >= x_lo && ix < x_hi) {        // q = to of the from pixel q - offset: d f_to += k * sign(f_to - f_from)
        const long from = base + (long)iy * g.w + ix;
        if (coef(n, p, iy * g.cw + (ix - x_lo), from, base + q, k)) {
          float b[8];
          load8<DT>(feat, (size_t)from * ld + c0, b);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] += k * sign0(a[e] - b[e]);
        }
      }
    }
  }
  if (act) store8<WSEG_F32>(d_feat, (size_t)(base + q) * ld_d + c0, acc);
}

// the loss's coefficient: the pair's kind from its two label bytes, dL / d aff from the seven scalars (an ignore pixel is in no valid pair)
struct AffLossCoef {
  const unsigned char* label;
  const float* aff;
  float w[3], fc;
  int P, n_from;
  __device__ __forceinline__ bool live(long pix) const { return label[pix] != 255u; }
  __device__ __forceinline__ bool operator()(int n, int p, int f, long from, long to, float& k) const {
    const int kind = pair_kind(label[from], label[to]);
    if (kind < 0) return false;
    k = pair_coef(kind, aff[((long)n * P + p) * n_from + f], w, fc);
    return true;
  }
};

// the coefficient of aff_pairs' own backward: every pair counts, d aff / d s = -aff / C times the incoming d_aff
struct AffPairsCoef {
  const float* aff;
  const float* d_aff;
  float fc;
  int P, n_from;
  __device__ __forceinline__ bool live(long) const { return true; }
  __device__ __forceinline__ bool operator()(int n, int p, int f, long, long, float& k) const {
    const long i = ((long)n * P + p) * n_from + f;
    k = d_aff[i] * (-aff[i] / fc);
    return true;
  }
};

template <int DT>
__global__ __launch_bounds__(256) void aff_loss_backward_kernel(const void* __restrict__ feat, int ld, int C, const unsigned char* __restrict__ label,
                                                                const float* __restrict__ aff, const float* __restrict__ out7,
                                                                const float* __restrict__ gscale, float* __restrict__ d_feat, int ld_d, int N,
                                                                AffGeo g) {
  const float gs = gscale ? gscale[0] : 1.f;
  const AffLossCoef coef = {label, aff, {gs / (4.f * out7[4]), gs / (4.f * out7[5]), gs / (2.f * out7[6])}, (float)C, g.P, g.n_from};
  aff_pair_row_walk<DT>(feat, ld, C, d_feat, ld_d, N, g, coef);
}

template <int DT>
__global__ __launch_bounds__(256) void aff_pairs_backward_kernel(const void* __restrict__ feat, int ld, int C, const float* __restrict__ aff,
                                                                 const float* __restrict__ d_aff, float* __restrict__ d_feat, int ld_d, int N,
                                                                 AffGeo g) {
  const AffPairsCoef coef = {aff, d_aff, (float)C, g.P, g.n_from};
  aff_pair_row_walk<DT>(feat, ld, C, d_feat, ld_d, N, g, coef);
}

int aff_loss_check(const char* what, int ld, int C, int N, int dtype) {
  WSEG_CHECK(N > 0, "%s: empty batch", what);
  WSEG_CHECK(C > 0 && C % 8 == 0 && C <= 512 && ld >= C && ld % 8 == 0, "%s: C=%d ld=%d (C %% 8 == 0, C <= 512, ld >= C, ld %% 8 == 0)", what, C, ld);
  WSEG_CHECK(dtype == WSEG_F32 || dtype == WSEG_BF16 || dtype == WSEG_F32X3, "%s: bad dtype %d", what, dtype);
  return 0;
}

long aff_loss_blocks(long items) { return (items + 3) / 4; }

}  // namespace

extern "C" long wseg_aff_loss_workspace_bytes(int N, int h, int w, int radius) {
  AffGeo g;
  if (N <= 0 || aff_geo(h, w, radius, g)) return -1;
  return aff_loss_blocks((long)N * g.n_from) * 6 * (long)sizeof(float);
}

extern "C" int wseg_aff_loss_forward(const void* feat, int ld, int C, const unsigned char* label, float* aff, void* workspace, float* out7, int N,
                                     int h, int w, int radius, int dtype, void* stream) {
  AffGeo g;
  if (int rc = aff_geo(h, w, radius, g)) return rc;
  if (int rc = aff_loss_check("aff_loss_forward", ld, C, N, dtype)) return rc;
  WSEG_CHECK(feat && label && workspace && out7, "aff_loss_forward: null pointer");
  const long blocks = aff_loss_blocks((long)N * g.n_from);
  WSEG_CHECK(blocks < (1L << 31), "aff_loss_forward: batch too large");
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  if (dtype == WSEG_BF16) hipLaunchKernelGGL(aff_loss_forward_kernel<WSEG_BF16>, dim3((unsigned)blocks), dim3(256), 0, s, feat, ld, C, label, aff, ws, N, g);
  else hipLaunchKernelGGL(aff_loss_forward_kernel<WSEG_F32>, dim3((unsigned)blocks), dim3(256), 0, s, feat, ld, C, label, aff, ws, N, g);
  WSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL(aff_loss_finish_kernel, dim3(1), dim3(256), 0, s, ws, (int)blocks, out7);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_aff_loss_backward(const void* feat, int ld, int C, const unsigned char* label, const float* aff, const float* out7,
                                      const float* gscale, float* d_feat, int ld_d, int N, int h, int w, int radius, int dtype, void* stream) {
  AffGeo g;
  if (int rc = aff_geo(h, w, radius, g)) return rc;
  if (int rc = aff_loss_check("aff_loss_backward", ld, C, N, dtype)) return rc;
  WSEG_CHECK(ld_d >= C && ld_d % 8 == 0, "aff_loss_backward: C=%d ld_d=%d (ld_d >= C, ld_d %% 8 == 0)", C, ld_d);
  WSEG_CHECK(feat && label && aff && out7 && d_feat, "aff_loss_backward: null pointer");
  const long blocks = aff_loss_blocks((long)N * h * w);
  WSEG_CHECK(blocks < (1L << 31), "aff_loss_backward: batch too large");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == WSEG_BF16)
    hipLaunchKernelGGL(aff_loss_backward_kernel<WSEG_BF16>, dim3((unsigned)blocks), dim3(256), 0, s, feat, ld, C, label, aff, out7, gscale, d_feat, ld_d, N, g);
  else
    hipLaunchKernelGGL(aff_loss_backward_kernel<WSEG_F32>, dim3((unsigned)blocks), dim3(256), 0, s, feat, ld, C, label, aff, out7, gscale, d_feat, ld_d, N, g);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_aff_pairs_backward(const void* feat, int ld, int C, const float* aff, const float* d_aff, float* d_feat, int ld_d, int N,
                                       int h, int w, int radius, int dtype, void* stream) {
  AffGeo g;
  if (int rc = aff_geo(h, w, radius, g)) return rc;
  if (int rc = aff_loss_check("aff_pairs_backward", ld, C, N, dtype)) return rc;
  WSEG_CHECK(ld_d >= C && ld_d % 8 == 0, "aff_pairs_backward: C=%d ld_d=%d (ld_d >= C, ld_d %% 8 == 0)", C, ld_d);
  WSEG_CHECK(feat && aff && d_aff && d_feat, "aff_pairs_backward: null pointer");
  const long blocks = aff_loss_blocks((long)N * h * w);
  WSEG_CHECK(blocks < (1L << 31), "aff_pairs_backward: batch too large");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == WSEG_BF16)
    hipLaunchKernelGGL(aff_pairs_backward_kernel<WSEG_BF16>, dim3((unsigned)blocks), dim3(256), 0, s, feat, ld, C, aff, d_aff, d_feat, ld_d, N, g);
  else
    hipLaunchKernelGGL(aff_pairs_backward_kernel<WSEG_F32>, dim3((unsigned)blocks), dim3(256), 0, s, feat, ld, C, aff, d_aff, d_feat, ld_d, N, g);
  WSEG_LAUNCH_CHECK();
  return 0;
}
