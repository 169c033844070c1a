// crf.hip — fully connected CRF (mean field) with EXACT Gaussian kernels, the refinement contrast_infer.py:102-134 (--out_crf) and
// aff_prepare.py:34-50 ask of pydensecrf.  pydensecrf approximates both filters with a permutohedral lattice; here every pair is evaluated:
//
//   filter(Q)[i][c] = n_i * sum_j k(f_i, f_j) * n_j * Q[j][c],   k = exp(-|f_i - f_j|^2 / 2),   n_i = 1 / sqrt(sum_j k(f_i, f_j) + 1e-20)
//   (DIAG_KERNEL + NORMALIZE_SYMMETRIC; the sum includes j = i)
//   bilateral f = (x/sxy, y/sxy, r/srgb, g/srgb, b/srgb): all pairs, crf_bilateral_kernel (the hot path: N^2 = 3.5e10 pairs at 375x500)
//   Gaussian  f = (x/sxy, y/sxy): separable, two 1-D passes over a window of radius ceil(6.5 sxy) (relative tail mass exp(-6.5^2/2) = 7e-10)
//   update: logit = -U + w_g filter_g(Q) + w_b filter_b(Q), Q = softmax(logit); U follows from the label (two values), never stored
//
// crf_bilateral_kernel, tiled like pcm.hip: one workgroup = 128 output pixels i (32 per wave, one pixel per lane&15 in two blocks),
// the source pixels j stream through LDS in 64-pixel tiles by LDS-DMA (double buffered).  Both buffers are stored so that a tile
// is one contiguous piece of global memory and every LDS read is a conflict-free ds_read_b128:
//   feat [npad/4][8][4]   f32: quad q = j>>2, feature (x, y, r, g, b, 0, 0, 0), slot j&3 — INTEGER values (< 2^24), so every difference is exact
//   Qn   [npad/4][NC][4]  f32: quad, column (label set s, label c) -> s*M + c, slot j&3;  Qn = n_j * Q, zero rows for j >= N
// A lane (p = lane&15, g = lane>>4) evaluates k(i = p, j = 4g + r) for r = 0..3 on the VALU as exp2 of
//   -(log2 e / 2) * ((dx^2 + dy^2) / sxy^2 + (dr^2 + dg^2 + db^2) / srgb^2)
// — from DIFFERENCES (always exact), their squared sums exact while H^2 + W^2 < 2^24 (merely rounded beyond); the expanded form f_i.f_j - |f_i|^2/2 - |f_j|^2/2 would cancel at |f|^2 ~ 8000.
// These four values ARE the A operand of four v_mfma_f32_16x16x4_f32 (m = p, k = g <-> source 4g + r); B is one float of the lane's
// ds_read_b128 of Qn (k = g, n = column): out[i][c] accumulates in exact f32 (an fmaf chain), NC / 16 MFMAs per (r, output block).
// S label sets of one image share every k: NC = 16 * ceil(S * M / 16) columns.
#include "common.h"
#include <math.h>

namespace {

constexpr int JT = 64;                       // source pixels per LDS tile
constexpr int FQ = 128;                      // bytes of one feature quad [8][4] f32
constexpr int F_TILE = (JT / 4) * FQ;        // 2048
constexpr int FLUSH = 4;                     // tiles per first-level sum (256 sources)
constexpr int WG_PIX = WSEG_CRF_PIX_ALIGN;   // 128 output pixels per workgroup

template <int NT>
__global__ __launch_bounds__(256, 2) void crf_bilateral_kernel(const float* __restrict__ feat, const float* __restrict__ Qn,
                                                               float* __restrict__ out, int npad, float ncs, float ncr) {
  constexpr int NC = NT * 16;
  constexpr int Q_TILE = (JT / 4) * NC * 16;                 // NT * 4096 B
  constexpr int BUF = F_TILE + Q_TILE;
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p = lane & 15, g = lane >> 4;
  const int i0 = blockIdx.x * WG_PIX + wid * 32;

  float fi[2][5];
#pragma unroll
  for (int ob = 0; ob < 2; ++ob) {
    const int i = i0 + ob * 16 + p;                          // < npad: feat is padded
    const float* src = feat + (size_t)(i >> 2) * 32 + (i & 3);
#pragma unroll
    for (int f = 0; f < 5; ++f) fi[ob][f] = src[f * 4];
  }

  // a tile is contiguous in both buffers: Q_TILE bytes = 4*NT wave pieces of 1 KiB (NT per wave), F_TILE = 2 pieces (waves 0, 1)
  auto stage = [&](int buf, int j0) {
    char* lf = smem + buf * BUF;
    char* lq = lf + F_TILE;
    const char* qsrc = reinterpret_cast<const char*>(Qn) + (size_t)(j0 >> 2) * NC * 16;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int piece = wid * NT + t;
      glds16(qsrc + piece * 1024 + lane * 16, lq + piece * 1024);
    }
    if (wid < 2) glds16(reinterpret_cast<const char*>(feat) + (size_t)(j0 >> 2) * FQ + wid * 1024 + lane * 16, lf + wid * 1024);
  };

  // two-level sum: acc runs over FLUSH tiles (256 sources), then joins tot — the rounding chain of a 187 500-term sum is
  // 256 + N/256 long instead of N
  f32x4 acc[2][NT], tot[2][NT];
#pragma unroll
  for (int ob = 0; ob < 2; ++ob)
#pragma unroll
    for (int t = 0; t < NT; ++t) { acc[ob][t] = (f32x4){0.f, 0.f, 0.f, 0.f}; tot[ob][t] = (f32x4){0.f, 0.f, 0.f, 0.f}; }

  const int ntile = npad / JT;
  stage(0, 0);
  __syncthreads();
  int cur = 0;
  for (int it = 0; it < ntile; ++it) {
    if (it + 1 < ntile) stage(cur ^ 1, (it + 1) * JT);
    const char* lf = smem + cur * BUF;
    const char* lq = lf + F_TILE;
#pragma unroll
    for (int b = 0; b < JT / 16; ++b) {
      const int quad = b * 4 + g;                            // sources 16b + 4g + r
      f32x4 fj[5];
#pragma unroll
      for (int f = 0; f < 5; ++f) fj[f] = *reinterpret_cast<const f32x4*>(lf + (quad * 8 + f) * 16);
      f32x4 qv[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) qv[t] = *reinterpret_cast<const f32x4*>(lq + ((quad * NC) + t * 16 + p) * 16);
      float kv[2][4];
#pragma unroll
      for (int ob = 0; ob < 2; ++ob)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float dx = fj[0][r] - fi[ob][0], dy = fj[1][r] - fi[ob][1];
          const float dr = fj[2][r] - fi[ob][2], dg = fj[3][r] - fi[ob][3], db = fj[4][r] - fi[ob][4];
          const float d_xy = fmaf(dy, dy, dx * dx);
          const float d_c = fmaf(db, db, fmaf(dg, dg, dr * dr));
          kv[ob][r] = __builtin_amdgcn_exp2f(fmaf(d_xy, ncs, d_c * ncr));
        }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int ob = 0; ob < 2; ++ob) acc[ob][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kv[ob][r], qv[t][r], acc[ob][t], 0, 0, 0);
    }
    if ((it & (FLUSH - 1)) == FLUSH - 1 || it == ntile - 1) {
#pragma unroll
      for (int ob = 0; ob < 2; ++ob)
#pragma unroll
        for (int t = 0; t < NT; ++t) { tot[ob][t] += acc[ob][t]; acc[ob][t] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    }
    __syncthreads();
    cur ^= 1;
  }

  // tot[ob][t][reg] <-> (i = i0 + 16 ob + 4g + reg, column t*16 + p)
#pragma unroll
  for (int ob = 0; ob < 2; ++ob)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      float* dst = out + (size_t)(i0 + ob * 16 + 4 * g + reg) * NC + p;
#pragma unroll
      for (int t = 0; t < NT; ++t) dst[t * 16] = tot[ob][t][reg];
    }
}

// truncated 1-D sum of the Gaussian weights around position x of a line of `len` pixels
__device__ __forceinline__ float gauss_line_sum(int x, int len, int R, float nc) {
  float s = 0.f;
  for (int d = -R; d <= R; ++d) {
    const int xx = x + d;
    if (xx >= 0 && xx < len) s += expf(nc * (float)(d * d));
  }
  return s;
}

// per pixel slot i < npad: integer features, the unit column the normalisation pass filters, and the Gaussian's n_i
__global__ __launch_bounds__(256) void crf_prepare_kernel(const unsigned char* __restrict__ img, int H, int W, int npad, int R, float nc,
                                                          float* __restrict__ feat, float* __restrict__ ones, float* __restrict__ ng) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= npad) return;
  const int N = H * W;
  const bool in = i < N;
  const int y = in ? i / W : 0, x = in ? i - y * W : 0;
  float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (in) {
    f[0] = (float)x; f[1] = (float)y;
    f[2] = (float)img[(size_t)i * 3]; f[3] = (float)img[(size_t)i * 3 + 1]; f[4] = (float)img[(size_t)i * 3 + 2];
  }
  float* fd = feat + (size_t)(i >> 2) * 32 + (i & 3);
#pragma unroll
  for (int k = 0; k < 8; ++k) fd[k * 4] = f[k];
  float* od = ones + (size_t)(i >> 2) * 64 + (i & 3);
#pragma unroll
  for (int c = 0; c < 16; ++c) od[c * 4] = (c == 0 && in) ? 1.f : 0.f;
  if (in) ng[i] = 1.f / sqrtf(gauss_line_sum(x, W, R, nc) * gauss_line_sum(y, H, R, nc) + 1e-20f);
}

__global__ __launch_bounds__(256) void crf_rsqrt_kernel(const float* __restrict__ sums, int stride, float* __restrict__ n, int N) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < N) n[i] = 1.f / sqrtf(sums[(size_t)i * stride] + 1e-20f);
}

// one 1-D pass of the separable Gaussian over [planes][H][W]; VERT: along y
template <int VERT>
__global__ __launch_bounds__(256) void crf_gauss_kernel(const float* __restrict__ in, float* __restrict__ out, long total, int H, int W, int R,
                                                        float nc) {
  extern __shared__ float wtab[];                            // [R + 1]
  for (int d = threadIdx.x; d <= R; d += 256) wtab[d] = expf(nc * (float)(d * d));
  __syncthreads();
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % W);
  const int y = (int)((idx / W) % H);
  const int pos = VERT ? y : x, len = VERT ? H : W;
  const long step = VERT ? W : 1;
  const int lo = max(-R, -pos), hi = min(R, len - 1 - pos);
  float acc = 0.f;
  for (int d = lo; d <= hi; ++d) acc = fmaf(wtab[d < 0 ? -d : d], in[idx + d * step], acc);
  out[idx] = acc;
}

struct CrfSrc { int src[WSEG_CRF_MAX_LABELS]; };

// labels[i] = argmax_c tensor[c][i] (the first maximum wins, numpy's rule); tensor[c] = cams[src[c]] (0 without a plane),
// tensor[0] = bg (rule 0) or (1 - max_c tensor[c])^alpha with tensor[0] = 0 inside the max (rule 1, aff_prepare.py:61)
__global__ __launch_bounds__(256) void crf_labels_kernel(const float* __restrict__ cams, CrfSrc ps, int M, int rule, float param,
                                                         unsigned char* __restrict__ labels, int N) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  float cmax = 0.f, best = 0.f;
  int arg = 0;
  bool any = false;
  for (int c = 1; c < M; ++c) {
    const int s = ps.src[c];
    const float v = s >= 0 ? cams[(size_t)s * N + i] : 0.f;
    cmax = fmaxf(cmax, v);
    if (!any || v > best) { best = v; arg = c; any = true; }
  }
  const float bg = rule == 0 ? param : powf(1.f - cmax, param);
  if (!any || !(best > bg)) arg = 0;                         // bg wins ties (index 0) and a NaN bg stays the arg-max, as in numpy
  labels[i] = (unsigned char)arg;
}

struct CrfUpd {
  const unsigned char* labels;     // [S][N]
  const float* prob;               // [M][N]: the unary's source in place of `labels` (crf_update_kernel<true>, S = 1)
  const float* outb;               // [npad][NC] unnormalised bilateral sums (null: the initial Q = softmax(-U))
  const float* outg;               // [S*M][N]   unnormalised Gaussian sums
  const float* nb; const float* ng;
  float* Qn; float* Qg;            // next iteration's filter inputs
  float* Qout; float* logits;      // [S][M][N], nullable
  unsigned char* amax;             // [S][N], nullable
  int S, M, N, npad, NC;
  float pe, ne, wb, wg;
};

// -U[c] at pixel i: unary_from_labels (gt_prob at the pixel's label) or, PROB, unary_from_softmax: ln(clip(prob[c][i], 1e-5, 1))
template <bool PROB>
__device__ __forceinline__ float crf_neg_unary(const CrfUpd& a, int c, int lab, int i) {
  if constexpr (PROB) return logf(fminf(fmaxf(a.prob[(size_t)c * a.N + i], 1e-5f), 1.f));
  else return -(c == lab ? a.pe : a.ne);
}

template <bool PROB>
__global__ __launch_bounds__(256) void crf_update_kernel(CrfUpd a) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)a.S * a.npad) return;
  const int s = (int)(t / a.npad), i = (int)(t - (long)s * a.npad);
  float* qn = a.Qn + ((size_t)(i >> 2) * a.NC) * 4 + (i & 3);
  if (s == 0)
    for (int c = a.S * a.M; c < a.NC; ++c) qn[c * 4] = 0.f;  // unused columns stay finite
  if (i >= a.N) {
    for (int c = 0; c < a.M; ++c) qn[(s * a.M + c) * 4] = 0.f;
    return;
  }
  const int lab = PROB ? 0 : a.labels[(size_t)s * a.N + i];
  const float nbi = a.nb[i], ngi = a.ng[i];
  float lg[WSEG_CRF_MAX_LABELS];
  float mx = -INFINITY;
  int arg = 0;
#pragma unroll
  for (int c = 0; c < WSEG_CRF_MAX_LABELS; ++c) {
    if (c < a.M) {
      float v = crf_neg_unary<PROB>(a, c, lab, i);
      if (a.outb) {
        const float fg = ngi * a.outg[(size_t)(s * a.M + c) * a.N + i];
        const float fb = nbi * a.outb[(size_t)i * a.NC + s * a.M + c];
        v = v + a.wg * fg + a.wb * fb;
      }
      lg[c] = v;
      if (v > mx) { mx = v; arg = c; }
    }
  }
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < WSEG_CRF_MAX_LABELS; ++c)
    if (c < a.M) { lg[c] = expf(lg[c] - mx); sum += lg[c]; }
  const float inv = 1.f / sum;
#pragma unroll
  for (int c = 0; c < WSEG_CRF_MAX_LABELS; ++c) {
    if (c < a.M) {
      const float q = lg[c] * inv;
      const size_t pl = (size_t)(s * a.M + c) * a.N + i;
      qn[(s * a.M + c) * 4] = q * nbi;
      a.Qg[pl] = q * ngi;
      if (a.Qout) a.Qout[pl] = q;
    }
  }
  if (a.logits) {                                            // recomputed: lg[] now holds the exponentials
    for (int c = 0; c < a.M; ++c) {
      float v = crf_neg_unary<PROB>(a, c, lab, i);
      if (a.outb) {
        const float fg = ngi * a.outg[(size_t)(s * a.M + c) * a.N + i];
        const float fb = nbi * a.outb[(size_t)i * a.NC + s * a.M + c];
        v = v + a.wg * fg + a.wb * fb;
      }
      a.logits[(size_t)(s * a.M + c) * a.N + i] = v;
    }
  }
  if (a.amax) a.amax[(size_t)s * a.N + i] = (unsigned char)arg;
}

int gauss_radius(float sxy) { return (int)ceilf(6.5f * sxy); }

}  // namespace

extern "C" int wseg_crf_padded_pixels(int npix) { return (npix + WG_PIX - 1) / WG_PIX * WG_PIX; }
extern "C" int wseg_crf_columns(int S, int M) { return (S * M + 15) / 16 * 16; }

extern "C" int wseg_crf_labels(const float* cams, const int* src, int n_labels, int rule, float param, unsigned char* labels, int npix,
                               void* stream) {
  WSEG_CHECK(src && labels && npix > 0, "crf_labels: null pointer / empty image");
  WSEG_CHECK(n_labels >= 2 && n_labels <= WSEG_CRF_MAX_LABELS, "crf_labels: n_labels=%d outside [2, %d]", n_labels, WSEG_CRF_MAX_LABELS);
  WSEG_CHECK(rule == WSEG_CRF_BG_CONST || rule == WSEG_CRF_BG_POWER, "crf_labels: unknown background rule %d", rule);
  CrfSrc ps;
  bool any = false;
  for (int c = 0; c < WSEG_CRF_MAX_LABELS; ++c) {
    ps.src[c] = (c == 0 || c >= n_labels) ? -1 : src[c];
    any = any || ps.src[c] >= 0;
  }
  WSEG_CHECK(cams || !any, "crf_labels: class planes without a CAM buffer");
  hipLaunchKernelGGL(crf_labels_kernel, dim3((npix + 255) / 256), dim3(256), 0, (hipStream_t)stream, cams, ps, n_labels, rule, param, labels, npix);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_crf_prepare(const unsigned char* img, int H, int W, float gauss_sxy, float* feat, float* ones, float* ng, void* stream) {
  WSEG_CHECK(img && feat && ones && ng && H > 0 && W > 0, "crf_prepare: null pointer / empty image");
  WSEG_CHECK((long)H * W <= (1L << 24), "crf_prepare: %dx%d exceeds 2^24 pixels", H, W);
  WSEG_CHECK(gauss_sxy > 0.f && gauss_radius(gauss_sxy) <= WSEG_CRF_MAX_RADIUS, "crf_prepare: Gaussian sxy=%g outside (0, %g]", gauss_sxy,
             WSEG_CRF_MAX_RADIUS / 6.5);
  const int npad = wseg_crf_padded_pixels(H * W);
  hipLaunchKernelGGL(crf_prepare_kernel, dim3(npad / 256 + 1), dim3(256), 0, (hipStream_t)stream, img, H, W, npad, gauss_radius(gauss_sxy),
                     -0.5f / (gauss_sxy * gauss_sxy), feat, ones, ng);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_crf_bilateral(const float* feat, const float* Qn, float* out, int npix, int ncols, float sxy, float srgb, void* stream) {
  WSEG_CHECK(feat && Qn && out && npix > 0, "crf_bilateral: null pointer / empty image");
  WSEG_CHECK(ncols > 0 && ncols % 16 == 0 && ncols <= WSEG_CRF_MAX_COLUMNS, "crf_bilateral: %d columns (a multiple of 16, at most %d)", ncols,
             WSEG_CRF_MAX_COLUMNS);
  WSEG_CHECK(sxy > 0.f && srgb > 0.f, "crf_bilateral: sxy=%g srgb=%g", sxy, srgb);
  const int npad = wseg_crf_padded_pixels(npix);
  const float h = 0.72134752044448170368f;                   // log2(e) / 2
  const float ncs = -h / (sxy * sxy), ncr = -h / (srgb * srgb);
  const dim3 grid(npad / WG_PIX);
  hipStream_t s = (hipStream_t)stream;
  switch (ncols / 16) {
    case 1: hipLaunchKernelGGL(crf_bilateral_kernel<1>, grid, dim3(256), 0, s, feat, Qn, out, npad, ncs, ncr); break;
    case 2: hipLaunchKernelGGL(crf_bilateral_kernel<2>, grid, dim3(256), 0, s, feat, Qn, out, npad, ncs, ncr); break;
    case 3: hipLaunchKernelGGL(crf_bilateral_kernel<3>, grid, dim3(256), 0, s, feat, Qn, out, npad, ncs, ncr); break;
    default: hipLaunchKernelGGL(crf_bilateral_kernel<4>, grid, dim3(256), 0, s, feat, Qn, out, npad, ncs, ncr); break;
  }
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_crf_rsqrt(const float* sums, int stride, float* n, int npix, void* stream) {
  WSEG_CHECK(sums && n && npix > 0 && stride > 0, "crf_rsqrt: bad arguments");
  hipLaunchKernelGGL(crf_rsqrt_kernel, dim3((npix + 255) / 256), dim3(256), 0, (hipStream_t)stream, sums, stride, n, npix);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_crf_gaussian(const float* in, float* tmp, float* out, int planes, int H, int W, float sxy, void* stream) {
  WSEG_CHECK(in && tmp && out && planes > 0 && H > 0 && W > 0, "crf_gaussian: null pointer / empty image");
  WSEG_CHECK(sxy > 0.f && gauss_radius(sxy) <= WSEG_CRF_MAX_RADIUS, "crf_gaussian: sxy=%g outside (0, %g]", sxy, WSEG_CRF_MAX_RADIUS / 6.5);
  const int R = gauss_radius(sxy);
  const float nc = -0.5f / (sxy * sxy);
  const long total = (long)planes * H * W;
  const dim3 grid((unsigned)((total + 255) / 256));
  const size_t lds = (size_t)(R + 1) * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(crf_gauss_kernel<0>, grid, dim3(256), lds, s, in, tmp, total, H, W, R, nc);
  WSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL(crf_gauss_kernel<1>, grid, dim3(256), lds, s, (const float*)tmp, out, total, H, W, R, nc);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_crf_update(const unsigned char* labels, const float* outb, const float* outg, const float* nb, const float* ng, float* Qn,
                               float* Qg, float* Qout, float* logits, unsigned char* amax, int S, int n_labels, int npix, float gt_prob,
                               float w_bilateral, float w_gaussian, void* stream) {
  WSEG_CHECK(labels && nb && ng && Qn && Qg && npix > 0, "crf_update: null pointer / empty image");
  WSEG_CHECK((outb == nullptr) == (outg == nullptr), "crf_update: the two filter outputs come together (both null: initial Q)");
  WSEG_CHECK(n_labels >= 2 && n_labels <= WSEG_CRF_MAX_LABELS, "crf_update: n_labels=%d outside [2, %d]", n_labels, WSEG_CRF_MAX_LABELS);
  WSEG_CHECK(S >= 1 && wseg_crf_columns(S, n_labels) <= WSEG_CRF_MAX_COLUMNS, "crf_update: %d label sets of %d labels exceed %d columns", S,
             n_labels, WSEG_CRF_MAX_COLUMNS);
  WSEG_CHECK(gt_prob > 0.f && gt_prob < 1.f, "crf_update: gt_prob=%g outside (0, 1)", gt_prob);
  CrfUpd a;
  a.prob = nullptr;
  a.labels = labels; a.outb = outb; a.outg = outg; a.nb = nb; a.ng = ng; a.Qn = Qn; a.Qg = Qg; a.Qout = Qout; a.logits = logits; a.amax = amax;
  a.S = S; a.M = n_labels; a.N = npix; a.npad = wseg_crf_padded_pixels(npix); a.NC = wseg_crf_columns(S, n_labels);
  a.pe = -logf(gt_prob); a.ne = -logf((1.f - gt_prob) / (float)(n_labels - 1));
  a.wb = w_bilateral; a.wg = w_gaussian;
  const long total = (long)S * a.npad;
  hipLaunchKernelGGL(crf_update_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_crf_update_prob(const float* prob, const float* outb, const float* outg, const float* nb, const float* ng, float* Qn,
                                    float* Qg, float* Qout, float* logits, unsigned char* amax, int n_labels, int npix, float w_bilateral,
                                    float w_gaussian, void* stream) {
  WSEG_CHECK(prob && nb && ng && Qn && Qg && npix > 0, "crf_update_prob: null pointer / empty image");
  WSEG_CHECK((outb == nullptr) == (outg == nullptr), "crf_update_prob: the two filter outputs come together (both null: initial Q)");
  WSEG_CHECK(n_labels >= 2 && n_labels <= WSEG_CRF_MAX_LABELS, "crf_update_prob: n_labels=%d outside [2, %d]", n_labels, WSEG_CRF_MAX_LABELS);
  CrfUpd a;
  a.prob = prob;
  a.labels = nullptr; a.outb = outb; a.outg = outg; a.nb = nb; a.ng = ng; a.Qn = Qn; a.Qg = Qg; a.Qout = Qout; a.logits = logits; a.amax = amax;
  a.S = 1; a.M = n_labels; a.N = npix; a.npad = wseg_crf_padded_pixels(npix); a.NC = wseg_crf_columns(1, n_labels);
  a.pe = a.ne = 0.f;
  a.wb = w_bilateral; a.wg = w_gaussian;
  hipLaunchKernelGGL(crf_update_kernel<true>, dim3((unsigned)((a.npad + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  WSEG_LAUNCH_CHECK();
  return 0;
}
