// seg_head.hip — the DeepLab-v1 head in training mode (segmentation/lib/net/deeplabv1.py:42-49: conv_fov -> bn_fov -> relu -> conv_fov2 -> bn_fov2
// -> relu -> dropout(0.5) -> cls_conv, built with plain nn.BatchNorm2d, train.py:52) on pixel rows [M][ld], f32 or bf16: everything between the
// three convolutions, forward and backward.
//   bn_stats          F.batch_norm(training=True)'s statistics: per column mean, invstd = 1/sqrt(var + eps) (biased var), the folded
//                     scale = gamma * invstd and shift = beta - mean * scale, and the running update (running_var from the unbiased variance)
//   bn_relu_drop      y = relu(z * scale[c] + shift[c]) [* keep / (1 - p)], rounded once to y's dtype; the keep bit is a counter hash of
//                     (row * C + col, key): no mask tensor exists
//   bn_relu_backward  dy = s * g * [y > 0]; s1 = sum dy, s2 = sum dy * xhat; dz = gamma * invstd * (dy - s1/M - xhat * s2/M)
//   col_sums          out[c] = sum over the rows (cls_conv's d_bias from the [M][24] gradient rows)
// One reduction machine serves the three column reductions.  A workgroup owns a chunk of R consecutive rows (sh_rows_per_chunk: 32 rows, more
// once M passes 16384 so that at most 512 chunks exist) and 512 columns: one wave covers a 512-column row with 16-byte (bf16) loads, the four
// waves take the rows r0 + wave, r0 + wave + 4, ...; every lane keeps its 8 columns' sums in f32 registers, the four waves' sums are added in
// the fixed order (w0 + w1) + (w2 + w3) and go to the caller's workspace as partials [chunk][slot][C].  A finish launch adds the partials
// in f64, ONE workgroup per 64 columns (a column's whole sum is one workgroup's): 16 groups of 64 threads walk the chunks g, g + 16, ...,
// eight partials' loads in flight at a time, then a fixed LDS tree over the groups.
// No kernel uses atomics and no order depends on scheduling: every output is bit-identical from run to run.  Nothing synchronises with the host.
//
// The variance is never E[x^2] - mean^2 in f32.  A chunk's partial is (shift, sum (x - shift), sum (x - shift)^2) with shift = the chunk's first
// row: the f32 sums are of the size of the column's spread, not of its mean.  The finish re-centres every partial about chunk 0's shift g in
// f64 (d = shift_k - g: S1 += s1 + n d, S2 += s2 + 2 d s1 + n d^2) and takes mean = g + S1/M, var = (S2 - S1^2/M)/M in f64, where the
// cancellation costs (mean - g)^2 / var * 2^-53.  A constant column gives every difference exactly 0: var = 0, invstd = 1/sqrt(eps).
#include <algorithm>
#include "common.h"

namespace {

constexpr int SH_COLS = 512;                                     // columns of a workgroup: 64 lanes x 8
constexpr int SH_MAX_CHUNKS = 512;
constexpr int SH_BATCH = 8;                                      // partials a finish thread loads before it adds them (a load's latency, not its bytes, is the cost)

inline int sh_rows_per_chunk(long M) {
  const long r = ((M + SH_MAX_CHUNKS - 1) / SH_MAX_CHUNKS + 3) / 4 * 4;
  return (int)std::max(32L, r);
}
inline int sh_chunks(long M) { return (int)((M + sh_rows_per_chunk(M) - 1) / sh_rows_per_chunk(M)); }

// ---- the per-element parts of the three reductions: K f32 sums per column.  begin() runs once per lane, add() once per row.
template <int DT>
struct StatsOp {                                                  // slots: shift, sum d, sum d^2 with d = x - shift
  static constexpr int K = 3;
  const void* x; int ld;
  struct Ref { float sh[8]; };
  __device__ __forceinline__ void begin(long r0, int c0, int wave, Ref& ref, float (&acc)[K][8]) const {
    load8<DT>(x, (size_t)r0 * ld + c0, ref.sh);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[0][e] = wave == 0 ? ref.sh[e] : 0.f;       // (the four waves' sum is the shift itself: s + 0 + 0 + 0)
  }
  __device__ __forceinline__ void add(long r, int c0, const Ref& ref, float (&acc)[K][8]) const {
    float v[8];
    load8<DT>(x, (size_t)r * ld + c0, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float d = v[e] - ref.sh[e];
      acc[1][e] += d;
      acc[2][e] = __builtin_fmaf(d, d, acc[2][e]);
    }
  }
};

template <int GDT, int DT>
struct BwdOp {                                                    // slots: sum dy, sum dy * xhat
  static constexpr int K = 2;
  const void* g; const void* y; const void* z;
  int ld_g, ld_y, ld_z;
  const float* mean; const float* invstd;
  float s;
  struct Ref { float mean[8], invstd[8]; };
  __device__ __forceinline__ void begin(long, int c0, int, Ref& ref, float (&)[K][8]) const {
    load8<WSEG_F32>(mean, c0, ref.mean);
    load8<WSEG_F32>(invstd, c0, ref.invstd);
  }
  __device__ __forceinline__ void add(long r, int c0, const Ref& ref, float (&acc)[K][8]) const {
    float a[8], b[8], v[8];
    load8<GDT>(g, (size_t)r * ld_g + c0, a);
    load8<DT>(y, (size_t)r * ld_y + c0, b);
    load8<DT>(z, (size_t)r * ld_z + c0, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float dy = b[e] > 0.f ? s * a[e] : 0.f;
      const float xhat = (v[e] - ref.mean[e]) * ref.invstd[e];
      acc[0][e] += dy;
      acc[1][e] = __builtin_fmaf(dy, xhat, acc[1][e]);
    }
  }
};

template <int DT>
struct SumOp {
  static constexpr int K = 1;
  const void* x; int ld;
  struct Ref {};
  __device__ __forceinline__ void begin(long, int, int, Ref&, float (&)[K][8]) const {}
  __device__ __forceinline__ void add(long r, int c0, const Ref&, float (&acc)[K][8]) const {
    float v[8];
    load8<DT>(x, (size_t)r * ld + c0, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[0][e] += v[e];
  }
};

// part[chunk][k][C] = the sums of rows [chunk * R, min(M, (chunk + 1) * R)); C % 8 == 0; grid (chunks, ceil(C / 512))
template <class Op>
__global__ __launch_bounds__(256) void sh_reduce_kernel(Op op, long M, int C, int R, float* __restrict__ part) {
  constexpr int K = Op::K;
  __shared__ float red[4][K][SH_COLS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c0 = (blockIdx.y * 64 + lane) * 8;
  const long r0 = (long)blockIdx.x * R;
  const long r1 = r0 + R < M ? r0 + R : M;
  float acc[K][8];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[k][e] = 0.f;
  if (c0 < C) {
    typename Op::Ref ref;
    op.begin(r0, c0, wave, ref, acc);
#pragma unroll 4
    for (long r = r0 + wave; r < r1; r += 4) op.add(r, c0, ref, acc);     // (unrolled: several rows' loads in flight; the adds keep their order)
  }
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) red[wave][k][lane * 8 + e] = acc[k][e];
  __syncthreads();
  for (int i = threadIdx.x; i < K * SH_COLS; i += 256) {
    const int k = i / SH_COLS, j = i - k * SH_COLS;
    const int c = blockIdx.y * SH_COLS + j;
    if (c < C) part[((size_t)blockIdx.x * K + k) * C + c] = (red[0][k][j] + red[1][k][j]) + (red[2][k][j] + red[3][k][j]);
  }
}

// the fixed tree over the 16 groups of the finish workgroup (1024 threads: group = t / 64, lane = t % 64); the total ends in red[0][k][lane]
template <int K>
__device__ __forceinline__ void sh_tree16(double (&red)[16][K][64], const double (&s)[K], int grp, int lane) {
#pragma unroll
  for (int k = 0; k < K; ++k) red[grp][k][lane] = s[k];
  __syncthreads();
  for (int o = 8; o > 0; o >>= 1) {
    if (grp < o) {
#pragma unroll
      for (int k = 0; k < K; ++k) red[grp][k][lane] += red[grp + o][k][lane];
    }
    __syncthreads();
  }
}

struct StatsOut {
  const float* gamma; const float* beta;
  float* mean; float* invstd; float* scale; float* shift; float* running_mean; float* running_var;
  double eps, momentum;
};

__global__ __launch_bounds__(1024) void sh_stats_finish_kernel(const float* __restrict__ part, int chunks, long M, int C, int R, StatsOut o) {
  __shared__ double red[16][2][64];
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  for (int cb = blockIdx.x * 64; cb < C; cb += gridDim.x * 64) {       // (launched with one workgroup per 64 columns: one pass)
    const int c = cb + lane;
    double s[2] = {0., 0.};
    double g = 0.;
    if (c < C) {
      g = (double)part[c];                                         // chunk 0's shift: the centre every partial is moved to
      for (int b0 = grp; b0 < chunks; b0 += 16 * SH_BATCH) {       // SH_BATCH partials' loads in flight, then added in the order of b
        float v[SH_BATCH][3];
#pragma unroll
        for (int j = 0; j < SH_BATCH; ++j) {
          const int b = b0 + 16 * j;
          const float* p = part + (size_t)(b < chunks ? b : b0) * 3 * C + c;
          v[j][0] = p[0]; v[j][1] = p[C]; v[j][2] = p[2 * (size_t)C];
        }
#pragma unroll
        for (int j = 0; j < SH_BATCH; ++j) {
          const int b = b0 + 16 * j;
          if (b < chunks) {
            const long left = M - (long)b * R;
            const double n = (double)(left < R ? left : R);
            const double d = (double)v[j][0] - g, s1 = (double)v[j][1], s2 = (double)v[j][2];
            s[0] += s1 + n * d;
            s[1] += s2 + 2. * d * s1 + n * d * d;
          }
        }
      }
    }
    sh_tree16<2>(red, s, grp, lane);
    if (grp == 0 && c < C) {
      const double S1 = red[0][0][lane], S2 = red[0][1][lane], m = (double)M;
      const double mean = g + S1 / m;
      double var = (S2 - S1 * S1 / m) / m;
      var = var > 0. ? var : 0.;
      const double invstd = 1. / sqrt(var + o.eps);
      o.mean[c] = (float)mean;
      o.invstd[c] = (float)invstd;
      if (o.scale) {
        const double sc = (double)o.gamma[c] * invstd;
        o.scale[c] = (float)sc;
        o.shift[c] = (float)((double)o.beta[c] - mean * sc);
      }
      if (o.running_mean) o.running_mean[c] = (float)((1. - o.momentum) * (double)o.running_mean[c] + o.momentum * mean);
      if (o.running_var) o.running_var[c] = (float)((1. - o.momentum) * (double)o.running_var[c] + o.momentum * (var * m / (m - 1.)));
    }
    __syncthreads();
  }
}

// K = 1: out0[c] = the sum (c < Cw).  K = 2 (the BN backward): res[0][C] = gamma * invstd, res[1][C] = s1 / M, res[2][C] = s2 / M for the apply
// launch, d_beta = s1 and d_gamma = s2 where non-NULL.
template <int K>
__global__ __launch_bounds__(1024) void sh_sums_finish_kernel(const float* __restrict__ part, int chunks, long M, int C, int Cw,
                                                              const float* __restrict__ gamma, const float* __restrict__ invstd,
                                                              float* __restrict__ res, float* __restrict__ out0, float* __restrict__ out1) {
  __shared__ double red[16][K][64];
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  for (int cb = blockIdx.x * 64; cb < C; cb += gridDim.x * 64) {       // (launched with one workgroup per 64 columns: one pass)
    const int c = cb + lane;
    double s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0.;
    if (c < C)
      for (int b0 = grp; b0 < chunks; b0 += 16 * SH_BATCH) {
        float v[SH_BATCH][K];
#pragma unroll
        for (int j = 0; j < SH_BATCH; ++j) {
          const int b = b0 + 16 * j;
#pragma unroll
          for (int k = 0; k < K; ++k) v[j][k] = part[((size_t)(b < chunks ? b : b0) * K + k) * C + c];
        }
#pragma unroll
        for (int j = 0; j < SH_BATCH; ++j) {
          if (b0 + 16 * j < chunks) {
#pragma unroll
            for (int k = 0; k < K; ++k) s[k] += (double)v[j][k];
          }
        }
      }
    sh_tree16<K>(red, s, grp, lane);
    if (grp == 0 && c < Cw) {
      if (K == 1) {
        out0[c] = (float)red[0][0][lane];
      } else {
        const double S1 = red[0][0][lane], S2 = red[0][K - 1][lane];
        res[c] = gamma[c] * invstd[c];
        res[C + c] = (float)(S1 / (double)M);
        res[2 * (size_t)C + c] = (float)(S2 / (double)M);
        if (out0) out0[c] = (float)S1;
        if (out1) out1[c] = (float)S2;
      }
    }
    __syncthreads();
  }
}

// the 32-bit mix of synth.hash_uniform: two xorshift-multiply rounds and a final xorshift
__device__ __forceinline__ unsigned sh_mix32(unsigned h) {
  h ^= h >> 16; h *= 0x45D9F3Bu;
  h ^= h >> 16; h *= 0x45D9F3Bu;
  h ^= h >> 16;
  return h;
}

// r = fmaf(z, a, b) on its way to bf16: where r sits exactly on a bf16 tie although the exact z a + b does not, step one f32 ulp towards the exact
// value, so that the bf16 rounding that follows is the single rounding of z a + b.  The sign of the residual: z a is exact in double, its sum
// with b is split into the double s and the exact residual e (two-sum); s - r is exact (s and r agree to 24 bits), and |e| is below any
// non-zero s - r.  Runs on the tie pattern only.
__device__ __forceinline__ float sh_off_the_false_tie(float r, float z, float a, float b) {
  unsigned u = __float_as_uint(r);
  if ((u & 0xFFFFu) == 0x8000u) {
    const double p = (double)z * (double)a, bd = (double)b;
    const double s = p + bd, bb = s - p;
    const double e = (p - (s - bb)) + (bd - bb);
    const double t = s - (double)r;
    const double d = t != 0. ? t : e;
    if (d != 0.) u = ((d > 0.) == (r > 0.f)) ? u + 1u : u - 1u;
  }
  return __uint_as_float(u);
}

// streaming, as elu_backward_rows: 8 columns per thread and step, grid-stride over the M * C / 8 chunks
template <int ZDT, int YDT>
__global__ __launch_bounds__(256) void sh_bn_relu_drop_kernel(const void* z, int ld_z, const float* __restrict__ scale, const float* __restrict__ shift,
                                                              void* y, int ld_y, unsigned chunks, unsigned cpr, int drop, float p, float keep_scale,
                                                              unsigned key) {
  const unsigned step = gridDim.x * 256u;
  for (unsigned long i = blockIdx.x * 256u + threadIdx.x; i < chunks; i += step) {
    const unsigned m = (unsigned)i / cpr, c = ((unsigned)i - m * cpr) * 8u;
    float v[8], a[8], b[8], o[8];
    load8<ZDT>(z, (size_t)m * ld_z + c, v);
    load8<WSEG_F32>(scale, c, a);
    load8<WSEG_F32>(shift, c, b);
    const unsigned i0 = m * (cpr * 8u) + c;                          // row * C + col < 2^32 (checked by the launch function)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float r = __builtin_fmaf(v[e], a[e], b[e]);
      if (YDT == WSEG_BF16) r = sh_off_the_false_tie(r, v[e], a[e], b[e]);      // (a keep factor that is a power of two, p = 0.5, keeps the tie pattern)
      r = fmaxf(r, 0.f);
      if (drop) {
        const unsigned u = sh_mix32(sh_mix32(i0 + e) + key) >> 8;
        r = (float)u * 0x1p-24f >= p ? r * keep_scale : 0.f;
      }
      o[e] = r;
    }
    store8<YDT>(y, (size_t)m * ld_y + c, o);
  }
}

template <int GDT, int DT>
__global__ __launch_bounds__(256) void sh_bn_bwd_apply_kernel(const void* g, int ld_g, const void* y, int ld_y, const void* z, int ld_z,
                                                              const float* __restrict__ mean, const float* __restrict__ invstd,
                                                              const float* __restrict__ res, int C, float s, void* dz, int ld_dz, unsigned chunks,
                                                              unsigned cpr) {
  const unsigned step = gridDim.x * 256u;
  for (unsigned long i = blockIdx.x * 256u + threadIdx.x; i < chunks; i += step) {
    const unsigned m = (unsigned)i / cpr, c = ((unsigned)i - m * cpr) * 8u;
    float a[8], b[8], v[8], mu[8], is[8], k[8], m1[8], m2[8], o[8];
    load8<GDT>(g, (size_t)m * ld_g + c, a);                          // (read before the store below: dz may be g)
    load8<DT>(y, (size_t)m * ld_y + c, b);
    load8<DT>(z, (size_t)m * ld_z + c, v);
    load8<WSEG_F32>(mean, c, mu);
    load8<WSEG_F32>(invstd, c, is);
    load8<WSEG_F32>(res, c, k);
    load8<WSEG_F32>(res, (size_t)C + c, m1);
    load8<WSEG_F32>(res, 2 * (size_t)C + c, m2);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float dy = b[e] > 0.f ? s * a[e] : 0.f;
      const float xhat = (v[e] - mu[e]) * is[e];
      o[e] = k[e] * ((dy - m1[e]) - xhat * m2[e]);
    }
    store8<DT>(dz, (size_t)m * ld_dz + c, o);
  }
}

bool sh_dtype(int dt) { return dt == WSEG_F32 || dt == WSEG_BF16; }
bool sh_al16(const void* p) { return p && ((uintptr_t)p & 15) == 0; }

int sh_check_rows(const char* what, const char* name, const void* p, int ld, int dtype, long M, int C) {
  WSEG_CHECK(sh_dtype(dtype), "%s: %s dtype %d (f32 = 0 or bf16 = 1)", what, name, dtype);
  WSEG_CHECK(sh_al16(p), "%s: %s null or not 16-byte aligned", what, name);
  WSEG_CHECK(ld % 8 == 0 && ld >= C, "%s: ld of %s = %d must be a multiple of 8 and >= C = %d", what, name, ld, C);
  WSEG_CHECK(M * (long)ld < (1L << 40), "%s: %s too large (M=%ld ld=%d)", what, name, M, ld);
  return 0;
}

int sh_check_dims(const char* what, long M, int C, long min_rows) {
  WSEG_CHECK(C > 0 && C % 8 == 0, "%s: C=%d must be a positive multiple of 8", what, C);
  WSEG_CHECK(M >= min_rows && M < (1L << 31), "%s: M=%ld outside [%ld, 2^31)", what, M, min_rows);
  return 0;
}

unsigned sh_stream_blocks(long chunks) { return (unsigned)std::min((chunks + 255) / 256, 256L * 8); }

}  // namespace

extern "C" long wseg_bn_stats_workspace_bytes(long M, int C) {
  if (M < 1 || M >= (1L << 31) || C <= 0 || C % 8) {
    wseg_set_error("bn_stats_workspace_bytes: M=%ld C=%d (1 <= M < 2^31, C a positive multiple of 8)", M, C);
    return -1;
  }
  return ((long)sh_chunks(M) * 3 + 3) * C * (long)sizeof(float);
}

extern "C" int wseg_bn_stats(const void* x, int ld, int dtype, long M, int C, const float* gamma, const float* beta, double eps, double momentum,
                             float* mean, float* invstd, float* scale, float* shift, float* running_mean, float* running_var, void* workspace,
                             void* stream) {
  if (int rc = sh_check_dims("bn_stats", M, C, 1)) return rc;
  WSEG_CHECK(M >= 2, "bn_stats: M=%ld: batch statistics need more than one value per channel", M);
  if (int rc = sh_check_rows("bn_stats", "x", x, ld, dtype, M, C)) return rc;
  WSEG_CHECK(mean && invstd && sh_al16(workspace), "bn_stats: mean / invstd null, or workspace null or not 16-byte aligned");
  WSEG_CHECK((scale != nullptr) == (shift != nullptr) && (!scale || (gamma && beta)), "bn_stats: scale and shift come together and need gamma and beta");
  WSEG_CHECK(eps >= 0. && momentum >= 0. && momentum <= 1., "bn_stats: eps=%g momentum=%g", eps, momentum);
  const int R = sh_rows_per_chunk(M), chunks = sh_chunks(M);
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)workspace;
  const dim3 grid((unsigned)chunks, (unsigned)((C + SH_COLS - 1) / SH_COLS));
  with_const<2>(dtype, [&](auto dt) {
    StatsOp<decltype(dt)::value> op{x, ld};
    hipLaunchKernelGGL((sh_reduce_kernel<StatsOp<decltype(dt)::value>>), grid, dim3(256), 0, s, op, M, C, R, part);
  });
  WSEG_LAUNCH_CHECK();
  const StatsOut o{gamma, beta, mean, invstd, scale, shift, running_mean, running_var, eps, momentum};
  hipLaunchKernelGGL(sh_stats_finish_kernel, dim3((unsigned)((C + 63) / 64)), dim3(1024), 0, s, part, chunks, M, C, R, o);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_bn_relu_drop(const void* z, int ld_z, int z_dtype, const float* scale, const float* shift, void* y, int ld_y, int y_dtype,
                                 long M, int C, float p, unsigned key, void* stream) {
  if (int rc = sh_check_dims("bn_relu_drop", M, C, 1)) return rc;
  if (int rc = sh_check_rows("bn_relu_drop", "z", z, ld_z, z_dtype, M, C)) return rc;
  if (int rc = sh_check_rows("bn_relu_drop", "y", y, ld_y, y_dtype, M, C)) return rc;
  WSEG_CHECK(sh_al16(scale) && sh_al16(shift), "bn_relu_drop: scale / shift null or not 16-byte aligned");
  WSEG_CHECK(p >= 0.f && p < 1.f, "bn_relu_drop: p=%g outside [0, 1)", p);
  WSEG_CHECK(M * (long)C < (1L << 32), "bn_relu_drop: M*C = %ld must stay below 2^32 (the mask's counter is one 32-bit word)", M * (long)C);
  WSEG_CHECK(z != y || (z_dtype == y_dtype && ld_z == ld_y), "bn_relu_drop: y may alias z only with the same dtype and ld");
  const long chunks = M * (long)(C / 8);
  hipStream_t s = (hipStream_t)stream;
  with_const<2>(z_dtype, [&](auto zd) {
    with_const<2>(y_dtype, [&](auto yd) {
      hipLaunchKernelGGL((sh_bn_relu_drop_kernel<decltype(zd)::value, decltype(yd)::value>), dim3(sh_stream_blocks(chunks)), dim3(256), 0, s, z, ld_z,
                         scale, shift, y, ld_y, (unsigned)chunks, (unsigned)(C / 8), p > 0.f ? 1 : 0, p, 1.f / (1.f - p), key);
    });
  });
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_bn_relu_backward(const void* g, int ld_g, int g_dtype, const void* y, int ld_y, const void* z, int ld_z, int dtype,
                                     const float* mean, const float* invstd, const float* gamma, float s, void* dz, int ld_dz, float* d_gamma,
                                     float* d_beta, long M, int C, void* workspace, void* stream) {
  if (int rc = sh_check_dims("bn_relu_backward", M, C, 2)) return rc;
  if (int rc = sh_check_rows("bn_relu_backward", "g", g, ld_g, g_dtype, M, C)) return rc;
  if (int rc = sh_check_rows("bn_relu_backward", "y", y, ld_y, dtype, M, C)) return rc;
  if (int rc = sh_check_rows("bn_relu_backward", "z", z, ld_z, dtype, M, C)) return rc;
  if (int rc = sh_check_rows("bn_relu_backward", "dz", dz, ld_dz, dtype, M, C)) return rc;
  WSEG_CHECK(sh_al16(mean) && sh_al16(invstd) && sh_al16(gamma), "bn_relu_backward: mean / invstd / gamma null or not 16-byte aligned");
  WSEG_CHECK(sh_al16(workspace), "bn_relu_backward: workspace null or not 16-byte aligned");
  WSEG_CHECK(g != dz || (g_dtype == dtype && ld_g == ld_dz), "bn_relu_backward: dz may alias g only with the same dtype and ld");
  WSEG_CHECK(dz != y && dz != z, "bn_relu_backward: dz may not alias y or z");
  const int R = sh_rows_per_chunk(M), chunks = sh_chunks(M);
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)workspace;
  float* res = part + (size_t)chunks * 3 * C;                       // [3][C] behind the partials (which use 2 of their 3 slots here)
  const dim3 grid((unsigned)chunks, (unsigned)((C + SH_COLS - 1) / SH_COLS));
  const long nchunk = M * (long)(C / 8);
  WSEG_CHECK(nchunk < (1L << 31), "bn_relu_backward: too many elements (M=%ld C=%d)", M, C);
  with_const<2>(g_dtype, [&](auto gd) {
    with_const<2>(dtype, [&](auto dt) {
      typedef BwdOp<decltype(gd)::value, decltype(dt)::value> Op;
      Op op{g, y, z, ld_g, ld_y, ld_z, mean, invstd, s};
      hipLaunchKernelGGL((sh_reduce_kernel<Op>), grid, dim3(256), 0, st, op, M, C, R, part);
    });
  });
  WSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL((sh_sums_finish_kernel<2>), dim3((unsigned)((C + 63) / 64)), dim3(1024), 0, st, part, chunks, M, C, C, gamma, invstd, res, d_beta, d_gamma);
  WSEG_LAUNCH_CHECK();
  with_const<2>(g_dtype, [&](auto gd) {
    with_const<2>(dtype, [&](auto dt) {
      hipLaunchKernelGGL((sh_bn_bwd_apply_kernel<decltype(gd)::value, decltype(dt)::value>), dim3(sh_stream_blocks(nchunk)), dim3(256), 0, st, g, ld_g,
                         y, ld_y, z, ld_z, mean, invstd, res, C, s, dz, ld_dz, (unsigned)nchunk, (unsigned)(C / 8));
    });
  });
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_col_sums(const void* rows, int ld, int dtype, long M, int C, float* out, void* workspace, void* stream) {
  WSEG_CHECK(C > 0, "col_sums: C=%d", C);
  const int C8 = (C + 7) / 8 * 8;                                   // whole 8-column chunks are read; only the first C sums are written
  if (int rc = sh_check_dims("col_sums", M, C8, 1)) return rc;
  if (int rc = sh_check_rows("col_sums", "rows", rows, ld, dtype, M, C8)) return rc;
  WSEG_CHECK(out && sh_al16(workspace), "col_sums: out null, or workspace null or not 16-byte aligned");
  const int R = sh_rows_per_chunk(M), chunks = sh_chunks(M);
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)workspace;
  const dim3 grid((unsigned)chunks, (unsigned)((C8 + SH_COLS - 1) / SH_COLS));
  with_const<2>(dtype, [&](auto dt) {
    SumOp<decltype(dt)::value> op{rows, ld};
    hipLaunchKernelGGL((sh_reduce_kernel<SumOp<decltype(dt)::value>>), grid, dim3(256), 0, s, op, M, C8, R, part);
  });
  WSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL((sh_sums_finish_kernel<1>), dim3((unsigned)((C8 + 63) / 64)), dim3(1024), 0, s, part, chunks, M, C8, C, (const float*)nullptr, (const float*)nullptr,
                     (float*)nullptr, out, (float*)nullptr);
  WSEG_LAUNCH_CHECK();
  return 0;
}
