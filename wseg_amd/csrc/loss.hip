// loss.hip — the SEAM losses of contrast_train.py:138-243 as HIP kernels (forward values and hand-written gradients): classification, the radix
// select behind the min-pool / ECR top-k sums, ER + ECR, the f_proj row resize and the head gradient, pseudo labels and batch prototypes.  The
// map statistics are in maps.hip, the pixel-to-prototype contrast in nce.hip.  All 21-class maps are planar f32.
// The kernels are HBM/latency-bound integer+float work: coalesced planar access, wavefront
// shuffles for per-pixel 21-wide reductions / ranks, LDS for per-plane and per-class reductions.
#include <algorithm>
#include "loss_helpers.h"

namespace {

// ---- classification loss (contrast_train.py:142,155,159-160): z = GAP, mean BCE-with-logits over N*20
//      out[0] += loss ; dz[n][c] = coef * (sigmoid(z) - y) / (20 N)   (c >= 1; dz[n][0] = 0), as a per-pixel bias /npix
__global__ void cls_loss_kernel(const float* __restrict__ stats, const float* __restrict__ label20, float* __restrict__ loss_out,
                                float* __restrict__ plane_bias, int N, int npix, float coef) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < N * 21; i += blockDim.x) {
    const int n = i / 21, c = i - n * 21;
    float bias = 0.f;
    if (c >= 1) {
      const float z = stats[(size_t)i * 6 + 2] / npix;
      const float y = label20[n * 20 + c - 1];
      // -(y*logsigmoid(z) + (1-y)*logsigmoid(-z)); logsigmoid(z) = min(z,0) - log1p(exp(-|z|))
      const float l1p = log1pf(expf(-fabsf(z)));
      const float ls_p = fminf(z, 0.f) - l1p, ls_n = fminf(-z, 0.f) - l1p;
      acc += -(y * ls_p + (1.f - y) * ls_n);
      const float sg = 1.f / (1.f + expf(-z));
      bias = coef * (sg - y) / (20.f * N) / npix;           // d loss / d U[n,c,pixel]
    }
    plane_bias[i] = bias;
  }
  const float tot = block_sum(acc, red);
  if (threadIdx.x == 0) atomicAdd(loss_out, tot / (20.f * N));
}

// ---- radix select of the k-th order statistic per row (values as order-preserving uint keys: f2key)
// state[row] = {prefix, mask, k_remaining}; one pass handles 8 bits (shift = 24,16,8,0)
__global__ __launch_bounds__(256) void select_hist_kernel(const float* __restrict__ vals, int n, int use_abs, const unsigned* __restrict__ state,
                                                          unsigned* __restrict__ hist, int shift) {
  __shared__ unsigned h[4][256];                            // one sub-histogram per wave: values cluster, LDS atomics on one
  const int row = blockIdx.y, wv = threadIdx.x >> 6;        // bucket serialise
#pragma unroll
  for (int w = 0; w < 4; ++w) h[w][threadIdx.x] = 0;
  __syncthreads();
  const unsigned prefix = state[row * 4 + 0], mask = state[row * 4 + 1];
  const float* v = vals + (size_t)row * n;
  auto count = [&](float f) {
    if (use_abs) f = fabsf(f);
    const unsigned k = f2key(f);
    if ((k & mask) == prefix) atomicAdd(&h[wv][(k >> shift) & 255u], 1u);
  };
  if ((n & 3) == 0) {                                       // 16-B loads (the rows of both callers: 448^2 and 21 * 128^2 values)
    const float4* v4 = reinterpret_cast<const float4*>(v);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < (n >> 2); i += gridDim.x * 256) {
      const float4 q = v4[i];
      count(q.x); count(q.y); count(q.z); count(q.w);
    }
  } else {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) count(v[i]);
  }
  __syncthreads();
  const unsigned t = h[0][threadIdx.x] + h[1][threadIdx.x] + h[2][threadIdx.x] + h[3][threadIdx.x];
  if (t) atomicAdd(&hist[row * 256 + threadIdx.x], t);
}
// choose the bucket holding the k-th (k counted from the small end: 1-based rank) and narrow the prefix.
// One wave per row: lane l owns buckets 4l..4l+3, a shuffle scan finds the lane whose running count crosses k.
__global__ __launch_bounds__(64) void select_scan_kernel(unsigned* __restrict__ state, unsigned* __restrict__ hist, int shift, int rows) {
  const int row = blockIdx.x, lane = threadIdx.x;
  if (row >= rows) return;
  const unsigned k = state[row * 4 + 2];
  uint4* hrow = reinterpret_cast<uint4*>(hist + (size_t)row * 256);
  const uint4 c = hrow[lane];
  const unsigned s = c.x + c.y + c.z + c.w;
  unsigned inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  const unsigned exc = inc - s;
  const unsigned total = __shfl(inc, 63, 64);
  hrow[lane] = make_uint4(0u, 0u, 0u, 0u);
  int b = -1; unsigned cum = exc;
  if (exc < k && inc >= k) {                       // exactly one lane (k >= 1); first bucket with running count >= k
    const unsigned cs[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (b < 0) { if (cum + cs[j] >= k) b = lane * 4 + j; else cum += cs[j]; }
    }
  } else if (lane == 63 && total < k) {            // (cannot happen for finite inputs: keep the serial loop's result)
    b = 255; cum = total;
  }
  if (b >= 0) {
    state[row * 4 + 0] |= ((unsigned)b << shift);
    state[row * 4 + 1] |= (255u << shift);
    state[row * 4 + 2] = k - cum;
  }
}
__global__ void select_init_kernel(unsigned* __restrict__ state, unsigned* __restrict__ hist, int rows, unsigned rank_small, float* __restrict__ res) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows) { state[i * 4 + 0] = 0; state[i * 4 + 1] = 0; state[i * 4 + 2] = rank_small; state[i * 4 + 3] = 0; }
  if (i < rows * 4) res[i] = 0.f;                  // (the sums the last pass accumulates into: cleared here, not by a memset launch in front of it)
  if (i < rows * 256) hist[i] = 0;
}
// after 4 passes state.prefix is the key of the threshold.  Accumulate per row:
//   res[row] = {thr, sum of relu?(v) strictly beyond thr, count strictly beyond, count equal}
__global__ __launch_bounds__(256) void select_sum_kernel(const float* __restrict__ vals, int n, int use_abs, int largest, int relu_vals,
                                                         const unsigned* __restrict__ state, float* __restrict__ res) {
  __shared__ float red[4];
  const int row = blockIdx.y;
  const float thr = key2f(state[row * 4 + 0]);
  const float* v = vals + (size_t)row * n;
  float s = 0.f, cs = 0.f, ce = 0.f;
  auto take = [&](float f) {
    if (use_abs) f = fabsf(f);
    const bool beyond = largest ? (f > thr) : (f < thr);
    if (beyond) { s += relu_vals ? fmaxf(f, 0.f) : f; cs += 1.f; }
    else if (f == thr) ce += 1.f;
  };
  if ((n & 3) == 0) {
    const float4* v4 = reinterpret_cast<const float4*>(v);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < (n >> 2); i += gridDim.x * 256) {
      const float4 q = v4[i];
      take(q.x); take(q.y); take(q.z); take(q.w);
    }
  } else {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) take(v[i]);
  }
  const float S = block_sum(s, red), CS = block_sum(cs, red), CE = block_sum(ce, red);
  if (threadIdx.x == 0) {
    if (blockIdx.x == 0) res[row * 4 + 0] = thr;
    atomicAdd(&res[row * 4 + 1], S); atomicAdd(&res[row * 4 + 2], CS); atomicAdd(&res[row * 4 + 3], CE);
  }
}
// loss += scale * sum_rows ( sum_strict + (k - cnt_strict) * f(thr) )
__global__ void select_finish_kernel(const float* __restrict__ res, int rows, int k, int relu_vals, float scale, float* __restrict__ loss_out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    float t = 0.f;
    for (int r = 0; r < rows; ++r) {
      const float thr = relu_vals ? fmaxf(res[r * 4 + 0], 0.f) : res[r * 4 + 0];
      t += res[r * 4 + 1] + ((float)k - res[r * 4 + 2]) * thr;
    }
    atomicAdd(loss_out, t * scale);
  }
}

// ---- ER + ECR preparation on the 128x128 maps (contrast_train.py:163-169)
// per pixel: ER sum, G_c1/G_c2 (ER gradients, fg only), dlt1 = r1 - oh(c2), dlt2 = r2 - oh(c1) (all 21 channels)
__global__ void er_ecr_prep_kernel(const float* __restrict__ c1, const float* __restrict__ c2, const float* __restrict__ r1,
                                   const float* __restrict__ r2, float* __restrict__ Gc1, float* __restrict__ Gc2,
                                   float* __restrict__ dlt1, float* __restrict__ dlt2, float* __restrict__ er_out,
                                   int npix, float er_coef, long total) {
  __shared__ float red[4];
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  float er = 0.f;
  if (idx < total) {
    const long n = idx / npix; const int p = (int)(idx - n * npix);
    const size_t base = (size_t)n * 21 * npix + p;
    float a[21], b[21];
    float m1 = -INFINITY, m2 = -INFINITY;
    for (int c = 1; c < 21; ++c) {
      a[c] = c1[base + (size_t)c * npix]; b[c] = c2[base + (size_t)c * npix];
      m1 = fmaxf(m1, a[c]); m2 = fmaxf(m2, b[c]);
      const float df = a[c] - b[c];
      er += fabsf(df);
      const float sg = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);
      Gc1[base + (size_t)c * npix] = sg * er_coef;
      Gc2[base + (size_t)c * npix] = -sg * er_coef;
    }
    Gc1[base] = 0.f; Gc2[base] = 0.f;
    a[0] = 1.f - m1; b[0] = 1.f - m2;                    // cam[:,0] = 1 - max fg
    for (int c = 0; c < 21; ++c) {
      const float oh2 = (c == 0 || b[c] == m2) ? b[c] : 0.f;
      const float oh1 = (c == 0 || a[c] == m1) ? a[c] : 0.f;
      dlt1[base + (size_t)c * npix] = r1[base + (size_t)c * npix] - oh2;
      dlt2[base + (size_t)c * npix] = r2[base + (size_t)c * npix] - oh1;
    }
  }
  const float t = block_sum(er, red);
  if (threadIdx.x == 0 && t != 0.f) atomicAdd(er_out, t);
}

// ECR backward: G_r = coef * sign(dlt) for the K largest |dlt| of each sample (ties at thr share the remainder)
__global__ void ecr_bwd_kernel(const float* __restrict__ dlt, const float* __restrict__ res, float* __restrict__ Gr, int per_row, int k, float coef, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const long row = idx / per_row;
  const float d = dlt[idx], v = fabsf(d), thr = res[row * 4 + 0];
  float w = 0.f;
  if (v > thr) w = 1.f;
  else if (v == thr) { const float ce = res[row * 4 + 3]; w = ce > 0.f ? ((float)k - res[row * 4 + 2]) / ce : 0.f; }
  const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  Gr[idx] = w * sg * coef;
}

// ---- f_proj rows (head rows cols [0,128), any dtype) -> F [N*oh*ow][128] f32, bilinear align_corners=True
template <int DT>
__global__ void rows_resize_fwd_kernel(const void* __restrict__ head, int ld, float* __restrict__ F, int ih, int iw, int oh, int ow, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;      // over N*oh*ow*128
  if (idx >= total) return;
  const int ch = (int)(idx & 127); const long pix = idx >> 7;
  const int ox = (int)(pix % ow); const long r = pix / ow;
  const int oy = (int)(r % oh); const long n = r / oh;
  int y0, y1, x0, x1; float fy, fx;
  src_index(oy, ac_scale(ih, oh), ih, y0, y1, fy); src_index(ox, ac_scale(iw, ow), iw, x0, x1, fx);
  auto f = [&](int y, int x) { return elem<DT>::ld(head, (((size_t)n * ih + y) * iw + x) * ld + ch); };
  F[idx] = (1.f - fy) * ((1.f - fx) * f(y0, x0) + fx * f(y0, x1)) + fy * ((1.f - fx) * f(y1, x0) + fx * f(y1, x1));
}

// ---- d(head rows): cols [0,128) = relu-masked adjoint of the row resize applied to dF, cols [128,149) = d_cam_low, rest 0
template <int DT>
__global__ void head_grad_fused_kernel(const float* __restrict__ dF, const float* __restrict__ d_cam, const void* __restrict__ head,
                                       void* __restrict__ d_head, int ld, int ih, int iw, int oh, int ow, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;      // over N*ih*iw*(ld/8)
  if (idx >= total) return;
  const int v8 = ld / 8;
  const long pix = idx / v8; const int c8 = (int)(idx - pix * v8) * 8;
  const int x = (int)(pix % iw); const long r = pix / iw;
  const int y = (int)(r % ih); const long n = r / ih;
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;
  if (c8 < 128) {
    const float sy = ac_scale(ih, oh), sx = ac_scale(iw, ow);
    int oy_lo, oy_hi, ox_lo, ox_hi;
    if (sy > 0.f) { oy_lo = max(0, (int)floorf((y - 1) / sy) - 1); oy_hi = min(oh - 1, (int)ceilf((y + 1) / sy) + 1); } else { oy_lo = 0; oy_hi = oh - 1; }
    if (sx > 0.f) { ox_lo = max(0, (int)floorf((x - 1) / sx) - 1); ox_hi = min(ow - 1, (int)ceilf((x + 1) / sx) + 1); } else { ox_lo = 0; ox_hi = ow - 1; }
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
      int y0, y1; float fy;
      src_index(oy, sy, ih, y0, y1, fy);
      const float wy = (y == y0 ? 1.f - fy : 0.f) + (y == y1 ? fy : 0.f);
      if (wy == 0.f) continue;
      for (int ox = ox_lo; ox <= ox_hi; ++ox) {
        int x0, x1; float fx;
        src_index(ox, sx, iw, x0, x1, fx);
        const float w = wy * ((x == x0 ? 1.f - fx : 0.f) + (x == x1 ? fx : 0.f));
        if (w == 0.f) continue;
        const float4* g = reinterpret_cast<const float4*>(dF + ((((size_t)n * oh + oy) * ow + ox) << 7) + c8);
        const float4 g0 = g[0], g1 = g[1];
        o[0] += w * g0.x; o[1] += w * g0.y; o[2] += w * g0.z; o[3] += w * g0.w;
        o[4] += w * g1.x; o[5] += w * g1.y; o[6] += w * g1.z; o[7] += w * g1.w;
      }
    }
    float hv[8];
    load8<DT>(head, (size_t)pix * ld + c8, hv);
#pragma unroll
    for (int e = 0; e < 8; ++e) if (!(hv[e] > 0.f)) o[e] = 0.f;
  } else if (c8 < 152 && d_cam) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = c8 + e - 128;
      if (c < 21) o[e] = d_cam[(((size_t)n * 21 + c) * ih + y) * iw + x];
    }
  }
  store8<DT>(d_head, (size_t)pix * ld + c8, o);
}

// ---- pseudo labels (contrast_train.py:186-197): one workgroup per image over npix (=256) pixels
__global__ __launch_bounds__(256) void pseudo_label_kernel(const float* __restrict__ R, const float* __restrict__ label20, float bg_thr,
                                                           int* __restrict__ y, float* __restrict__ ncam, int npix) {
  __shared__ float s_mx[21], s_mn[21];
  __shared__ float red_a[256], red_b[256];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* Rn = R + (size_t)n * 21 * npix;
  for (int c = 0; c < 21; ++c) {
    float mx = 0.f, mn = INFINITY;
    for (int p = tid; p < npix; p += 256) { const float v = fmaxf(Rn[(size_t)c * npix + p], 0.f); mx = fmaxf(mx, v); mn = fminf(mn, v); }
    red_a[tid] = mx; red_b[tid] = mn;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) { red_a[tid] = fmaxf(red_a[tid], red_a[tid + o]); red_b[tid] = fminf(red_b[tid], red_b[tid + o]); } __syncthreads(); }
    if (tid == 0) { s_mx[c] = red_a[0]; s_mn[c] = red_b[0]; }
    __syncthreads();
  }
  for (int p = tid; p < npix; p += 256) {
    float best = -INFINITY; int bc = 0;
    for (int c = 0; c < 21; ++c) {
      float v = fmaxf(Rn[(size_t)c * npix + p], 0.f);
      if (v < s_mn[c] + 1e-5f) v = 0.f;
      v = (v - s_mn[c] - 1e-5f) / (s_mx[c] - s_mn[c] + 1e-5f);
      if (c == 0) v = bg_thr;
      ncam[((size_t)n * 21 + c) * npix + p] = v;
      const float L = c == 0 ? 1.f : label20[n * 20 + c - 1];
      const float s = v * L;                               // softmax is monotone: argmax of the logits
      if (s > best) { best = s; bc = c; }
    }
    y[(size_t)n * npix + p] = bc;
  }
}

// ---- batch prototypes (contrast_train.py:199-209): one workgroup per class; candidates = top-K of T[c][:]
//      T[c][p] = ncam[n][c][pix], p = n*npix + pix.  Constant rows use the supplied tie index set (Q5).
__global__ __launch_bounds__(256) void proto_candidates_kernel(const float* __restrict__ ncam, const float* __restrict__ F, const int* __restrict__ tie_idx,
                                                               float* __restrict__ cand_val, float* __restrict__ cand_feat, int* __restrict__ cand_const,
                                                               int N, int npix, int K) {
  extern __shared__ float sv[];                            // [P] values
  __shared__ float r_v[256]; __shared__ int r_i[256];
  __shared__ int sel[64];
  __shared__ float s_gmin;
  const int c = blockIdx.x, tid = threadIdx.x;
  const int P = N * npix;
  float lmx = -INFINITY, lmn = INFINITY;
  for (int p = tid; p < P; p += 256) {
    const int n = p / npix, pix = p - n * npix;
    float v = ncam[((size_t)n * 21 + c) * npix + pix];
    if (v != v) v = -INFINITY;                             // NaN ranks as -inf (a diverged step: the class prototype turns NaN below)
    sv[p] = v; lmx = fmaxf(lmx, v); lmn = fminf(lmn, v);
  }
  r_v[tid] = lmx; __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (tid < o) r_v[tid] = fmaxf(r_v[tid], r_v[tid + o]); __syncthreads(); }
  const float gmx = r_v[0]; __syncthreads();
  r_v[tid] = lmn; __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (tid < o) r_v[tid] = fminf(r_v[tid], r_v[tid + o]); __syncthreads(); }
  if (tid == 0) s_gmin = r_v[0];
  __syncthreads();
  const bool is_const = (gmx == s_gmin);
  if (is_const) {
    if (tid < K) sel[tid] = min(max(tie_idx[tid], 0), P - 1);
    __syncthreads();
  } else {
    // K rounds of (max value, lowest index): wave shuffles + one LDS hop.  A taken value becomes NaN, which no compare
    // selects again; every value left is >= -inf, so while K <= P each round finds an index (bi < P).
    for (int k = 0; k < K; ++k) {
      float bv = -INFINITY; int bi = 0x7fffffff;
      for (int p = tid; p < P; p += 256) { const float v = sv[p]; if (v > bv || (v == bv && p < bi)) { bv = v; bi = p; } }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
      }
      if ((tid & 63) == 0) { r_v[tid >> 6] = bv; r_i[tid >> 6] = bi; }
      __syncthreads();
      if (tid == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) if (r_v[w] > bv || (r_v[w] == bv && r_i[w] < bi)) { bv = r_v[w]; bi = r_i[w]; }
        if (bi >= P) bi = 0;                               // (unreachable: no sentinel reaches an address)
        sel[k] = bi; sv[bi] = NAN;
      }
      __syncthreads();
    }
  }
  if (tid == 0) cand_const[c] = is_const ? 1 : 0;
  for (int k = 0; k < K; ++k) {
    const int p = sel[k];
    const int n = p / npix, pix = p - n * npix;
    if (tid == 0) cand_val[c * K + k] = ncam[((size_t)n * 21 + c) * npix + pix];
    if (tid < 128) cand_feat[((size_t)c * K + k) * 128 + tid] = F[(size_t)p * 128 + tid];
  }
}
// merge world*K candidates per class -> top K -> weighted mean -> L2 normalise (F.normalize eps 1e-12)
__global__ __launch_bounds__(128) void proto_merge_kernel(const float* __restrict__ cand_val, const float* __restrict__ cand_feat, const int* __restrict__ cand_const,
                                                          float* __restrict__ protos, int world, int K, long rs_val, long rs_feat, long rs_const) {
  __shared__ float vals[512]; __shared__ int order[64]; __shared__ float red[2]; __shared__ int cst_s;
  const int c = blockIdx.x, tid = threadIdx.x;
  const int M = world * K;                                  // rank w's [21][K] values / [21][K][128] features / [21] flags at w * rs_*
  for (int i = tid; i < M; i += 128) {
    const int w = i / K, k = i - w * K;
    const float v = cand_val[(size_t)w * rs_val + c * K + k];
    vals[i] = v != v ? -INFINITY : v;                       // NaN ranks as -inf: the compares below then order every pair
  }
  if (tid < K) order[tid] = tid;                            // (every slot holds a valid index even before the ranking)
  if (tid == 0) {
    bool cst = true;
    for (int w = 0; w < world; ++w) cst = cst && cand_const[(size_t)w * rs_const + c];
    cst_s = cst ? 1 : 0;
  }
  __syncthreads();
  if (!cst_s) {                                             // (fully tied: rank 0's set, global pixels first: order[] as initialised)
    // rank by counting (round 2 selected serially on one thread: K x M compares, 40 us at world 8): candidate i is the
    // (#{j : v_j > v_i or (v_j == v_i and j < i)})-th largest — the order of K rounds of "first maximum"
    for (int i = tid; i < M; i += 128) {
      const float v = vals[i];
      int r = 0;
      for (int j = 0; j < M; ++j) { const float u = vals[j]; r += (u > v || (u == v && j < i)) ? 1 : 0; }
      if (r < K) order[r] = i;
    }
  }
  __syncthreads();
  float acc = 0.f, wsum = 0.f;
  for (int k = 0; k < K; ++k) {
    const int i = order[k]; const int w = i / K, kk = i - w * K;
    const float v = cand_val[(size_t)w * rs_val + c * K + kk];
    acc += v * cand_feat[(size_t)w * rs_feat + ((size_t)c * K + kk) * 128 + tid];
    wsum += v;
  }
  const float pr = acc / wsum;
  const float ss = block_sum(pr * pr, red);
  protos[c * 128 + tid] = pr / fmaxf(sqrtf(ss), 1e-12f);
}

}  // namespace

#define GRID1(total) dim3((unsigned)(((total) + 255) / 256)), dim3(256)
#define ST ((hipStream_t)stream)

extern "C" int wseg_cls_loss(const float* stats, const float* label20, float* loss_out, float* plane_bias, int N, int npix, float coef, void* stream) {
  WSEG_CHECK(stats && label20 && loss_out && plane_bias && N > 0, "cls_loss: bad arguments");
  hipLaunchKernelGGL(cls_loss_kernel, dim3(1), dim3(256), 0, ST, stats, label20, loss_out, plane_bias, N, npix, coef);
  WSEG_LAUNCH_CHECK();
  return 0;
}

// k-th order statistic per row + partial sums.  largest=1: the k largest; res[row] = {thr, sum_strict, cnt_strict, cnt_tie}
// workspace: unsigned state[rows*4] + unsigned hist[rows*256]  (wseg_select_workspace_bytes)
extern "C" size_t wseg_select_workspace_bytes(int rows) { return (size_t)rows * (4 + 256) * sizeof(unsigned); }
extern "C" int wseg_select_kth(const float* vals, int rows, int n, int k, int largest, int use_abs, int relu_vals,
                               float* res, void* workspace, void* stream) {
  WSEG_CHECK(vals && res && workspace && rows > 0 && n > 0 && k >= 1 && k <= n, "select_kth: bad arguments (rows=%d n=%d k=%d)", rows, n, k);
  unsigned* state = (unsigned*)workspace;
  unsigned* hist = state + (size_t)rows * 4;
  const unsigned rank_small = largest ? (unsigned)(n - k + 1) : (unsigned)k;
  hipLaunchKernelGGL(select_init_kernel, dim3((rows * 256 + 255) / 256), dim3(256), 0, ST, state, hist, rows, rank_small, res);
  const int gx = std::max(1, std::min(128, (n + 4095) / 4096));  // histogram passes: enough workgroups to stream the rows (4 floats per thread and trip;
                                                                 // 32 / 64 / 128 per row measured equal, 16: +10 %, 8: +40 %)
  const int gs = std::max(1, std::min(32, (n + 8191) / 8192));   // final sums: few workgroups per row (their partials meet in same-address atomics)
  for (int shift = 24; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(select_hist_kernel, dim3(gx, rows), dim3(256), 0, ST, vals, n, use_abs, state, hist, shift);
    hipLaunchKernelGGL(select_scan_kernel, dim3(rows), dim3(64), 0, ST, state, hist, shift, rows);
  }
  hipLaunchKernelGGL(select_sum_kernel, dim3(gs, rows), dim3(256), 0, ST, vals, n, use_abs, largest, relu_vals, state, res);
  WSEG_LAUNCH_CHECK();
  return 0;
}
extern "C" int wseg_select_finish(const float* res, int rows, int k, int relu_vals, float scale, float* loss_out, void* stream) {
  WSEG_CHECK(res && loss_out && rows > 0, "select_finish: bad arguments");
  hipLaunchKernelGGL(select_finish_kernel, dim3(1), dim3(64), 0, ST, res, rows, k, relu_vals, scale, loss_out);
  WSEG_LAUNCH_CHECK();
  return 0;
}

// the 8 logged scalars of contrast_train.py:174, 389-395, 401-408 from the step's accumulators (one launch instead of a handful of torch scalar ops):
// acc = [cls1+cls2, (rvmin1+rvmin2)/2, er_sum, ecr, cross, cross2, intra, -]; out = [loss, cls, er, ecr, nce, intra, cross, cross2]
static __global__ void loss_finish_kernel(const float* __restrict__ acc, float er_coef, float* __restrict__ out) {
  if (threadIdx.x != 0) return;
  const float cls = acc[0] * 0.5f + acc[1], er = acc[2] * er_coef, ecr = acc[3], nce = acc[4] + acc[5] + acc[6];
  out[0] = cls + er + ecr + nce; out[1] = cls; out[2] = er; out[3] = ecr; out[4] = nce; out[5] = acc[6]; out[6] = acc[4]; out[7] = acc[5];
}
extern "C" int wseg_loss_finish(const float* acc, float er_coef, float* out8, void* stream) {
  WSEG_CHECK(acc && out8, "loss_finish: bad arguments");
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(64), 0, ST, acc, er_coef, out8);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_er_ecr_prep(const float* c1, const float* c2, const float* r1, const float* r2, float* Gc1, float* Gc2,
                                float* dlt1, float* dlt2, float* er_sum, int N, int npix, float er_coef, void* stream) {
  WSEG_CHECK(c1 && c2 && r1 && r2 && Gc1 && Gc2 && dlt1 && dlt2 && er_sum, "er_ecr_prep: bad arguments");
  const long total = (long)N * npix;
  hipLaunchKernelGGL(er_ecr_prep_kernel, GRID1(total), 0, ST, c1, c2, r1, r2, Gc1, Gc2, dlt1, dlt2, er_sum, npix, er_coef, total);
  WSEG_LAUNCH_CHECK();
  return 0;
}
extern "C" int wseg_ecr_backward(const float* dlt, const float* res, float* Gr, int N, int per_row, int k, float coef, void* stream) {
  WSEG_CHECK(dlt && res && Gr, "ecr_backward: bad arguments");
  const long total = (long)N * per_row;
  hipLaunchKernelGGL(ecr_bwd_kernel, GRID1(total), 0, ST, dlt, res, Gr, per_row, k, coef, total);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_rows_resize_forward(const void* head, int ld, float* F, int N, int ih, int iw, int oh, int ow, int dtype, void* stream) {
  WSEG_CHECK(head && F && ld >= 128, "rows_resize_forward: bad arguments");
  const long total = (long)N * oh * ow * 128;
  if (dtype == WSEG_BF16) hipLaunchKernelGGL(rows_resize_fwd_kernel<WSEG_BF16>, GRID1(total), 0, ST, head, ld, F, ih, iw, oh, ow, total);
  else hipLaunchKernelGGL(rows_resize_fwd_kernel<WSEG_F32>, GRID1(total), 0, ST, head, ld, F, ih, iw, oh, ow, total);
  WSEG_LAUNCH_CHECK();
  return 0;
}
extern "C" int wseg_head_grad_fused(const float* dF, const float* d_cam_low, const void* head, void* d_head, int ld,
                                    int N, int ih, int iw, int oh, int ow, int dtype, void* stream) {
  WSEG_CHECK(dF && head && d_head && ld % 8 == 0 && ld >= 152, "head_grad_fused: bad arguments");
  const long total = (long)N * ih * iw * (ld / 8);
  if (dtype == WSEG_BF16) hipLaunchKernelGGL(head_grad_fused_kernel<WSEG_BF16>, GRID1(total), 0, ST, dF, d_cam_low, head, d_head, ld, ih, iw, oh, ow, total);
  else hipLaunchKernelGGL(head_grad_fused_kernel<WSEG_F32>, GRID1(total), 0, ST, dF, d_cam_low, head, d_head, ld, ih, iw, oh, ow, total);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_pseudo_label(const float* R, const float* label20, float bg_thr, int* y, float* ncam, int N, int npix, void* stream) {
  WSEG_CHECK(R && label20 && y && ncam && N > 0 && npix > 0, "pseudo_label: bad arguments");
  hipLaunchKernelGGL(pseudo_label_kernel, dim3(N), dim3(256), 0, ST, R, label20, bg_thr, y, ncam, npix);
  WSEG_LAUNCH_CHECK();
  return 0;
}
extern "C" int wseg_proto_candidates(const float* ncam, const float* F, const int* tie_idx, float* cand_val, float* cand_feat, int* cand_const,
                                     int N, int npix, int K, void* stream) {
  WSEG_CHECK(ncam && F && tie_idx && cand_val && cand_feat && cand_const && K >= 1 && K <= 64, "proto_candidates: bad arguments");
  const size_t P = (size_t)N * npix;
  WSEG_CHECK(P * 4 <= 128 * 1024 && (size_t)K <= P, "proto_candidates: P=%zu too large for one workgroup's LDS", P);
  hipLaunchKernelGGL(proto_candidates_kernel, dim3(21), dim3(256), P * 4, ST, ncam, F, tie_idx, cand_val, cand_feat, cand_const, N, npix, K);
  WSEG_LAUNCH_CHECK();
  return 0;
}
extern "C" int wseg_proto_merge(const float* cand_val, const float* cand_feat, const int* cand_const, float* protos, int world, int K,
                                long rank_stride, void* stream) {
  WSEG_CHECK(cand_val && cand_feat && cand_const && protos && world >= 1 && world * K <= 512 && K <= 64, "proto_merge: bad arguments");
  // rank_stride 0: contiguous [world][21][K] / [world][21][K][128] / [world][21]; else all three advance by rank_stride elements per rank
  const long rv = rank_stride ? rank_stride : 21L * K, rf = rank_stride ? rank_stride : 21L * K * 128, rc = rank_stride ? rank_stride : 21L;
  hipLaunchKernelGGL(proto_merge_kernel, dim3(21), dim3(128), 0, ST, cand_val, cand_feat, cand_const, protos, world, K, rv, rf, rc);
  WSEG_LAUNCH_CHECK();
  return 0;
}
