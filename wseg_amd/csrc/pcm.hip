// pcm.hip — PCM affinity refinement (network/resnet38_contrast.py:63-75) without ever
// materialising the hw x hw affinity.  pcm_kernel: exact-f32 MFMA (v_mfma_f32_16x16x4_f32);
// pcm_bf16_kernel: the throughput mode's bf16 MFMA (v_mfma_f32_16x16x32_bf16).
//
//   S[i,j]   = Fh_i . Fh_j                       (Fh = L2-normalised f9 features, [hw][192])
//   forward : out[j][c] = sum_i relu(S[i,j]) * G[i][c]           G[:,21] == 1  -> out[j][21] = column sum
//             cam_rv[c][j] = out[j][c] / (out[j][21] + 1e-5)
//   backward: W[i,j] = (S[i,j] > 0) * sum_c P[i][c] * Q[j][c]
//             dFh[j][k] += sum_i W[i,j] * Fh[i][k]
//     called twice, (P,Q) = (G,DN) and (DN,G): the second call is the same sum over the transposed
//     dS, which yields the row-side gradient with the identical data flow.
//
// One workgroup = 64 columns j of one image (one 16-column sub-tile per wave, its Fh_j fragment
// held in registers); rows i stream through LDS in 32-row tiles by LDS-DMA (double buffered,
// XOR-swizzled 16-B chunks).  The two kernels share everything that does not depend on the MFMA
// shape — indices, column fragments, staging, the tile walk, the epilogue — and keep their own
// S / gate / accumulate products.
#include "common.h"

namespace {

constexpr int KF = 192;                     // feature channels
constexpr int IT = 32;                      // rows per i-tile

// ---- LDS swizzles: slot of 16-B chunk c in tile row `row`.  Each is an XOR, so it is its own inverse: staging calls it with the slot
// to find the source chunk, every read calls it with the chunk to find the slot.
// f32 Fh tile (768-B rows, all rows on one bank phase): the 16 rows of a ds_read_b128 fragment (row = col, one chunk) land in 16 slots;
// the backward's accumulate product reads single floats of rows 4g + r through the same map.
__device__ constexpr int swz_fh(int c, int row) { return (c & ~15) | ((c ^ row) & 15); }
// f32 P / G tile (128-B rows, two rows per bank phase): ds_read_b128 rows of the gate product, single floats of the forward's accumulate product.
__device__ constexpr int swz_g(int c, int row) { return c ^ ((row >> 1) & 7); }
// bf16 Fb tile (384-B rows, two rows per bank phase): ds_read_b128 rows of the S product and the ds_read_b64_tr_b16 (rows 4g..4g+3,
// half a chunk per lane) of the backward's accumulate product.
__device__ constexpr int swz_fb(int c, int row) { return (c & ~7) | ((c ^ (row >> 1)) & 7); }
// bf16 P tile (64-B rows): read as it lies.
__device__ constexpr int swz_none(int c, int) { return c; }

struct PcmIdx { int lane, wid, n, j0, col, g; };      // wave `wid` owns columns j0..j0+15 of image n; lane = (g, col)
__device__ __forceinline__ PcmIdx pcm_idx() {
  const int tid = threadIdx.x;
  PcmIdx ix;
  ix.lane = tid & 63;
  ix.wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  ix.n = blockIdx.y;
  ix.j0 = blockIdx.x * 64 + ix.wid * 16;
  ix.col = ix.lane & 15;
  ix.g = ix.lane >> 4;
  return ix;
}

// This lane's fragment of column j0 + col (clamped to the image's last pixel): 16-B chunks b * 4 + g of its row; `rows` = the image's
// dense rows of ROW elements.
template <int ROW, int NB, class V, class T>
__device__ __forceinline__ void col_frag(const T* rows, const PcmIdx& ix, int hw, V (&f)[NB]) {
  const int jr = min(ix.j0 + ix.col, hw - 1);
  const V* src = reinterpret_cast<const V*>(rows + (size_t)jr * ROW);
#pragma unroll
  for (int b = 0; b < NB; ++b) f[b] = src[b * 4 + ix.g];
}

// One 1 KiB piece of a tile of CPR chunks (CPR * 16 bytes) per row by LDS-DMA: lane l fills slot piece * 64 + l of the tile from the
// swizzled chunk of image row i0 + row (`rows` = the image's dense source rows), or from the zero page behind the image's last row.
template <int CPR, int (*SWZ)(int, int), class T>
__device__ __forceinline__ void stage_piece(char* tile, int piece, int lane, const T* rows, int i0, int hw) {
  const int ci = piece * 64 + lane;
  const int row = ci / CPR, pc = ci - row * CPR;
  const int i = i0 + row;
  const char* src = (i < hw) ? reinterpret_cast<const char*>(rows) + (size_t)i * (CPR * 16) + SWZ(pc, row) * 16
                             : reinterpret_cast<const char*>(g_wseg_zero_page) + (lane & 15) * 16;
  glds16(src, tile + piece * 1024);
}

// The double-buffered walk over the 32-row tiles: stage(buf, i0) requests tile i0 into buffer buf, compute(buf) consumes a landed one.
template <class Stage, class Compute>
__device__ __forceinline__ void pcm_tile_walk(int hw, Stage stage, Compute compute) {
  const int nti = (hw + IT - 1) / IT;
  stage(0, 0);
  __syncthreads();
  int cur = 0;
  for (int it = 0; it < nti; ++it) {
    if (it + 1 < nti) stage(cur ^ 1, (it + 1) * IT);
    compute(cur);
    __syncthreads();
    cur ^= 1;
  }
}

// acc[t][reg] <-> (j = j0 + 4g + reg, nn = t*16 + col), the C/D layout of both MFMA shapes.
// forward : out0 = cam_rv [N][21][hw], out1 = den [N][hw]
// backward: out0 = dFh [N][hw][192], accumulated (this launch is the only writer of row j)
template <int BWD, int NT>
__device__ __forceinline__ void pcm_epilogue(const f32x4 (&acc)[NT], const PcmIdx& ix, int hw, float* __restrict__ out0, float* __restrict__ out1) {
  const int n = ix.n, col = ix.col;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int j = ix.j0 + 4 * ix.g + reg;
    if constexpr (!BWD) {
      const float den = __shfl(acc[1][reg], ix.g * 16 + 5, 64);    // column c = 21 lives in tile 1, col 5
      if (j < hw) {
        out0[((size_t)n * 21 + col) * hw + j] = acc[0][reg] / (den + 1e-5f);
        if (col < 5) out0[((size_t)n * 21 + 16 + col) * hw + j] = acc[1][reg] / (den + 1e-5f);
        if (col == 5) out1[(size_t)n * hw + j] = den;
      }
    } else if (j < hw) {
      float* dst = out0 + ((size_t)n * hw + j) * KF + col;
#pragma unroll
      for (int t = 0; t < NT; ++t) dst[t * 16] += acc[t][reg];
    }
  }
}

// ---- exact f32.  The S accumulator's C/D layout (col = lane&15, row = 4*(lane>>4)+reg) IS the A-operand layout of the second
// product when MFMA r takes k-index g <-> row 4g+r, so relu(S) / W goes from accumulator to operand without touching LDS.
// Stage = Fh tile [32 rows][192 f32] + P/G tile [32 rows][32 f32].
template <int BWD>
__global__ __launch_bounds__(256, 2) void pcm_kernel(const float* __restrict__ Fh, const float* __restrict__ Pm,
                                                     const float* __restrict__ Qm, float* __restrict__ out0,
                                                     float* __restrict__ out1, int hw) {
  constexpr int FROW = KF * 4;                // 768 B per Fh row
  constexpr int F_TILE = IT * FROW;           // 24576
  constexpr int BUF = F_TILE + IT * 128;      // 28672 per stage
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
  const PcmIdx ix = pcm_idx();
  const int lane = ix.lane, wid = ix.wid, col = ix.col, g = ix.g;
  const size_t img = (size_t)ix.n * hw;       // this image's first row
  const float* Fn = Fh + img * KF;
  const float* Pn = Pm + img * 32;

  f32x4 bj[12], qj[2];                        // Fh[j0+col][blk*16 + 4g + e], Q[j0+col][k2*16 + 4g + e]
  col_frag<KF>(Fn, ix, hw, bj);
  if (BWD) col_frag<32>(Qm + img * 32, ix, hw, qj);
  constexpr int NT = BWD ? 12 : 2;
  f32x4 acc[NT] = {};

  pcm_tile_walk(
      hw,
      [&](int buf, int i0) {                  // Fh tile: 24 pieces, 6 per wave; P/G tile: one piece per wave
        char* lf = smem + buf * BUF;
#pragma unroll
        for (int t = 0; t < 6; ++t) stage_piece<48, swz_fh>(lf, wid * 6 + t, lane, Fn, i0, hw);
        stage_piece<8, swz_g>(lf + F_TILE, wid, lane, Pn, i0, hw);
      },
      [&](int buf) {
        const char* lf = smem + buf * BUF;
        const char* lg = lf + F_TILE;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          const int row = sub * 16 + col;                      // A-operand row (pixel i) for this lane
          f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int b = 0; b < 12; ++b) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(lf + row * FROW + swz_fh(b * 4 + g, row) * 16);
#pragma unroll
            for (int e = 0; e < 4; ++e) s = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], bj[b][e], s, 0, 0, 0);
          }
          // s[r] = S[i = sub*16 + 4g + r][j = col]
          float wv[4];
          if (!BWD) {
#pragma unroll
            for (int r = 0; r < 4; ++r) wv[r] = fmaxf(s[r], 0.f);
          } else {
            f32x4 t = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2) {
              const f32x4 a = *reinterpret_cast<const f32x4*>(lg + row * 128 + swz_g(k2 * 4 + g, row) * 16);
#pragma unroll
              for (int e = 0; e < 4; ++e) t = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], qj[k2][e], t, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) wv[r] = s[r] > 0.f ? t[r] : 0.f;
          }
          // accumulate out[j][nn] += sum_i W[i,j] * V[i][nn]; MFMA r: k-index g <-> row i = 4g + r
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int vi = sub * 16 + 4 * g + r;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
              const int lc = t * 4 + (col >> 2);               // 16-B chunk of the V row (G forward, Fh backward) holding column t*16+col
              const char* v = BWD ? lf + vi * FROW + swz_fh(lc, vi) * 16 : lg + vi * 128 + swz_g(lc, vi) * 16;
              acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[r], *reinterpret_cast<const float*>(v + (col & 3) * 4), acc[t], 0, 0, 0);
            }
          }
        }
      });
  pcm_epilogue<BWD>(acc, ix, hw, out0, out1);
}

// ---- bf16 MFMA (throughput mode).  Same data flow as pcm_kernel, but every product runs on v_mfma_f32_16x16x32_bf16:
//   S      : Fb_i . Fb_j over 192 channels = 6 MFMAs per 16x16 sub-tile (A: ds_read_b128 rows, B: registers)
//   t      : P_i . Q_j over the 32 gate channels = 1 MFMA
//   acc    : out[j][n] += sum_{i in 32-row tile} W[i,j] V[i][n] = 1 MFMA per 16 columns n; its A operand is built
//            from BOTH sub-tiles' accumulators with k-slot (g,e) <-> row (e>>2)*16 + 4g + (e&3), so the values a
//            lane needs are its own; the matching B operand is two ds_read_b64_tr_b16 (rows 4g..4g+3 and 16+4g..).
// Inputs are bf16 copies (Fb [N][hw][192], P/Q [N][hw][32]); outputs stay f32.
// Backward (BWD): the gate-channel product t_ij = P_i . Q_j = sum_c G_ic g_jc / D_j - (sum_c g_jc rv_jc) / D_j is a DIFFERENCE of two sums that nearly
// cancel wherever G_i is close to the refined map rv_j (rv_j is the affinity-weighted mean of the G_i) — with both operands rounded to bf16 BEFORE the
// cancellation the f9 / f8_3 / f8_4 gradients came out at cosine 0.94 against the f32 kernels under identical gate decisions (round 3, the injected-
// decision test).  It is therefore computed in split precision: P = Ph + Pl, Q = Qh + Ql (bf16 each, 16-17 significant bits), t = Pl.Qh + Ph.Ql + Ph.Qh —
// 3 MFMAs instead of 1 beside the 6 of S.  S itself only decides the ReLU gate, and W = gate * t is rounded to bf16 AFTER the cancellation.
// Stage = Fb tile [32 rows][192 bf16] + P tile [32 rows][32 bf16] (backward: hi, then lo).
template <int BWD>
__global__ __launch_bounds__(256, 2) void pcm_bf16_kernel(const bf16_t* __restrict__ Fb, const bf16_t* __restrict__ Pm,
                                                          const bf16_t* __restrict__ Qm, const bf16_t* __restrict__ Pl_,
                                                          const bf16_t* __restrict__ Ql_, float* __restrict__ out0,
                                                          float* __restrict__ out1, int hw) {
  constexpr int FR = KF * 2;                  // 384 B per Fb row
  constexpr int F_T = IT * FR;                // 12288
  constexpr int P_T = IT * 64;                // 2048
  constexpr int STG = F_T + (BWD ? 2 : 1) * P_T;
  __shared__ __attribute__((aligned(16))) char smem[2 * STG];
  const PcmIdx ix = pcm_idx();
  const int lane = ix.lane, wid = ix.wid, col = ix.col, g = ix.g;
  const size_t img = (size_t)ix.n * hw;       // this image's first row
  const bf16_t* Fn = Fb + img * KF;
  const bf16_t* Pn = Pm + img * 32;
  const bf16_t* Pln = BWD ? Pl_ + img * 32 : nullptr;

  bf16x8 bj[6], qj[1], ql[1];                 // Fb[j0+col][32b + 8g + e], Qh / Ql[j0+col][8g + e]
  col_frag<KF>(Fn, ix, hw, bj);
  if (BWD) { col_frag<32>(Qm + img * 32, ix, hw, qj); col_frag<32>(Ql_ + img * 32, ix, hw, ql); }
  constexpr int NT = BWD ? 12 : 2;
  f32x4 acc[NT] = {};
  const int q = col >> 2, p = lane & 3;

  pcm_tile_walk(
      hw,
      [&](int buf, int i0) {                  // Fb tile: 12 pieces, 3 per wave; P tile: 2 pieces
        char* lf = smem + buf * STG;
#pragma unroll
        for (int t = 0; t < 3; ++t) stage_piece<24, swz_fb>(lf, wid * 3 + t, lane, Fn, i0, hw);
        if (wid < 2 || BWD)                   // waves 0, 1 stage the P tile; backward: waves 2, 3 stage the lo part behind it
          stage_piece<4, swz_none>(lf + F_T + (wid >> 1) * P_T, wid & 1, lane, wid < 2 ? Pn : Pln, i0, hw);
      },
      [&](int buf) {
        const char* lf = smem + buf * STG;
        const char* lp = lf + F_T;
        float wv[2][4];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          const int row = sub * 16 + col;
          f32x4 sv = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int b = 0; b < 6; ++b) {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(lf + row * FR + swz_fb(b * 4 + g, row) * 16);
            sv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bj[b], sv, 0, 0, 0);
          }
          if (!BWD) {
#pragma unroll
            for (int r = 0; r < 4; ++r) wv[sub][r] = fmaxf(sv[r], 0.f);
          } else {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(lp + row * 64 + g * 16);
            const bf16x8 al = *reinterpret_cast<const bf16x8*>(lp + P_T + row * 64 + g * 16);
            f32x4 tv = (f32x4){0.f, 0.f, 0.f, 0.f};
            tv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, qj[0], tv, 0, 0, 0);       // small terms first
            tv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, ql[0], tv, 0, 0, 0);
            tv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, qj[0], tv, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) wv[sub][r] = sv[r] > 0.f ? tv[r] : 0.f;
          }
        }
        // A operand of the accumulate product: k-slot (g, e) <-> tile row (e>>2)*16 + 4g + (e&3)
        bf16x8 wa;
#pragma unroll
        for (int e = 0; e < 8; ++e) wa[e] = (short)f32_to_bf16(wv[e >> 2][e & 3]);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          bf16x8 vb;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int row = h * 16 + 4 * g + q;                // lane 4q+p of the 16-lane group addresses row q of the 4-row block
            const char* v = BWD ? lf + row * FR + swz_fb(t * 2 + (p >> 1), row) * 16 + (p & 1) * 8 : lp + row * 64 + t * 32 + p * 8;
            const bf16x4 x = __builtin_amdgcn_ds_read_tr16_b64_v4i16((bf16x4 __attribute__((address_space(3)))*)v);
#pragma unroll
            for (int e = 0; e < 4; ++e) vb[h * 4 + e] = x[e];
          }
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa, vb, acc[t], 0, 0, 0);
        }
      });
  pcm_epilogue<BWD>(acc, ix, hw, out0, out1);
}

// Fh = F / (||F|| + 1e-5)   (one wave per pixel row of 192 channels)
template <int DT>
__global__ void l2norm_fwd_kernel(const void* __restrict__ F, int ldf, float* __restrict__ Fh, float* __restrict__ nrm, long rows) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  float v[3];
  float ss = 0.f;
#pragma unroll
  for (int t = 0; t < 3; ++t) { v[t] = elem<DT>::ld(F, (size_t)row * ldf + t * 64 + lane); ss += v[t] * v[t]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  const float nr = sqrtf(ss);
  const float r = 1.f / (nr + 1e-5f);
#pragma unroll
  for (int t = 0; t < 3; ++t) Fh[(size_t)row * KF + t * 64 + lane] = v[t] * r;
  if (lane == 0) nrm[row] = nr;
}

// dF = dFh/(n+eps) - F * (dFh.F) / (n (n+eps)^2)
template <int DT>
__global__ void l2norm_bwd_kernel(const void* __restrict__ F, int ldf, const float* __restrict__ dFh, const float* __restrict__ nrm,
                                  void* __restrict__ dF, int lddf, long rows) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  float v[3], d[3];
  float dot = 0.f;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    v[t] = elem<DT>::ld(F, (size_t)row * ldf + t * 64 + lane);
    d[t] = dFh[(size_t)row * KF + t * 64 + lane];
    dot += v[t] * d[t];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
  const float nr = nrm[row];
  const float r = 1.f / (nr + 1e-5f);
  const float k = nr > 0.f ? dot * r * r / nr : 0.f;
#pragma unroll
  for (int t = 0; t < 3; ++t) elem<DT>::st(dF, (size_t)row * lddf + t * 64 + lane, d[t] * r - v[t] * k);
}

// DN[j][c] = d_out[c][j]/D_j (c<21), DN[j][21] = -sum_c d_out[c][j]*out[c][j]/D_j, rest 0
__global__ void pcm_dn_kernel(const float* __restrict__ d_rv, const float* __restrict__ rv, const float* __restrict__ den,
                              float* __restrict__ DN, int hw, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;   // over N*hw
  if (idx >= total) return;
  const long n = idx / hw; const int j = (int)(idx - n * hw);
  const float inv = 1.f / (den[idx] + 1e-5f);
  float dd = 0.f;
  float* o = DN + idx * 32;
  for (int c = 0; c < 21; ++c) {
    const float g = d_rv[((size_t)n * 21 + c) * hw + j];
    dd += g * rv[((size_t)n * 21 + c) * hw + j];
    o[c] = g * inv;
  }
  o[21] = -dd * inv;
  for (int c = 22; c < 32; ++c) o[c] = 0.f;
}

}  // namespace

extern "C" int wseg_pcm_forward(const float* Fh, const float* G, float* cam_rv, float* den, int N, int hw, void* stream) {
  WSEG_CHECK(Fh && G && cam_rv && den && N > 0 && hw > 0, "pcm_forward: bad arguments");
  dim3 grid((hw + 63) / 64, N);
  hipLaunchKernelGGL(pcm_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, Fh, G, (const float*)nullptr, cam_rv, den, hw);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_pcm_backward(const float* Fh, const float* G, const float* d_cam_rv, const float* cam_rv, const float* den,
                                 float* DN /*[N][hw][32] scratch*/, float* dFh /*[N][hw][192], zeroed by caller*/, int N, int hw, void* stream) {
  WSEG_CHECK(Fh && G && d_cam_rv && cam_rv && den && DN && dFh && N > 0 && hw > 0, "pcm_backward: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const long total = (long)N * hw;
  hipLaunchKernelGGL(pcm_dn_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_cam_rv, cam_rv, den, DN, hw, total);
  dim3 grid((hw + 63) / 64, N);
  hipLaunchKernelGGL(pcm_kernel<1>, grid, dim3(256), 0, s, Fh, G, (const float*)DN, dFh, (float*)nullptr, hw);
  hipLaunchKernelGGL(pcm_kernel<1>, grid, dim3(256), 0, s, Fh, (const float*)DN, G, dFh, (float*)nullptr, hw);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_l2norm_forward(const void* F, int ldf, float* Fh, float* nrm, long rows, int dtype, void* stream) {
  WSEG_CHECK(F && Fh && nrm && rows > 0 && ldf >= KF, "l2norm_forward: bad arguments");
  dim3 grid((unsigned)((rows + 3) / 4));
  if (dtype == WSEG_BF16) hipLaunchKernelGGL(l2norm_fwd_kernel<WSEG_BF16>, grid, dim3(256), 0, (hipStream_t)stream, F, ldf, Fh, nrm, rows);
  else hipLaunchKernelGGL(l2norm_fwd_kernel<WSEG_F32>, grid, dim3(256), 0, (hipStream_t)stream, F, ldf, Fh, nrm, rows);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_l2norm_backward(const void* F, int ldf, const float* dFh, const float* nrm, void* dF, int lddf, long rows, int dtype, void* stream) {
  WSEG_CHECK(F && dFh && nrm && dF && rows > 0, "l2norm_backward: bad arguments");
  dim3 grid((unsigned)((rows + 3) / 4));
  if (dtype == WSEG_BF16) hipLaunchKernelGGL(l2norm_bwd_kernel<WSEG_BF16>, grid, dim3(256), 0, (hipStream_t)stream, F, ldf, dFh, nrm, dF, lddf, rows);
  else hipLaunchKernelGGL(l2norm_bwd_kernel<WSEG_F32>, grid, dim3(256), 0, (hipStream_t)stream, F, ldf, dFh, nrm, dF, lddf, rows);
  WSEG_LAUNCH_CHECK();
  return 0;
}

// bf16-MFMA PCM (throughput mode): Fb / Gb are bf16 copies of Fh [N][hw][192] and G [N][hw][32]
extern "C" int wseg_pcm_forward_bf16(const void* Fb, const void* Gb, float* cam_rv, float* den, int N, int hw, void* stream) {
  WSEG_CHECK(Fb && Gb && cam_rv && den && N > 0 && hw > 0, "pcm_forward_bf16: bad arguments");
  dim3 grid((hw + 63) / 64, N);
  hipLaunchKernelGGL(pcm_bf16_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)Fb, (const bf16_t*)Gb, (const bf16_t*)nullptr,
                     (const bf16_t*)nullptr, (const bf16_t*)nullptr, cam_rv, den, hw);
  WSEG_LAUNCH_CHECK();
  return 0;
}
extern "C" int wseg_pcm_backward_bf16(const void* Fb, const void* Gb, const void* Gl, const float* d_cam_rv, const float* cam_rv, const float* den,
                                      float* DN, void* DNb, void* DNl, float* dFh, int N, int hw, void* stream) {
  WSEG_CHECK(Fb && Gb && Gl && d_cam_rv && cam_rv && den && DN && DNb && DNl && dFh && N > 0 && hw > 0, "pcm_backward_bf16: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const long total = (long)N * hw;
  hipLaunchKernelGGL(pcm_dn_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_cam_rv, cam_rv, den, DN, hw, total);
  if (const int rc = wseg_split_bf16(DN, DNb, DNl, total * 32, stream)) return rc;
  dim3 grid((hw + 63) / 64, N);
  hipLaunchKernelGGL(pcm_bf16_kernel<1>, grid, dim3(256), 0, s, (const bf16_t*)Fb, (const bf16_t*)Gb, (const bf16_t*)DNb, (const bf16_t*)Gl, (const bf16_t*)DNl,
                     dFh, (float*)nullptr, hw);
  hipLaunchKernelGGL(pcm_bf16_kernel<1>, grid, dim3(256), 0, s, (const bf16_t*)Fb, (const bf16_t*)DNb, (const bf16_t*)Gb, (const bf16_t*)DNl, (const bf16_t*)Gl,
                     dFh, (float*)nullptr, hw);
  WSEG_LAUNCH_CHECK();
  return 0;
}
