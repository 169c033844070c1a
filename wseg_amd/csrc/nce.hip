// nce.hip — the pixel-to-prototype contrast of contrast_train.py:245-334 as HIP kernels: the per-pixel records and the hard-pixel sampling that
// reads them (single rank: a sort in LDS; gathered batch: a radix select per class), and the fused similarities + InfoNCE terms + gradient.
#include <algorithm>
#include "loss_helpers.h"

namespace {

// ---- hard pixel sampling weights (contrast_train.py:302-331), single workgroup, P <= 8192.
//   key1 = S_own[p][y_p] (similarity order), key2 = random key or host flag.  w[p] = (#selections)/(2*half*C).
__global__ __launch_bounds__(1024) void intra_weights_kernel(const int* __restrict__ y, const float* __restrict__ S_own, int ld_s, const float* __restrict__ rkey,
                                                             const unsigned char* __restrict__ rand_flag, float* __restrict__ w, int P) {
  extern __shared__ unsigned long long keys[];              // [P2] sort buffer
  __shared__ int cnt[21], start[21], nclass;
  const int tid = threadIdx.x;
  int P2 = 1; while (P2 < P) P2 <<= 1;
  if (tid < 21) cnt[tid] = 0;
  __syncthreads();
  for (int p = tid; p < P; p += 1024) atomicAdd(&cnt[y[p]], 1);
  __syncthreads();
  if (tid == 0) { int s = 0, C = 0; for (int c = 0; c < 21; ++c) { start[c] = s; s += cnt[c]; if (cnt[c] > 0) ++C; } nclass = C; }
  for (int p = tid; p < P; p += 1024) w[p] = 0.f;
  __syncthreads();
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1 && rand_flag) {                           // host-provided random half (RNG-parity mode)
      for (int p = tid; p < P; p += 1024) if (rand_flag[p]) { const int c = y[p]; const int half = cnt[c] / 2; if (cnt[c] >= 2) w[p] += 1.f / (2.f * half * nclass); }
      break;
    }
    for (int i = tid; i < P2; i += 1024) {
      unsigned long long k = ~0ull;
      if (i < P) {
        const float f = pass == 0 ? (ld_s == 1 ? S_own[i] : S_own[(size_t)i * ld_s + y[i]]) : rkey[i];
        k = ((unsigned long long)y[i] << 56) | ((unsigned long long)f2key(f) << 24) | (unsigned long long)i;   // i < 2^24
      }
      keys[i] = k;
    }
    __syncthreads();
    for (int k2 = 2; k2 <= P2; k2 <<= 1)
      for (int j = k2 >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < P2; i += 1024) {
          const int l = i ^ j;
          if (l > i) {
            const bool up = (i & k2) == 0;
            const unsigned long long a = keys[i], b = keys[l];
            if ((a > b) == up) { keys[i] = b; keys[l] = a; }
          }
        }
        __syncthreads();
      }
    for (int i = tid; i < P; i += 1024) {
      const unsigned long long k = keys[i];
      const int c = (int)(k >> 56); const int p = (int)(k & 0xFFFFFFull);
      const int len = cnt[c], r = i - start[c];
      if (len < 2) continue;
      const int half = len / 2;
      bool selected;
      if (pass == 0) { const int kk = (int)((double)len * 0.6); selected = r >= kk - half && r < kk; }
      else selected = r < half;
      if (selected) w[p] += 1.f / (2.f * half * nclass);
    }
    __syncthreads();
  }
}

// ---- hard-pixel sampling over the GLOBAL batch (data parallel; contrast_train.py:302-334 runs on the gathered batch).
// The per-pixel records {label, own-class similarity, random key} of every rank are written by nce_records_kernel below and all-gathered.
// intra_weights_global: `rec` = gathered records, rank r's [3][P] block at rec + r*rank_stride (global pixel g = r*P + p).  Per class c with
// len >= 2 pixels the reference keeps (a) a random half and (b) the pixels whose similarity rank lies in
// [int(0.6 len) - len/2, int(0.6 len)); both are order statistics of unique 56-bit keys (value << 24 | g), found by a 7-pass radix
// select — no global sort.  ONE WORKGROUP PER CLASS (grid 21; round 2 ran all 63 selections in a single workgroup, which at world 8 —
// 32 768 records per view — sat serially between the all-gather and the fused NCE launch): workgroup c counts its members (and which classes
// occur at all), runs the three selections of its class over the gathered records (per-wave private histograms: the first digit of a
// similarity or a uniform key is the same for most of a class, so a shared histogram serialises on two or three buckets), and writes the
// weights of ITS class's pixels of this rank: w[p] = scale * (#selections of p) / (2 * (len/2) * classes present).
__global__ __launch_bounds__(1024) void intra_weights_global_kernel(const float* __restrict__ rec, float* __restrict__ w, int P, int ranks,
                                                                    int own_rank, float scale, long rank_stride) {
  __shared__ unsigned hist[16][3][256];                       // [wave][selection][bucket]
  __shared__ unsigned long long prefix[3];
  __shared__ unsigned remaining[3];
  __shared__ int present[21], cnt_s, nclass_s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = blockIdx.x;
  // Sweep over the records of ranks [r0, r1): every lane takes FOUR consecutive pixels per step as 16-byte loads of the label / similarity / key
  // rows (all three requested before any is used; no per-record division), fn(g, label, similarity bits, key bits) per record.  vec: rows 16-byte aligned.
  const bool vec = (P & 3) == 0 && (rank_stride & 3) == 0 && (reinterpret_cast<size_t>(rec) & 15) == 0;
  auto sweep = [&](int r0, int r1, bool need_keys, auto&& fn) {
    for (int r = r0; r < r1; ++r) {
      const float* base = rec + (size_t)r * rank_stride;
      for (int p0 = tid * 4; p0 < P; p0 += 4096) {
        float lb[4], sv[4] = {0.f, 0.f, 0.f, 0.f}, kv[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec) {
          const f32x4 l4 = *reinterpret_cast<const f32x4*>(base + p0);
          f32x4 s4 = (f32x4){0.f, 0.f, 0.f, 0.f}, k4 = s4;
          if (need_keys) { s4 = *reinterpret_cast<const f32x4*>(base + P + p0); k4 = *reinterpret_cast<const f32x4*>(base + 2 * (size_t)P + p0); }
#pragma unroll
          for (int e = 0; e < 4; ++e) { lb[e] = l4[e]; sv[e] = s4[e]; kv[e] = k4[e]; }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int p = min(p0 + e, P - 1);
            lb[e] = base[p];
            if (need_keys) { sv[e] = base[P + p]; kv[e] = base[2 * (size_t)P + p]; }
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (p0 + e < P) fn(r * P + p0 + e, __float_as_int(lb[e]), f2key(sv[e]), f2key(kv[e]));
      }
    }
  };
  if (tid < 21) present[tid] = 0;
  if (tid == 0) cnt_s = 0;
  __syncthreads();
  int mine = 0;
  sweep(0, ranks, false, [&](int, int l, unsigned, unsigned) {
    present[l] = 1;                                          // (plain store: every writer writes the same value)
    mine += l == c ? 1 : 0;
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if (lane == 0 && mine) atomicAdd(&cnt_s, mine);
  __syncthreads();
  if (tid == 0) { int C = 0; for (int k = 0; k < 21; ++k) C += present[k]; nclass_s = C; }
  const int len = cnt_s, half = len / 2, kk = (int)((double)len * 0.6);
  const int g0 = own_rank * P;
  if (len < 2) {                                             // (uniform) absent or single-pixel class: counted in C, no term (contrast_train.py:312-313)
    sweep(own_rank, own_rank + 1, false, [&](int g, int l, unsigned, unsigned) { if (l == c) w[g - g0] = 0.f; });
    return;
  }
  if (tid < 3) {
    prefix[tid] = 0ull;
    remaining[tid] = (unsigned)(tid == 0 ? kk - half : (tid == 1 ? kk : half));     // 0-based target rank within the class
  }
  for (int shift = 48; shift >= 0; shift -= 8) {
    for (int i = tid; i < 16 * 3 * 256; i += 1024) (&hist[0][0][0])[i] = 0u;
    __syncthreads();
    const unsigned long long pf0 = prefix[0], pf1 = prefix[1], pf2 = prefix[2];
    sweep(0, ranks, true, [&](int g, int l, unsigned sk, unsigned rk) {
      if (l != c) return;
      const unsigned long long ks = ((unsigned long long)sk << 24) | (unsigned long long)g, kr = ((unsigned long long)rk << 24) | (unsigned long long)g;
      const unsigned bs = (unsigned)(ks >> shift) & 255u, br = (unsigned)(kr >> shift) & 255u;
      if (shift == 48 || (ks >> (shift + 8)) == (pf0 >> (shift + 8))) atomicAdd(&hist[wv][0][bs], 1u);
      if (shift == 48 || (ks >> (shift + 8)) == (pf1 >> (shift + 8))) atomicAdd(&hist[wv][1][bs], 1u);
      if (shift == 48 || (kr >> (shift + 8)) == (pf2 >> (shift + 8))) atomicAdd(&hist[wv][2][br], 1u);
    });
    __syncthreads();
    if (wv < 3) {                                  // one wave per selection: lane l owns buckets 4l..4l+3 (summed over the 16 private copies)
      const int s_ = wv;
      unsigned cs[4] = {0u, 0u, 0u, 0u};
      for (int k = 0; k < 16; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) cs[j] += hist[k][s_][lane * 4 + j];
      }
      const unsigned rem = remaining[s_];
      const unsigned sum = cs[0] + cs[1] + cs[2] + cs[3];
      unsigned inc = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
      unsigned cum = inc - sum;
      if (cum <= rem && rem < inc) {               // exactly one lane when the class holds more than `rem` pixels
        int b = -1;
#pragma unroll
        for (int j = 0; j < 4; ++j) if (b < 0) { if (rem < cum + cs[j]) b = lane * 4 + j; else cum += cs[j]; }
        prefix[s_] |= (unsigned long long)b << shift;
        remaining[s_] = rem - cum;
      }
    }
    __syncthreads();
  }
  const float unit = scale / (2.f * (float)half * (float)nclass_s);
  const unsigned long long t0 = prefix[0], t1 = prefix[1], t2 = prefix[2];
  sweep(own_rank, own_rank + 1, true, [&](int g, int l, unsigned sk, unsigned rk) {
    if (l != c) return;
    const unsigned long long ks = ((unsigned long long)sk << 24) | (unsigned long long)g, kr = ((unsigned long long)rk << 24) | (unsigned long long)g;
    const int n_sel = (ks >= t0 && ks < t1 ? 1 : 0) + (kr < t2 ? 1 : 0);
    w[g - g0] = unit * (float)n_sel;
  });
}


// ============================================================================================================================
// Fused pixel-to-prototype contrast (contrast_train.py:245-334): the product path.  Two launches per step for BOTH views:
//   nce_records_kernel  F, prototypes, labels            -> per-pixel record {label, similarity to its own class, random key}
//                                                           (the inputs of the hard-pixel sampling)            520 B / pixel
//   nce_fused_kernel    F, both prototype sets, labels,
//                       hard-pixel weights                -> dF and the three loss sums                         1.03 KB / pixel
// The features are read once per launch and nothing but dF / 12-byte records is written: neither the normalised features nor
// [P,21] similarity rows ever reach HBM.  (An unfused formulation that wrote both was the tests' reference until
// tests/test_gpu_loss_kernels.py checked these kernels against float64; it is retired.)
// Similarities: one wave = 16 pixels x [21 own | 21 other | 6 pad] classes x 128 channels as 96 v_mfma_f32_16x16x4_f32 (exact
// f32), identical arithmetic in both kernels, so the record's similarity is bit-identical to the one the loss uses.
struct NceView { const float* F; const float* p_own; const float* p_oth; const int* y_own; const int* y_oth; const float* w_intra;
                 const float* rkey; float* rec; float* dF; };
struct NceArgs { NceView v[2]; int nviews, P; float coef_cross, coef_intra; float* sums; };

// similarities of 16 pixels (rows grp16*16 ..) to the 42 prototypes held in pb; returns acc[t][r] = S[pixel 4g+r][class t*16+col]
// already divided by the pixel's norm, and the lane's own row norm in `nr` (row = lane & 15)
// Feature tile of 16 pixels (8 KB) through LDS (the record pass): lane (col, g) needs 16 B at channel 16b + 4g of pixel `col` — 64-B pieces of 16
// different rows per load instruction when fetched straight into registers.  Here 8 LDS-DMA instructions fetch two WHOLE rows each (1 KB contiguous
// per wave instruction) and cost no registers, so a wave keeps TWO tiles (16 KB) in flight; the 16-B chunks are XOR-swizzled on the source side
// (chunk ^ row in the low 4 bits) so that the fragment reads of one chunk index from 16 rows fall into 16 different bank groups.  The tile belongs
// to ONE wave: no barrier, only that wave's vmcnt.  Measured at P = 2^22 per view: 2.92 -> 3.25 TB/s (exact f32), 2.83 -> 3.84 TB/s (split-bf16);
// with one tile in flight the staging alone changed nothing — these kernels are bound by bytes in flight per CU (latency), not by the load shape.
__device__ __forceinline__ void nce_tile_dma(const float* __restrict__ F, int P, int grp16, int lane, char* tile) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = 2 * i + (lane >> 5), pc = lane & 31;           // row inside the tile, physical 16-B chunk inside the row
    const int lc = (pc & 16) | ((pc ^ r) & 15);                  // logical chunk stored there
    glds16(F + (size_t)min(grp16 * 16 + r, P - 1) * 128 + lc * 4, tile + i * 1024);
  }
}
__device__ __forceinline__ void nce_frags_global(const float* __restrict__ F, int P, int grp16, int col, int g, f32x4 (&a)[8]) {
  const float* fr = F + (size_t)min(grp16 * 16 + col, P - 1) * 128 + 4 * g;
#pragma unroll
  for (int b = 0; b < 8; ++b) a[b] = *reinterpret_cast<const f32x4*>(fr + b * 16);
}
__device__ __forceinline__ void nce_frags_lds(const char* tile, int col, int g, f32x4 (&a)[8]) {
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const int lc = 4 * b + g;
    a[b] = *reinterpret_cast<const f32x4*>(tile + col * 512 + (((lc & 16) | ((lc ^ col) & 15)) << 4));
  }
}

template <int NT = 3>   // NT = 2: only the first 32 classes (the record pass needs the own-view prototypes only)
__device__ __forceinline__ void nce_sims16(const f32x4 (&a)[8], int col, int g, const f32x4 (&pb)[3][8], f32x4 (&acc)[3], float& nr) {
  float ss = 0.f;
#pragma unroll
  for (int b = 0; b < 8; ++b) ss += a[b][0] * a[b][0] + a[b][1] * a[b][1] + a[b][2] * a[b][2] + a[b][3] * a[b][3];
  ss += __shfl_xor(ss, 16, 64); ss += __shfl_xor(ss, 32, 64);
  nr = sqrtf(ss);
  const float inv = 1.f / fmaxf(nr, 1e-12f);
#pragma unroll
  for (int t = 0; t < 3; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int b = 0; b < 8; ++b)
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[b][e], pb[t][b][e], acc[t], 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float ir = __shfl(inv, 4 * g + r, 64);
#pragma unroll
    for (int t = 0; t < 3; ++t) acc[t][r] *= ir;
  }
}

__device__ __forceinline__ void nce_load_protos(const float* __restrict__ p_own, const float* __restrict__ p_oth, int col, int g, f32x4 (&pb)[3][8]) {
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int cc = t * 16 + col;
    const float* src = cc < 21 ? p_own + cc * 128 : (cc < 42 && p_oth ? p_oth + (cc - 21) * 128 : nullptr);
#pragma unroll
    for (int b = 0; b < 8; ++b) pb[t][b] = src ? *reinterpret_cast<const f32x4*>(src + b * 16 + 4 * g) : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
}

// ---- split-bf16 form of the same contraction (the record pass in the bf16 and bf16x3 precision modes; the fp32 mode and the fused loss kernel
// keep the exact-f32 MFMA above — a split-bf16 form of the fused kernel was measured: 2.97 vs 2.79 TB/s at P = 2^22, equal at the real shape, at the
// price of register spills; not kept).
// Operands x = hi + lo (bf16 each), product lo.hi + hi.lo + hi.hi on v_mfma_f32_16x16x32_bf16: 36 MFMAs of 16 cycles per 16 pixels instead of
// 96 of 32 — the exact-f32 MFMA (1/16 of the bf16 rate) is what bounds the f32 kernels, not HBM.  Lane (col, g) holds channels
// 32c + 4g + e and 32c + 16 + 4g + e (e = 0..3) of chunk c: exactly its two 16-B feature loads 2c and 2c + 1, same map for both operands.
struct NceProtosX3 { bf16x8 hi[3][4], lo[3][4]; };
__device__ __forceinline__ void nce_load_protos_x3(const float* __restrict__ p_own, const float* __restrict__ p_oth, int col, int g, NceProtosX3& pp) {
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int cc = t * 16 + col;
    const float* src = cc < 21 ? p_own + cc * 128 : (cc < 42 && p_oth ? p_oth + (cc - 21) * 128 : nullptr);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 q0 = (f32x4){0.f, 0.f, 0.f, 0.f}, q1 = q0;
      if (src) { q0 = *reinterpret_cast<const f32x4*>(src + 32 * c + 4 * g); q1 = *reinterpret_cast<const f32x4*>(src + 32 * c + 16 + 4 * g); }
      split_bf16x8(q0, q1, pp.hi[t][c], pp.lo[t][c]);
    }
  }
}
template <int NT = 3>
__device__ __forceinline__ void nce_sims16_x3(const f32x4 (&a)[8], int col, int g, const NceProtosX3& pp, f32x4 (&acc)[3], float& nr) {
  float ss = 0.f;
#pragma unroll
  for (int b = 0; b < 8; ++b) ss += a[b][0] * a[b][0] + a[b][1] * a[b][1] + a[b][2] * a[b][2] + a[b][3] * a[b][3];
  ss += __shfl_xor(ss, 16, 64); ss += __shfl_xor(ss, 32, 64);
  nr = sqrtf(ss);
  const float inv = 1.f / fmaxf(nr, 1e-12f);
#pragma unroll
  for (int t = 0; t < 3; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    bf16x8 ah, al;
    split_bf16x8(a[2 * c], a[2 * c + 1], ah, al);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, pp.hi[t][c], acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, pp.lo[t][c], acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, pp.hi[t][c], acc[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float ir = __shfl(inv, 4 * g + r, 64);
#pragma unroll
    for (int t = 0; t < 3; ++t) acc[t][r] *= ir;
  }
}

// One wave walks the 16-pixel tiles id = first + k * (waves in the grid) of BOTH views (view 0's tiles, then view 1's) with TWO tiles always in
// flight: tile k + 2 is requested into the buffer tile k was read from as soon as its fragments are in registers, so the wave never drains its
// queue (the unpipelined form — request two tiles, wait for both, compute both — had nothing in flight while it computed).  The record of pixel j
// of a tile is gathered into lane j (8 ds_bpermute from the lane that holds the pixel's own class), so every tile issues the SAME number of memory
// operations (8 LDS-DMA + label + key loads, 2-3 stores) and the only wait is one counted vmcnt.
template <bool X3>
__global__ __launch_bounds__(256) void nce_records_kernel(const NceArgs a) {
  // per wave: two 8-KB feature tiles, then per buffer 64 labels | 64 keys (lanes 0..15 are the tile's pixels).  ONE __shared__ object: beside a
  // second one the compiler puts a vmcnt(0) in front of every ds_read while LDS-DMA is in flight
  __shared__ __attribute__((aligned(16))) char lds[4][2 * 8192 + 2 * 512];
  const int lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  char* tile = lds[wv];
  char* side = lds[wv] + 2 * 8192;
  const int P = a.P, ngrp = (P + 15) >> 4, total = a.nviews * ngrp, W = gridDim.x * 4;
  const int first = blockIdx.x * 4 + wv;
  if (first >= total) return;
  const bool has_key = a.v[0].rkey != nullptr;               // (both views or none: checked on the host)
  f32x4 pb[X3 ? 1 : 3][8];
  NceProtosX3 pp;
  // (labels and keys travel through LDS as well: a register that is the destination of a load in flight across the loop edge makes the compiler
  //  copy it at the latch behind a vmcnt(0))
  auto request = [&](int id, int buf) {                       // tile `id` (clamped: a dummy request keeps the operation count fixed) -> buffer buf
    id = min(id, total - 1);
    const int vi = id >= ngrp ? 1 : 0;
    const NceView& v = a.v[vi];
    const int grp = id - vi * ngrp;
    nce_tile_dma(v.F, P, grp, lane, tile + buf * 8192);
    const int p = min(grp * 16 + col, P - 1);
    glds4(v.y_own + p, side + buf * 512);
    if (has_key) glds4(v.rkey + p, side + buf * 512 + 256);
  };
  int cur_v = -1;
  auto body = [&](int id, int buf) {                          // (buf is a literal at both call sites)
    const int vi = id >= ngrp ? 1 : 0, grp = id - vi * ngrp;
    const NceView& v = a.v[vi];
    if (vi != cur_v) {                                        // prototypes of the view (wave-uniform branch; at most twice per wave)
      cur_v = vi;
      if constexpr (X3) nce_load_protos_x3(v.p_own, nullptr, col, g, pp);
      else {
        nce_load_protos(v.p_own, nullptr, col, g, pb);
#pragma unroll
        for (int t = 0; t < 2; ++t)                           // a USE inside the branch: the compiler waits for these loads here, not (with a
#pragma unroll                                                //  vmcnt(0), which would drain the tiles in flight) at their first use in the loop
          for (int b = 0; b < 8; ++b) asm volatile("" : "+v"(pb[t][b]));
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else if (has_key) asm volatile("s_waitcnt vmcnt(13)" ::: "memory");   // younger than tile k: stores(k-2) 3, tile k+1 10, stores(k-1) 3
    else asm volatile("s_waitcnt vmcnt(11)" ::: "memory");                  // (2, 9, 2)
    f32x4 acc[3], fa[8]; float nr;
    nce_frags_lds(tile + buf * 8192, col, g, fa);
    const int yc = *reinterpret_cast<const int*>(side + buf * 512 + col * 4);
    const float kc = *reinterpret_cast<const float*>(side + buf * 512 + 256 + col * 4);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    request(id + 2 * W, buf);
    if constexpr (X3) nce_sims16_x3<2>(fa, col, g, pp, acc, nr); else nce_sims16<2>(fa, col, g, pb, acc, nr);
    // lane j < 16 <- similarity of pixel j to its class c: held by lane (c & 15) + 16 * (j >> 2) in acc[c >> 4][j & 3]
    const int src = (yc & 15) + 16 * (col >> 2);
    float sim = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float x = __shfl(acc[t][r], src, 64);
        if ((yc >> 4) == t && (col & 3) == r) sim = x;
      }
    const int p = grp * 16 + col;
    if (g == 0 && p < P) {
      v.rec[p] = __int_as_float(yc); v.rec[P + p] = sim;
      if (has_key) v.rec[2 * P + p] = kc;
    }
  };
  request(first, 0);
  request(first + W, 1);
  for (int id = first; id < total; id += 2 * W) {
    body(id, 0);
    if (id + W < total) body(id + W, 1);
  }
}

__global__ __launch_bounds__(256, 2) void nce_fused_kernel(const NceArgs a) {
  __shared__ float slab[4][64][45];                          // per wave: [pixel][42 similarities -> 44 dS values | norm]
  __shared__ float red[3][4];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), col = lane & 15, g = lane >> 4;
  const float itau = 10.f;                                   // 1 / 0.1
  const int P = a.P, ngrp = (P + 63) >> 6;
  float l_cross = 0.f, l_cross2 = 0.f, l_intra = 0.f;
  {
    for (int gid = blockIdx.x * 4 + wv; gid < a.nviews * ngrp; gid += gridDim.x * 4) {   // both views share the grid
      const NceView& v = a.v[gid >= ngrp ? 1 : 0];
      const int grp = gid >= ngrp ? gid - ngrp : gid;
      // ---------------- similarities of 4 x 16 pixels -> the wave's slab.  The features of sub-tile s + 1 are requested before the 96 MFMAs of
      // sub-tile s (two register sets), the labels / weights of phase A before everything: no load of this phase is waited for right after its issue
      const int pA = min(grp * 64 + lane, P - 1);
      const int yo = v.y_own[pA], yt = v.y_oth[pA];
      const float wA = v.w_intra[pA];
      {
        const float *po = v.p_own, *pt = v.p_oth;            // (opaque copies: keeps the compiler from hoisting the 96 prototype registers
        asm volatile("" : "+s"(po), "+s"(pt));               //  of this phase and the 88 of phase B over the whole loop — they never overlap)
        f32x4 pb[3][8], f0[8], f1[8];
        nce_frags_global(v.F, P, grp * 4, col, g, f0);
        nce_load_protos(po, pt, col, g, pb);
        auto sims_of = [&](int sub, const f32x4 (&fa)[8]) {
          f32x4 acc[3]; float nr;
          nce_sims16(fa, col, g, pb, acc, nr);
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int t = 0; t < 3; ++t) {
              const int cc = t * 16 + col;
              if (cc < 42) slab[wv][sub * 16 + 4 * g + r][cc] = acc[t][r];
            }
          if (g == 0) slab[wv][sub * 16 + col][44] = nr;
        };
        nce_frags_global(v.F, P, grp * 4 + 1, col, g, f1); __builtin_amdgcn_sched_barrier(0); sims_of(0, f0);
        nce_frags_global(v.F, P, grp * 4 + 2, col, g, f0); __builtin_amdgcn_sched_barrier(0); sims_of(1, f1);
        nce_frags_global(v.F, P, grp * 4 + 3, col, g, f1); __builtin_amdgcn_sched_barrier(0); sims_of(2, f0);
        sims_of(3, f1);
      }
      __builtin_amdgcn_wave_barrier();
      // ---------------- phase A, lane = pixel: the three InfoNCE terms and d(loss)/d(similarity)
      {
        const int p = grp * 64 + lane;
        const bool ok = p < P;
        const int pc = min(p, P - 1);
        float so[21], st[21];
#pragma unroll
        for (int c = 0; c < 21; ++c) { so[c] = slab[wv][lane][c]; st[c] = slab[wv][lane][21 + c]; }
        const float wi = ok ? wA : 0.f;
        float eo[21], et[21], sum_o = 0.f, sum_t = 0.f, e_yo_t = 0.f, e_yt_o = 0.f, e_yo_o = 0.f;
#pragma unroll
        for (int c = 0; c < 21; ++c) {
          eo[c] = expf(so[c] * itau); et[c] = expf(st[c] * itau);
          sum_o += eo[c]; sum_t += et[c];
          if (c == yo) { e_yo_t = et[c]; e_yo_o = eo[c]; }
          if (c == yt) e_yt_o = eo[c];
        }
        float a2 = e_yo_o;                                   // semi-hard negatives: similarity ranks 3..12 (descending, lower index first on ties)
        unsigned negmask = 0;
#pragma unroll
        for (int c = 0; c < 21; ++c) {
          int rank = 0;
#pragma unroll
          for (int c2 = 0; c2 < 21; ++c2) rank += (so[c2] > so[c] || (so[c2] == so[c] && c2 < c)) ? 1 : 0;
          if (rank >= 3 && rank <= 12) { negmask |= 1u << c; a2 += eo[c]; }
        }
        if (ok) {
          l_cross += -logf(e_yo_t / sum_t) * a.coef_cross;   // cross-prototype: other view's prototypes, own label (:262)
          l_cross2 += -logf(e_yt_o / sum_o) * a.coef_cross;  // cross-pseudo-label: own prototypes, other label (:272)
          if (wi != 0.f) l_intra += -logf(e_yo_o / a2) * wi * a.coef_intra;
        }
        const float kc = ok ? a.coef_cross * itau : 0.f, ki = a.coef_intra * wi * itau;
#pragma unroll
        for (int c = 0; c < 21; ++c) {
          float go = kc * (eo[c] / sum_o - (c == yt ? 1.f : 0.f));
          if (wi != 0.f) go += ki * (((c == yo ? 1.f : 0.f) + ((negmask >> c) & 1u)) * eo[c] / a2 - (c == yo ? 1.f : 0.f));
          slab[wv][lane][c] = go;
          slab[wv][lane][21 + c] = kc * (et[c] / sum_t - (c == yo ? 1.f : 0.f));
        }
        slab[wv][lane][42] = 0.f; slab[wv][lane][43] = 0.f;
      }
      __builtin_amdgcn_wave_barrier();
      // ---------------- phase B: d fn[ch][px] = sum_class [P_own|P_oth]^T[ch][class] * dS[class][px], then the F.normalize backward
      {
        const float *po = v.p_own, *pt = v.p_oth;
        asm volatile("" : "+s"(po), "+s"(pt));
        f32x4 f0[8], f1[8];
        nce_frags_global(v.F, P, grp * 4, col, g, f0);       // (second touch of the wave's own 32 KB of features: cache-resident; sub-tile s + 1 is
        float pa[8][11];                                     //  requested before the 88 MFMAs of sub-tile s)    A operand: [P_own|P_oth]^T[ch = mt*16+col][class 4kk+g]
#pragma unroll
        for (int kk = 0; kk < 11; ++kk) {
          const int cc = 4 * kk + g;
          const float* src = cc < 21 ? po + cc * 128 : (cc < 42 ? pt + (cc - 21) * 128 : nullptr);
#pragma unroll
          for (int mt = 0; mt < 8; ++mt) pa[mt][kk] = src ? src[mt * 16 + col] : 0.f;
        }
        auto grad_of = [&](int sub, f32x4 (&f)[8]) {
          const int p = grp * 64 + sub * 16 + col;           // B / C column = pixel
          f32x4 acc[8];
#pragma unroll
          for (int mt = 0; mt < 8; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kk = 0; kk < 11; ++kk) {
            const float bv = slab[wv][sub * 16 + col][4 * kk + g];
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[mt][kk], bv, acc[mt], 0, 0, 0);
          }
          const float nr = slab[wv][sub * 16 + col][44];
          const float inv_s = 1.f / fmaxf(nr, 1e-12f);
          float dot = 0.f;
#pragma unroll
          for (int mt = 0; mt < 8; ++mt) {
            f[mt] = f[mt] * inv_s;
            dot += acc[mt][0] * f[mt][0] + acc[mt][1] * f[mt][1] + acc[mt][2] * f[mt][2] + acc[mt][3] * f[mt][3];
          }
          dot += __shfl_xor(dot, 16, 64); dot += __shfl_xor(dot, 32, 64);
          const float inv = nr > 1e-12f ? 1.f / nr : 0.f;    // below eps F.normalize divides by a constant: treat as dead
          if (p < P) {
#pragma unroll
            for (int mt = 0; mt < 8; ++mt)
              *reinterpret_cast<f32x4*>(v.dF + (size_t)p * 128 + mt * 16 + 4 * g) = (acc[mt] - f[mt] * dot) * inv;
          }
        };
        nce_frags_global(v.F, P, grp * 4 + 1, col, g, f1); __builtin_amdgcn_sched_barrier(0); grad_of(0, f0);
        nce_frags_global(v.F, P, grp * 4 + 2, col, g, f0); __builtin_amdgcn_sched_barrier(0); grad_of(1, f1);
        nce_frags_global(v.F, P, grp * 4 + 3, col, g, f1); __builtin_amdgcn_sched_barrier(0); grad_of(2, f0);
        grad_of(3, f1);
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { l_cross += __shfl_xor(l_cross, o, 64); l_cross2 += __shfl_xor(l_cross2, o, 64); l_intra += __shfl_xor(l_intra, o, 64); }
  if (lane == 0) { red[0][wv] = l_cross; red[1][wv] = l_cross2; red[2][wv] = l_intra; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const float t = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
    if (t != 0.f) atomicAdd(&a.sums[threadIdx.x], t);
  }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int wseg_intra_weights(const int* y, const float* S_own, int ld_s, const float* rkey, const unsigned char* rand_flag, float* w, int P, void* stream) {
  WSEG_CHECK(y && S_own && w && (rkey || rand_flag) && P > 0 && P <= 8192 && (ld_s == 1 || ld_s == 21), "intra_weights: needs 0 < P <= 8192 (got %d), ld_s 1 or 21", P);
  int P2 = 1; while (P2 < P) P2 <<= 1;
  hipLaunchKernelGGL(intra_weights_kernel, dim3(1), dim3(1024), (size_t)P2 * 8, ST, y, S_own, ld_s, rkey, rand_flag, w, P);
  WSEG_LAUNCH_CHECK();
  return 0;
}
extern "C" int wseg_intra_weights_global(const float* rec, float* w, int P, int ranks, int own_rank, float scale, long rank_stride, void* stream) {
  WSEG_CHECK(rec && w && P > 0 && ranks > 0 && own_rank >= 0 && own_rank < ranks && (long)P * ranks < (1L << 24) && rank_stride >= 3L * P,
             "intra_weights_global: bad arguments (P=%d ranks=%d own=%d)", P, ranks, own_rank);
  hipLaunchKernelGGL(intra_weights_global_kernel, dim3(21), dim3(1024), 0, ST, rec, w, P, ranks, own_rank, scale, rank_stride);   // one workgroup per class
  WSEG_LAUNCH_CHECK();
  return 0;
}

static int nce_args(const wseg_nce_view* views, int nviews, int P, NceArgs& a, bool need_grad) {
  WSEG_CHECK(views && (nviews == 1 || nviews == 2) && P > 0, "nce: needs 1 or 2 views and P > 0");
  a.nviews = nviews; a.P = P;
  for (int i = 0; i < nviews; ++i) {
    const wseg_nce_view& w = views[i];
    WSEG_CHECK(w.F && w.p_own && w.y_own, "nce: view %d: F, p_own, y_own are required", i);
    if (need_grad) WSEG_CHECK(w.p_oth && w.y_oth && w.w_intra && w.dF, "nce_fused: view %d: p_oth, y_oth, w_intra, dF are required", i);
    else WSEG_CHECK(w.rec && (w.rkey != nullptr) == (views[0].rkey != nullptr), "nce_records: view %d: rec is required; rkey for every view or none", i);
    a.v[i] = NceView{w.F, w.p_own, w.p_oth, w.y_own, w.y_oth, w.w_intra, w.rkey, w.rec, w.dF};
  }
  return 0;
}
extern "C" int wseg_nce_records(const wseg_nce_view* views, int nviews, int P, int split_bf16, void* stream) {
  NceArgs a{};
  if (int rc = nce_args(views, nviews, P, a, false)) return rc;
  const dim3 grid(std::min(2048, (nviews * ((P + 15) / 16) + 3) / 4));
  if (split_bf16) hipLaunchKernelGGL(nce_records_kernel<true>, grid, dim3(256), 0, ST, a);
  else hipLaunchKernelGGL(nce_records_kernel<false>, grid, dim3(256), 0, ST, a);
  WSEG_LAUNCH_CHECK();
  return 0;
}
extern "C" int wseg_nce_fused(const wseg_nce_view* views, int nviews, int P, float coef_cross, float coef_intra, float* sums, void* stream) {
  NceArgs a{};
  WSEG_CHECK(sums, "nce_fused: sums is null");
  if (int rc = nce_args(views, nviews, P, a, true)) return rc;
  a.coef_cross = coef_cross; a.coef_intra = coef_intra; a.sums = sums;
  hipLaunchKernelGGL(nce_fused_kernel, dim3(std::min(2048, (nviews * ((P + 63) / 64) + 3) / 4)), dim3(256), 0, ST, a);
  WSEG_LAUNCH_CHECK();
  return 0;
}
