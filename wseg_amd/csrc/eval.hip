// eval.hip — the evaluator's pixel counting (eval.py:22-52) on the device: a confusion matrix of two uint8 masks, and the whole
// background-threshold curve of a CAM dictionary in ONE pass (include/wseg_hip.h states the contracts).
//
// Both are streaming kernels: every pixel is read once (once per present plane), 16 bytes per lane where the bases are aligned, a
// scalar loop for the tail or for unaligned buffers.  Counters are integers only: a workgroup-private 32-bit histogram in LDS (LDS
// atomics), flushed once per workgroup with 64-bit global atomic adds of its non-zero cells, so the sums are exact and independent of
// the order in which workgroups arrive.
//
// The curve's histogram is [22][20][T+1], 107 KB of 32-bit cells at T = 60.  An image has K present classes (usually 1-3), and a pixel's
// winner is one of them or the FIRST absent class (score 0.0; a later absent class can never be the lowest index of the maximum), so
// the workgroup histogram is [22][K+1][T+1]: 21 KB at K = 3.  Where that exceeds 64 KiB (the dynamic-LDS size a launch gets without
// opting in; K >= 12 at T = 60, which no VOC image reaches) the kernel keeps no workgroup histogram and adds straight into the global
// buffer, the lanes of a wave that share a cell adding once: slower, exact all the same, and no second LDS geometry to maintain.
#include <math.h>
#include "common.h"

namespace {

constexpr int ROWS = WSEG_EVAL_ROWS, NCLS = WSEG_EVAL_CLASSES, MAXT = WSEG_EVAL_MAX_THR;
constexpr int THR_PAD = 2 * MAXT;                  // thresholds padded with +inf to a power of two: the branch-free search below
constexpr int CURVE_HEAD = THR_PAD + 2 * NCLS + 8; // dwords in front of the LDS histogram: thr, plane[], cls[] (+8: a multiple of 4)
constexpr int MAX_BLOCKS = 1024;
constexpr long MAX_PIXELS = 1L << 40;              // (a workgroup counts n / gridDim pixels in 32 bits)
constexpr size_t LDS_LIMIT = 65536;

__device__ __forceinline__ unsigned gt_row(unsigned g) { return g < 21u ? g : 21u; }

__global__ __launch_bounds__(256) void eval_confusion_kernel(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ gt,
                                                             long n, int vec, unsigned long long* __restrict__ conf) {
  __shared__ unsigned h[ROWS * ROWS];
  for (int j = threadIdx.x; j < ROWS * ROWS; j += 256) h[j] = 0u;
  __syncthreads();
  auto count = [&](unsigned g, unsigned p) {
    if (g != 255u) atomicAdd(&h[gt_row(g) * ROWS + gt_row(p)], 1u);
  };
  const long step = (long)gridDim.x * 256, first = (long)blockIdx.x * 256 + threadIdx.x;
  const long nvec = vec ? n / 16 : 0;
  for (long q = first; q < nvec; q += step) {
    const uint4 pv = reinterpret_cast<const uint4*>(pred)[q], gv = reinterpret_cast<const uint4*>(gt)[q];
    const unsigned pw[4] = {pv.x, pv.y, pv.z, pv.w}, gw[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int b = 0; b < 32; b += 8) count((gw[j] >> b) & 255u, (pw[j] >> b) & 255u);
  }
  for (long i = nvec * 16 + first; i < n; i += step) count(gt[i], pred[i]);
  __syncthreads();
  for (int j = threadIdx.x; j < ROWS * ROWS; j += 256)
    if (h[j]) atomicAdd(&conf[j], (unsigned long long)h[j]);
}

struct CurveArgs {
  float thr[MAXT];
  int plane[NCLS];       // live winner e reads this plane; -1: the first absent class, score 0.0
  int cls[NCLS];         // ... and is this class (ascending, so the first maximum is the lowest class)
  int nlive, T;
};

template <bool LDS_HIST>
__global__ __launch_bounds__(256) void eval_curve_kernel(const float* __restrict__ planes, long plane_stride, CurveArgs a,
                                                         const unsigned char* __restrict__ gt, long n, int vec,
                                                         unsigned long long* __restrict__ hist) {
  extern __shared__ unsigned lds[];
  float* s_thr = reinterpret_cast<float*>(lds);
  int* s_plane = reinterpret_cast<int*>(lds) + THR_PAD;
  int* s_cls = s_plane + NCLS;
  unsigned* h = lds + CURVE_HEAD;
  const int nlive = a.nlive, T1 = a.T + 1, cells = LDS_HIST ? ROWS * nlive * T1 : 0;
  const int tid = threadIdx.x;
  if (tid < THR_PAD) s_thr[tid] = tid < MAXT ? a.thr[tid & (MAXT - 1)] : INFINITY;      // (a.thr is +inf from entry T on)
  if (tid < NCLS) { s_plane[tid] = a.plane[tid]; s_cls[tid] = a.cls[tid]; }
  for (int j = threadIdx.x; j < cells; j += 256) h[j] = 0u;
  __syncthreads();

  // the pixel's cell in `hist` (-1: gt 255, not counted); with a workgroup histogram the count goes into it here
  auto count = [&](unsigned g, float m, int e) -> int {
    if (g == 255u) return -1;
    int k = 0;                                   // thresholds strictly below m: thr is non-decreasing and +inf beyond T
#pragma unroll
    for (int s = THR_PAD / 2; s >= 1; s >>= 1)
      if (s_thr[k + s - 1] < m) k += s;
    if (LDS_HIST) atomicAdd(&h[((int)gt_row(g) * nlive + e) * T1 + k], 1u);
    return ((int)gt_row(g) * NCLS + s_cls[e]) * T1 + k;
  };
  // without a workgroup histogram: the lanes of a wave that count into the same cell add once (neighbouring pixels mostly share a
  // cell, and one global address takes one atomic at a time).  Reached by every lane that is still in the loop; cell < 0: nothing to add.
  auto global_add = [&](int cell) {
    unsigned long long todo = __ballot(cell >= 0);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int c = __shfl(cell, leader);
      const unsigned long long same = __ballot(cell == c);
      if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[c], (unsigned long long)__popcll(same));
      todo &= ~same;
    }
  };
  const long step = (long)gridDim.x * 256, first = (long)blockIdx.x * 256 + threadIdx.x;
  const long nvec = vec ? n / 4 : 0;
  for (long q = first; q < nvec; q += step) {
    const unsigned gw = reinterpret_cast<const unsigned*>(gt)[q];
    float best[4] = {0.f, 0.f, 0.f, 0.f};
    int arg[4] = {0, 0, 0, 0};
    for (int e0 = 0; e0 < nlive; e0 += 4) {      // four planes' loads in flight before the first compare (an image has 1-3 classes)
      f32x4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int p = e0 + j < nlive ? s_plane[e0 + j] : -1;
        v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p >= 0) v[j] = *reinterpret_cast<const f32x4*>(planes + p * plane_stride + 4 * q);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = e0 + j;
        if (e >= nlive) break;
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (e == 0 || v[j][t] > best[t]) { best[t] = v[j][t]; arg[t] = e; }
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int cell = count((gw >> (8 * t)) & 255u, best[t], arg[t]);
      if (!LDS_HIST) global_add(cell);
    }
  }
  for (long i = nvec * 4 + first; i < n; i += step) {
    float best = 0.f;
    int arg = 0;
    for (int e = 0; e < nlive; ++e) {
      const int p = s_plane[e];
      const float v = p >= 0 ? planes[p * plane_stride + i] : 0.f;
      if (e == 0 || v > best) { best = v; arg = e; }
    }
    const int cell = count(gt[i], best, arg);
    if (!LDS_HIST) global_add(cell);
  }
  if (!LDS_HIST) return;
  __syncthreads();
  for (int j = threadIdx.x; j < cells; j += 256) {
    const unsigned v = h[j];
    if (!v) continue;
    const int re = j / T1, k = j - re * T1, row = re / nlive, e = re - row * nlive;
    atomicAdd(&hist[((long)row * NCLS + s_cls[e]) * T1 + k], (unsigned long long)v);
  }
}

int grid_for(long work, int per_thread) {
  const long b = (work + 256L * per_thread - 1) / (256L * per_thread);
  return (int)(b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b));
}

}  // namespace

extern "C" int wseg_eval_confusion(const unsigned char* pred, const unsigned char* gt, long n, unsigned long long* conf, void* stream) {
  WSEG_CHECK(pred && gt && conf, "eval_confusion: null pointer");
  WSEG_CHECK(n > 0 && n <= MAX_PIXELS, "eval_confusion: n=%ld outside [1, 2^40]", n);
  const int vec = ((uintptr_t)pred % 16 == 0 && (uintptr_t)gt % 16 == 0) ? 1 : 0;
  const int nwg = grid_for(vec ? n / 16 + 15 : n, vec ? 1 : 4);
  hipLaunchKernelGGL(eval_confusion_kernel, dim3(nwg), dim3(256), 0, (hipStream_t)stream, pred, gt, n, vec, conf);
  WSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int wseg_eval_curve(const float* planes, long plane_stride, int nplanes, const int* src, const unsigned char* gt, long n,
                               const float* thr, int T, unsigned long long* hist, void* stream) {
  WSEG_CHECK(src && gt && thr && hist, "eval_curve: null pointer");
  WSEG_CHECK(n > 0 && n <= MAX_PIXELS, "eval_curve: n=%ld outside [1, 2^40]", n);
  WSEG_CHECK(T >= 1 && T <= MAXT, "eval_curve: %d thresholds, outside [1, %d]", T, MAXT);
  WSEG_CHECK(nplanes >= 0, "eval_curve: nplanes=%d", nplanes);
  CurveArgs a;
  for (int i = 0; i < MAXT; ++i) a.thr[i] = INFINITY;
  for (int i = 0; i < T; ++i) {
    WSEG_CHECK(thr[i] == thr[i] && (i == 0 || thr[i] >= thr[i - 1]), "eval_curve: the thresholds must be non-decreasing (entry %d)", i);
    a.thr[i] = thr[i];
  }
  a.nlive = 0;
  a.T = T;
  bool absent = false, present = false;
  for (int c = 0; c < NCLS; ++c) {
    a.plane[c] = -1;
    a.cls[c] = 0;
    WSEG_CHECK(src[c] >= -1 && src[c] < nplanes, "eval_curve: src[%d]=%d outside [-1, %d)", c, src[c], nplanes);
    if (src[c] < 0 && absent) continue;           // only the first absent class can win
    (src[c] < 0 ? absent : present) = true;
    a.plane[a.nlive] = src[c];
    a.cls[a.nlive++] = c;
  }
  WSEG_CHECK(planes || !present, "eval_curve: class planes without a plane buffer");
  WSEG_CHECK(!present || nplanes == 1 || plane_stride >= n, "eval_curve: plane stride %ld below the %ld pixels of a plane", plane_stride, n);
  const int vec = ((!present || ((uintptr_t)planes % 16 == 0 && plane_stride % 4 == 0)) && (uintptr_t)gt % 4 == 0) ? 1 : 0;
  const int nwg = grid_for(vec ? n / 4 + 3 : n, vec ? 1 : 4);
  const size_t head = CURVE_HEAD * sizeof(unsigned), lds = head + (size_t)ROWS * a.nlive * (T + 1) * sizeof(unsigned);
  hipStream_t s = (hipStream_t)stream;
  if (lds <= LDS_LIMIT) hipLaunchKernelGGL(eval_curve_kernel<true>, dim3(nwg), dim3(256), lds, s, planes, plane_stride, a, gt, n, vec, hist);
  else hipLaunchKernelGGL(eval_curve_kernel<false>, dim3(nwg), dim3(256), head, s, planes, plane_stride, a, gt, n, vec, hist);
  WSEG_LAUNCH_CHECK();
  return 0;
}
