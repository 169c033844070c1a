// aff_head.hip — the ELU backward of the AffinityNet head (network/resnet38_aff.py:39-42: f8_3, f8_4, f8_5, f9 are F.elu(conv(.))) on pixel rows.
//
//   dz[m][c] = gscale * g[m][c] * (y[m][c] > 0 ? 1 : y[m][c] + 1)        c in [0, C)
//
// y is the saved ELU OUTPUT (elu'(z) = 1 for z > 0, exp(z) = y + 1 otherwise: no pre-activation is kept); g is the upstream gradient — f32 from
// aff_loss_backward, or the f9 data gradient in the engine's activation dtype — and the kernel is also the f32 -> bf16 cast of the loss gradient.
// Purely streaming: every thread moves 8 consecutive channels per step (16-byte loads and stores), grid-stride over the M * C / 8 chunks, no LDS,
// no atomics, plain vector stores.  A thread reads its chunk of g before it writes the same chunk of dz, so dz may alias g (same dtype and ld).
// Exact properties (tests/test_gpu_aff_head.py): y > 0 -> gscale * g rounded ONCE to dz's dtype; y == -1 -> exactly 0; y == 0 -> the y + 1 branch,
// derivative 1.
#include <algorithm>
#include "common.h"

namespace {

// p = RN_f32(gs * g) on its way to bf16: where p sits exactly on a bf16 tie although the exact product does not, step one f32 ulp towards the
// exact product, so that the bf16 rounding that follows is the single rounding of gs * g (the fma gives the product's residual exactly)
__device__ __forceinline__ float off_the_false_tie(float p, float gs, float g) {
  unsigned u = __float_as_uint(p);
  if ((u & 0xFFFFu) == 0x8000u) {
    const float err = __builtin_fmaf(gs, g, -p);
    if (err != 0.f) u = ((err > 0.f) == (p > 0.f)) ? u + 1u : u - 1u;
  }
  return __uint_as_float(u);
}

template <int GDT, int YDT, int ZDT>
__global__ __launch_bounds__(256) void elu_backward_rows_kernel(const void* g, int ld_g, const void* y, int ld_y, const float* __restrict__ gscale,
                                                                void* dz, int ld_dz, unsigned chunks, unsigned cpr) {
  const bool scaled = gscale != nullptr;
  const float gs = scaled ? gscale[0] : 1.f;
  const unsigned step = gridDim.x * 256u;
  for (unsigned long i = blockIdx.x * 256u + threadIdx.x; i < chunks; i += step) {
    const unsigned m = (unsigned)i / cpr, c = ((unsigned)i - m * cpr) * 8u;
    float a[8], b[8], o[8];
    load8<GDT>(g, (size_t)m * ld_g + c, a);
    load8<YDT>(y, (size_t)m * ld_y + c, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float p = scaled ? gs * a[e] : a[e];
      const float f = b[e] > 0.f ? 1.f : b[e] + 1.f;                  // elu' from the ELU output
      if (f == 1.f) {                                                 // (y > 0, and y == 0 through the other branch: gscale * g, rounded once)
        if (ZDT == WSEG_BF16 && GDT == WSEG_F32 && scaled) p = off_the_false_tie(p, gs, a[e]);
        o[e] = p;
      } else {
        o[e] = p * f;
      }
    }
    store8<ZDT>(dz, (size_t)m * ld_dz + c, o);
  }
}

bool rows_dtype(int dt) { return dt == WSEG_F32 || dt == WSEG_BF16; }

}  // namespace

extern "C" int wseg_elu_backward_rows(const void* g, int ld_g, int g_dtype, const void* y, int ld_y, int y_dtype, const float* gscale, void* dz,
                                      int ld_dz, int dz_dtype, long M, int C, void* stream) {
  WSEG_CHECK(rows_dtype(g_dtype) && rows_dtype(y_dtype) && rows_dtype(dz_dtype), "elu_backward_rows: bad dtype (g %d, y %d, dz %d): f32 (0) or bf16 (1)",
             g_dtype, y_dtype, dz_dtype);
  WSEG_CHECK(M > 0 && C > 0 && C % 8 == 0, "elu_backward_rows: M=%ld C=%d (M > 0, C > 0, C %% 8 == 0)", M, C);
  WSEG_CHECK(ld_g % 8 == 0 && ld_y % 8 == 0 && ld_dz % 8 == 0 && ld_g >= C && ld_y >= C && ld_dz >= C,
             "elu_backward_rows: ld_g=%d ld_y=%d ld_dz=%d (each %% 8 == 0 and >= C=%d)", ld_g, ld_y, ld_dz, C);
  WSEG_CHECK(g && y && dz, "elu_backward_rows: null pointer");
  WSEG_CHECK((uintptr_t)g % 16 == 0 && (uintptr_t)y % 16 == 0 && (uintptr_t)dz % 16 == 0, "elu_backward_rows: g, y and dz must be 16-byte aligned");
  WSEG_CHECK(g != dz || (g_dtype == dz_dtype && ld_g == ld_dz), "elu_backward_rows: dz may alias g only with the same dtype and ld");
  const long chunks = M * (long)(C / 8);
  WSEG_CHECK(chunks < (1L << 31), "elu_backward_rows: too many elements (M=%ld C=%d)", M, C);
  const unsigned blocks = (unsigned)std::min((chunks + 255) / 256, 256L * 8);      // at most 8 workgroups per CU; the loop strides over the rest
  hipStream_t s = (hipStream_t)stream;
  with_const<2>(g_dtype, [&](auto gd) {
    with_const<2>(y_dtype, [&](auto yd) {
      with_const<2>(dz_dtype, [&](auto zd) {
        hipLaunchKernelGGL((elu_backward_rows_kernel<decltype(gd)::value, decltype(yd)::value, decltype(zd)::value>), dim3(blocks), dim3(256), 0, s, g,
                           ld_g, y, ld_y, gscale, dz, ld_dz, (unsigned)chunks, (unsigned)(C / 8));
      });
    });
  });
  WSEG_LAUNCH_CHECK();
  return 0;
}
