// conv_wgrad.hip — the C entry points of the convolution weight gradient; the kernels and the host-side plan live in conv_wgrad_kernels.h
// (shared with conv_igemm.hip, whose wseg_conv_bwd_pair launches the data-gradient and the weight-gradient tiles of a layer as one grid).
#include "conv_wgrad_kernels.h"

using namespace wseg_wg;

extern "C" int wseg_wgrad_plan(const wseg_wgrad_desc* d, wseg_launch_plan* out) {
  Plan pl;
  WSEG_CHECK(out, "wgrad_plan: null output");
  if (int rc = wgrad_plan(d, pl)) return rc;
  wgrad_plan_report(pl, out);
  return 0;
}

extern "C" int wseg_conv_wgrad(const wseg_wgrad_desc* d, void* stream) {
  Plan pl;
  if (int rc = wgrad_plan(d, pl)) return rc;
  const Args& a = pl.a;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(a.nwg);
  if (pl.pipe)
    with_const<2>(pl.unit, [&](auto unit) { hipLaunchKernelGGL((conv_wgrad_pipe_kernel<decltype(unit)::value>), grid, dim3(512), 0, s, a); });
  else
    with_const<3>(d->dtype, [&](auto dt) { hipLaunchKernelGGL((conv_wgrad_kernel<decltype(dt)::value, 128, 128, 2, 2>), grid, dim3(256), 0, s, a); });
  WSEG_LAUNCH_CHECK();
  return 0;
}
