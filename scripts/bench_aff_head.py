#!/usr/bin/env python
"""AffinityNet head timing at the training shape (N = 8, 56 x 56 feature map: 25088 pixel rows), per precision mode.

Device time (CUDA events around `--reps` back-to-back calls, medians over `--iters` such windows, after a warm-up of every timed call) of
  the head forward with context (Engine.run_aff_head: four ELU GEMM launches),
  the head backward (wseg_amd/aff_head.py), and of it the two ELU-backward launches (csrc/aff_head.hip) alone — the GEMM launches are the rest,
  the same head in plain torch on the device (F.conv2d + F.elu under autograd, NCHW, in the mode's storage dtype), forward + backward,
and the achieved bytes/s of the ELU-backward kernel (g and y read once, dz written once) against torch.where(y > 0, g, g * (y + 1)).
The HIP path's results are compared with the plain-torch ones before anything is timed.

  python scripts/bench_aff_head.py [--iters 20] [--reps 10] [--out profiles/r10_aff_head.txt]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_aff_loss import HBM_PEAK, timed  # noqa: E402  (scripts/bench_aff_loss.py: the same timing windows)
from wseg_amd import _lib as L, synth  # noqa: E402
from wseg_amd.aff_head import aff_head_backward, aff_head_forward  # noqa: E402
from wseg_amd.resnet38_aff import Net  # noqa: E402

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "bf16x3": torch.float32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--N", type=int, default=8)
    ap.add_argument("--size", type=int, default=56)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_aff_head.py measures on the GPU only"
    N, h, w, C = args.N, args.size, args.size, 448
    M = N * h * w
    gen = torch.Generator(device="cuda").manual_seed(0)
    base = [torch.randn(M, c, generator=gen, device="cuda") for c in (512, 1024, 4096)]
    base[2] = torch.relu(base[2])
    d_f9 = torch.randn(M, C, generator=gen, device="cuda") * 1e-3
    sd = synth.procedural_aff_state_dict(0)
    lines = [f"AffinityNet head, N={N} {h}x{w} ({M} rows; conv4 512 / conv5 1024 / conv6 4096 -> 448 -> 448 channels); device ms per call: "
             f"median [min, max] of {args.iters} windows of {args.reps} calls"]
    for mode in ("bf16", "fp32", "bf16x3"):
        tdt = TDT[mode]
        net = Net(precision=mode)
        net.load_state_dict(sd, strict=True)
        net.cuda()
        c4, c5, t = (x.to(tdt) for x in base)
        f9, ctx = aff_head_forward(net, c4, c5, t, N, h, w)
        eng = ctx["eng"]
        eng.attach_grads()
        eng.flat_g.zero_()
        ds = aff_head_backward(ctx, d_f9)

        # the same head in plain torch, in the mode's storage dtype
        nchw = [x.view(N, h, w, -1).permute(0, 3, 1, 2).contiguous().requires_grad_() for x in (c4, c5, t)]
        wts = [getattr(net, k).weight.detach().to(tdt).contiguous().requires_grad_() for k in ("f8_3", "f8_4", "f8_5", "f9")]
        g_nchw = d_f9.view(N, h, w, C).permute(0, 3, 1, 2).to(tdt).contiguous()

        def plain():
            for v in nchw + wts:
                v.grad = None
            feat = torch.cat([F.elu(F.conv2d(x, wt)) for x, wt in zip(nchw, wts[:3])], dim=1)
            out = F.elu(F.conv2d(feat, wts[3]))
            out.backward(g_nchw)
            return out

        out = plain()
        rel = lambda a, b: float((a.float() - b.float()).abs().max() / b.float().abs().max())
        dev = [rel(f9, out.detach().permute(0, 2, 3, 1).reshape(M, C))]
        dev += [rel(d, x.grad.permute(0, 2, 3, 1).reshape(M, -1)) for d, x in zip(ds, nchw)]
        dev += [rel(eng.grad_slice(k).view(wt.shape[0], -1), wt.grad.reshape(wt.shape[0], -1)) for k, wt in zip(("f8_3", "f8_4", "f8_5", "f9"), wts)]
        tol = 5e-2 if mode == "bf16" else 1e-3
        assert max(dev) < tol, (mode, dev)

        dz9, dzf = torch.empty(M, C, device="cuda", dtype=tdt), torch.empty(M, C, device="cuda", dtype=tdt)
        d_feat = torch.randn(M, C, generator=gen, device="cuda").to(tdt)

        def elu_two():                                        # the backward's two ELU launches: f32 loss gradient -> dz9, d_feat -> dzf
            L.elu_backward_rows(d_f9, C, ctx["f9"], C, None, dz9, C, M, C)
            L.elu_backward_rows(d_feat, C, ctx["feat"], C, None, dzf, C, M, C)

        def elu_one():
            L.elu_backward_rows(d_feat, C, ctx["feat"], C, None, dzf, C, M, C)

        y, g = ctx["feat"], d_feat

        def where_one():
            return torch.where(y > 0, g, g * (y + 1))

        calls = (("hip forward with context", lambda: aff_head_forward(net, c4, c5, t, N, h, w)),
                 ("hip backward", lambda: aff_head_backward(ctx, d_f9)),
                 ("  of it: the two ELU-backward launches", elu_two),
                 ("plain torch forward+backward", plain),
                 ("ELU backward, one launch (g, y, dz in the mode's dtype)", elu_one),
                 ("torch.where(y > 0, g, g * (y + 1))", where_one))
        for _, fn in calls:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        tm = {k: timed(fn, args.iters, args.reps) for k, fn in calls}
        lines.append(f"-- {mode}: max relative deviation from plain torch (f9, d_conv4, d_conv5, d_t, dW f8_3, f8_4, f8_5, f9): " + ", ".join(f"{v:.1e}" for v in dev))
        nbytes = 3 * M * C * y.element_size()
        for k, (med, lo, hi) in tm.items():
            extra = ""
            if "ELU backward, one" in k or "torch.where" in k:
                extra = f"   {nbytes / 1e6:.1f} MB -> {nbytes / (med * 1e-3) / 1e12:.2f} TB/s, {100 * nbytes / (med * 1e-3) / HBM_PEAK:.0f} % of the HBM peak"
            lines.append(f"   {k:58s} {med:8.3f} [{lo:.3f}, {hi:.3f}]{extra}")
        gemm = tm["hip backward"][0] - tm["  of it: the two ELU-backward launches"][0]
        both = tm["hip forward with context"][0] + tm["hip backward"][0]
        sp = tm["plain torch forward+backward"][0] / both
        lines.append(f"   backward GEMM launches (backward minus the ELU launches) {gemm:.3f}; hip forward+backward {both:.3f} is {sp:.2f}x "
                     f"{'faster' if sp > 1 else 'SLOWER'} than plain torch")
        del net, ctx, nchw, wts
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
