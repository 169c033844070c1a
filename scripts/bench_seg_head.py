#!/usr/bin/env python
"""DeepLab-v1 head training path, timing at the experiment's shape (N = 10, 56 x 56 stride-8 map: 31360 pixel rows of 4096 -> 512 -> 512 -> 21
channels), per precision mode.

Device time (events around `--reps` back-to-back calls, medians over `--iters` such windows, after a warm-up of every timed call) of
  every launch of wseg_amd.seg_head on its own: the three forward convs, the six backward GEMMs (with the plan the library chose and the
    algorithmic TF/s), and the four kernels of csrc/seg_head.hip (with the bytes they must move at least, bytes/s and the share of the HBM peak);
  the head forward with context, the head backward, and both;
  the same chain in plain torch on the device (F.conv2d at dilation 12, F.batch_norm(training=True), relu, F.dropout, two 1x1 convs, autograd;
    NCHW, in the mode's storage dtype), forward + backward, with the peak device memory of both paths.
The HIP path's first BatchNorm-ReLU output is compared with plain torch's before anything is timed (behind it the dropout masks differ).

  python scripts/bench_seg_head.py [--iters 10] [--reps 5] [--out profiles/r22_seg_head.txt]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_aff_loss import HBM_PEAK, peak_mb, timed  # noqa: E402  (scripts/bench_aff_loss.py: the same timing windows)
from wseg_amd import _lib as L, arch, synth  # noqa: E402
from wseg_amd.deeplabv1_resnet38 import Net  # noqa: E402
from wseg_amd.engine import DT_OF, head_conv  # noqa: E402
from wseg_amd.seg_head import backward_launches, seg_head_backward, seg_head_forward  # noqa: E402

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "bf16x3": torch.float32}
FAMILY = {1: "64x128", 2: "128x128", 3: "224x256", 4: "256x256", 5: "512x128", 6: "wgrad 128x128", 7: "wgrad 256x256"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--N", type=int, default=10)
    ap.add_argument("--size", type=int, default=56)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_seg_head.py measures on the GPU only"
    N, h, w = args.N, args.size, args.size
    M, dims, DIL = N * h * w, [(args.size, args.size)], arch.SEG_HEAD_DILATION
    gen = torch.Generator(device="cuda").manual_seed(0)
    base = torch.relu(torch.randn(M, 4096, generator=gen, device="cuda"))
    d_rows = torch.zeros(M, 24, device="cuda")
    d_rows[:, :21] = torch.randn(M, 21, generator=gen, device="cuda") / M
    sd = synth.procedural_seg_state_dict(0)
    lines = [f"DeepLab-v1 head, training path, N={N} {h}x{w} ({M} rows; 4096 -> 512 (3x3, dilation {DIL}) -> 512 -> 21); device ms per call: "
             f"median [min, max] of {args.iters} windows of {args.reps} calls"]
    for mode in ("bf16", "fp32", "bf16x3"):
        tdt, dt = TDT[mode], DT_OF[mode]
        es = 2 if tdt == torch.bfloat16 else 4
        net = Net(precision=mode)
        net.load_state_dict(sd, strict=True)
        net.cuda().train()
        t = base.to(tdt)
        key = synth.dropout_key(0, 0)
        rows, ctx = seg_head_forward(net, t, N, h, w, key)
        eng = ctx["eng"]
        eng.attach_grads()
        eng.flat_g.zero_()
        cap = {}
        d_t = seg_head_backward(ctx, d_rows, capture=cap)
        P = eng.head_wt(t.device)

        # the same chain in plain torch, in the mode's storage dtype
        x0 = t.view(N, h, w, 4096).permute(0, 3, 1, 2).contiguous().requires_grad_()
        wts = [getattr(net, k).weight.detach().to(tdt).contiguous().requires_grad_() for k in ("conv_fov", "conv_fov2", "cls_conv")]
        bias = net.cls_conv.bias.detach().to(tdt).requires_grad_()
        bnp = [(b.weight.detach().clone().requires_grad_(), b.bias.detach().clone().requires_grad_(), b.running_mean.clone(), b.running_var.clone())
               for b in (net.bn_fov, net.bn_fov2)]
        g_nchw = d_rows[:, :21].reshape(N, h, w, 21).permute(0, 3, 1, 2).to(tdt).contiguous()
        keep = {}

        def plain():
            for v in [x0, bias] + wts + [q for b in bnp for q in b[:2]]:
                v.grad = None
            y = F.conv2d(x0, wts[0], None, 1, DIL, DIL)
            y = F.relu(F.batch_norm(y, bnp[0][2], bnp[0][3], bnp[0][0], bnp[0][1], True, 0.0003, 1e-5))
            keep["y1"] = y
            y = F.conv2d(y, wts[1])
            y = F.relu(F.batch_norm(y, bnp[1][2], bnp[1][3], bnp[1][0], bnp[1][1], True, 0.0003, 1e-5))
            out = F.conv2d(F.dropout(y, 0.5, True), wts[2], bias)
            out.backward(g_nchw)
            return out

        plain()
        y1p = keep["y1"].detach().permute(0, 2, 3, 1).reshape(M, 512).float()
        dev = float((ctx["y1"].float() - y1p).abs().max() / y1p.abs().max())
        assert dev < (5e-2 if mode == "bf16" else 1e-3), (mode, dev)
        keep.clear()

        launches = backward_launches(N, h, w, dt)
        fwd_conv = {name: head_conv(name, ci, co if co % 8 == 0 else arch.SEG_CLS_ROWS, dims, k=k, dil=DIL if k > 1 else 1)
                    for name, (co, ci, k) in arch.SEG_HEAD_CONVS.items()}
        cdt = L.F32X3 if dt == L.F32X3 else None
        z1, y1, z2, y2 = ctx["z1"], ctx["y1"], ctx["z2"], ctx["y2"]
        st1, st2 = ctx["stats1"], ctx["stats2"]
        tmp = torch.empty(M, 512, device="cuda", dtype=tdt)
        tmp4096 = torch.empty(M, 4096, device="cuda", dtype=tdt)
        rows_t = torch.empty(M, 24, device="cuda", dtype=tdt)
        ws = torch.empty(L.bn_stats_workspace_bytes(M, 512), device="cuda", dtype=torch.uint8)
        vec = torch.empty(8, 512, device="cuda")
        bias24 = eng._seg_train_bias
        gemm = {}       # name: (fn, plan, flops)

        def add_fwd(name, inp, out, **kw):
            c = fwd_conv[name]
            akw = dict(c.fwd_kw(N), dtype=cdt, **kw)
            args_ = (inp, P["w"][name], out, None) if not kw else (inp, P["w"][name], None, out)
            gemm["fwd " + name] = (lambda: L.conv_igemm(*args_, **akw), L.conv_plan(*args_, **akw), L._flops_label("fwd", **akw)[0])

        add_fwd("conv_fov", t, tmp)
        add_fwd("conv_fov2", y1, tmp)
        add_fwd("cls_conv", y2, rows_t, shift=bias24, relu_out2=0)
        srcs = {"cls_conv": (y2, cap["d_pad"]), "conv_fov2": (y1, cap["dz2"]), "conv_fov": (t, cap["dz1"])}
        for name in ("cls_conv", "conv_fov2", "conv_fov"):
            x, dy = srcs[name]
            wkw, dkw = launches["wgrad_" + name], launches["dgrad_" + name]
            dw = eng.grad_slice(name)
            out = tmp4096 if name == "conv_fov" else tmp
            gemm["wgrad " + name] = (lambda x=x, dy=dy, dw=dw, wkw=wkw: L.conv_wgrad(x, dy, dw, **wkw), L.wgrad_plan(x, dy, dw, **wkw),
                                     L._flops_label("wgrad", **wkw)[0])
            gemm["dgrad " + name] = (lambda dy=dy, wt=P["wt"][name], out=out, dkw=dkw: L.conv_igemm(dy, wt, out, None, **dkw),
                                     L.conv_plan(dy, P["wt"][name], out, None, **dkw), L._flops_label("dgrad", **dkw)[0])
        g512 = cap["d_y2"]
        kern = {        # name: (fn, least bytes)
            "bn_stats (reduce + finish)": (lambda: L.bn_stats(z1, 512, M, 512, net.bn_fov.weight.detach(), net.bn_fov.bias.detach(), 1e-5, 0.0003,
                                                              vec[0], vec[1], vec[2], vec[3], vec[4], vec[5], ws), M * 512 * es),
            "bn_relu_drop, no dropout": (lambda: L.bn_relu_drop(z1, 512, st1[2], st1[3], tmp, 512, M, 512, 0.0, key), 2 * M * 512 * es),
            "bn_relu_drop, p = 0.5": (lambda: L.bn_relu_drop(z2, 512, st2[2], st2[3], tmp, 512, M, 512, 0.5, key), 2 * M * 512 * es),
            "bn_relu_backward (reduce + finish + apply)": (lambda: L.bn_relu_backward(g512, 512, y2, 512, z2, 512, st2[0], st2[1], net.bn_fov2.weight.detach(),
                                                                                     2.0, tmp, 512, vec[6], vec[7], M, 512, ws), 7 * M * 512 * es),
            "col_sums of the [M][24] f32 gradient rows": (lambda: L.col_sums(d_rows, 24, M, 21, vec[0], ws), M * 24 * 4),
        }
        whole = {"hip forward with context": lambda: seg_head_forward(net, t, N, h, w, key),
                 "hip backward": lambda: seg_head_backward(ctx, d_rows),
                 "hip forward+backward": lambda: seg_head_backward(seg_head_forward(net, t, N, h, w, key)[1], d_rows),
                 "plain torch forward+backward": plain}
        for fn in [v[0] for v in gemm.values()] + [v[0] for v in kern.values()] + list(whole.values()):
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        lines.append(f"-- {mode}: max deviation of relu(bn_fov(conv_fov)) from plain torch, relative to its max: {dev:.1e}")
        for k, (fn, plan, flops) in gemm.items():
            med, lo, hi = timed(fn, args.iters, args.reps)
            lines.append(f"   {k:48s} {med:8.3f} [{lo:.3f}, {hi:.3f}]   {FAMILY.get(plan.family, plan.family)} tiles, {plan.nwg} workgroups"
                         f"{', nsplit %d' % plan.nsplit if plan.nsplit else ''}   {flops / 1e9:.1f} GFLOP -> {flops / (med * 1e-3) / 1e12:.1f} TF/s")
        for k, (fn, nbytes) in kern.items():
            med, lo, hi = timed(fn, args.iters, args.reps)
            lines.append(f"   {k:48s} {med:8.3f} [{lo:.3f}, {hi:.3f}]   least traffic {nbytes / 1e6:.1f} MB -> {nbytes / (med * 1e-3) / 1e12:.2f} TB/s, "
                         f"{100 * nbytes / (med * 1e-3) / HBM_PEAK:.0f} % of the HBM peak")
        tm = {k: timed(fn, args.iters, args.reps) for k, fn in whole.items()}
        for k, (med, lo, hi) in tm.items():
            lines.append(f"   {k:48s} {med:8.3f} [{lo:.3f}, {hi:.3f}]")
        mem_hip, mem_plain = peak_mb(whole["hip forward+backward"]), peak_mb(plain)
        sp = tm["plain torch forward+backward"][0] / tm["hip forward+backward"][0]
        lines.append(f"   hip forward+backward is {sp:.2f}x {'faster' if sp > 1 else 'SLOWER'} than plain torch; peak device memory beyond the inputs: "
                     f"hip {mem_hip:.0f} MB, plain torch {mem_plain:.0f} MB")
        del net, ctx, cap, x0, wts, bnp, gemm, kern, whole, P, eng, d_t, rows
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
