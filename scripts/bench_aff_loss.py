#!/usr/bin/env python
"""AffinityNet training-loss timing at the training shape (N = 8, 56 x 56 feature map, 448 channels, radius 5: 34 offsets, 2496 from pixels).

Device time (CUDA events around `--reps` back-to-back calls, medians over `--iters` such windows, after a warm-up of every timed call) of
the HIP path (csrc/aff_loss.hip) forward, backward and both, in f32 and bf16, against the reference's formulation in plain torch on the
same device and the same values (two index_select gathers of [N, 448, 34 * 2496], three float label tensors; forward + backward through
autograd, f32), with the peak device memory of both.  The two paths' losses are compared before anything is timed.  The bytes the HIP
kernels must move at least (every feature row once per direction, the gradient rows once) give the share of the HBM peak.

  python scripts/bench_aff_loss.py [--iters 20] [--reps 10] [--out profiles/r09_aff_loss.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wseg_amd import synth  # noqa: E402
from wseg_amd.aff_loss import aff_loss_rows, aff_loss_rows_backward, pair_labels  # noqa: E402
from wseg_amd.resnet38_aff import indices_of_pairs, pair_offsets  # noqa: E402

HBM_PEAK = 8.0e12            # bytes / s (MI355X)


def timed(fn, iters, reps):
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / reps)
    return statistics.median(ts), min(ts), max(ts)


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--N", type=int, default=8)
    ap.add_argument("--size", type=int, default=56)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_aff_loss.py measures on the GPU only"
    N, h, w, C, r = args.N, args.size, args.size, 448, 5
    P = len(pair_offsets(r))
    M = N * h * w
    base = F.elu(torch.randn(N, C, h, w, generator=torch.Generator().manual_seed(0))).cuda()
    maps = torch.stack([synth.synthetic_aff_label_map(h, w, i) for i in range(N)])
    label = maps.cuda()
    labels = [torch.from_numpy(np.stack([pair_labels(m, r)[j] for m in maps.numpy()])).cuda() for j in range(3)]
    ind_from, ind_to = (torch.from_numpy(a).cuda() for a in indices_of_pairs(r, (h, w)))

    def plain(x):
        """forward + backward of the reference's formulation; returns the loss"""
        x = x.detach().requires_grad_()
        v = x.view(N, C, -1)
        ff = torch.index_select(v, 2, ind_from).unsqueeze(2)
        ft = torch.index_select(v, 2, ind_to).view(N, C, P, -1)
        aff = torch.exp(-torch.mean(torch.abs(ft - ff), dim=1))
        cnt = [lab.sum() + 1e-5 for lab in labels]
        parts = [(labels[0] * -torch.log(aff + 1e-5)).sum() / cnt[0], (labels[1] * -torch.log(aff + 1e-5)).sum() / cnt[1],
                 (labels[2] * -torch.log((1. + 1e-5) - aff)).sum() / cnt[2]]
        loss = parts[0] / 4 + parts[1] / 4 + parts[2] / 2
        loss.backward()
        return loss.detach(), x.grad

    lines = [f"AffinityNet training loss, N={N} {h}x{w} C={C} radius {r} (P={P}, {N * (h - r + 1) * (w - 2 * r + 2)} from pixels); "
             f"device ms per call: median [min, max] of {args.iters} windows of {args.reps} calls"]
    for dtype, name in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        rows = base.permute(0, 2, 3, 1).reshape(M, C).to(dtype).contiguous()
        nchw = rows.float().view(N, h, w, C).permute(0, 3, 1, 2).contiguous()          # the same values for the plain path (f32)
        out7, ctx = aff_loss_rows(rows, C, C, label, N, h, w, r)
        d = torch.empty(M, C, device="cuda")
        aff_loss_rows_backward(ctx, out=d)
        p_loss, p_grad = plain(nchw)
        rel = abs(float(out7[0]) - float(p_loss)) / abs(float(p_loss))
        gdiff = float((d.view(N, h, w, C).permute(0, 3, 1, 2) - p_grad).abs().max() / p_grad.abs().max())
        assert rel < 1e-5 and gdiff < 1e-4, (rel, gdiff)

        def fwd():
            return aff_loss_rows(rows, C, C, label, N, h, w, r)

        def bwd():
            aff_loss_rows_backward(ctx, out=d)

        def both():
            aff_loss_rows_backward(fwd()[1], out=d)

        for fn in (fwd, bwd, both, lambda: plain(nchw)):                              # warm-up of every timed call
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {k: timed(fn, args.iters, args.reps) for k, fn in (("hip forward", fwd), ("hip backward", bwd), ("hip forward+backward", both),
                                                               ("plain torch forward+backward (f32)", lambda: plain(nchw)))}
        mem_hip, mem_plain = peak_mb(both), peak_mb(lambda: plain(nchw))
        esz = rows.element_size()
        min_bytes = {"hip forward": M * C * esz, "hip backward": M * C * esz + M * C * 4}
        lines.append(f"-- features in {name}: loss hip {float(out7[0]):.6f} / plain {float(p_loss):.6f} (rel {rel:.1e}), gradient max diff / max {gdiff:.1e}")
        for k, (med, lo, hi) in t.items():
            extra = ""
            if k in min_bytes:
                extra = f"   least traffic {min_bytes[k] / 1e6:.1f} MB -> {min_bytes[k] / (med * 1e-3) / 1e12:.2f} TB/s, {100 * min_bytes[k] / (med * 1e-3) / HBM_PEAK:.0f} % of the HBM peak"
            lines.append(f"   {k:38s} {med:8.3f} [{lo:.3f}, {hi:.3f}]{extra}")
        sp = t["plain torch forward+backward (f32)"][0] / t["hip forward+backward"][0]
        lines.append(f"   hip forward+backward is {sp:.1f}x {'faster' if sp > 1 else 'SLOWER'} than plain torch; peak device memory beyond the inputs: "
                     f"hip {mem_hip:.1f} MB, plain torch {mem_plain:.1f} MB")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
