#!/usr/bin/env python
"""DeepLab-v1 training-loss timing at the experiment's shape (N = 10, stride-8 logits 56 x 56 -> labels 448 x 448, 21 classes, about 10 % of
the label pixels ignored).

Device time (events around `--reps` back-to-back calls, medians over `--iters` such windows, after a warm-up of every timed call) of the
HIP path (csrc/seg_loss.hip) forward, backward and both — per kernel launch sequence: forward = seg_ce_forward + seg_ce_finish, backward =
seg_ce_backward — for f32 and bf16 rows, against the reference's formulation in plain torch on the same device and the same values
(F.interpolate bilinear align_corners=True to [N, 21, 448, 448], F.cross_entropy ignore_index=255; forward + backward through autograd,
f32), with the peak device memory of both.  The two paths' losses and gradients are compared before anything is timed.  The bytes the HIP
kernels must move at least (forward: the coarse rows and the label bytes read, the lse plane written; backward: rows, labels and lse read,
the gradient rows written) give the bytes/s and the share of the HBM peak.

  python scripts/bench_seg_loss.py [--iters 20] [--reps 10] [--out profiles/r21_seg_loss.txt]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_aff_loss import HBM_PEAK, peak_mb, timed  # noqa: E402  (scripts/bench_aff_loss.py: the same timing windows)
from wseg_amd.seg_loss import seg_ce_rows, seg_ce_rows_backward  # noqa: E402

LD = 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--N", type=int, default=10)
    ap.add_argument("--coarse", type=int, default=56)
    ap.add_argument("--size", type=int, default=448)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_seg_loss.py measures on the GPU only"
    N, fh, fw, H, W, C = args.N, args.coarse, args.coarse, args.size, args.size, 21
    M = N * fh * fw
    g = torch.Generator().manual_seed(0)
    base = 4.0 * torch.randn(N, C, fh, fw, generator=g)
    label = torch.randint(0, C, (N, H, W), generator=g, dtype=torch.int64).to(torch.uint8)
    for n in range(N):                                            # about 10 % ignored: a band of rows and a band of columns per image
        y0, x0 = int(torch.randint(0, H - H // 20, (1,), generator=g)), int(torch.randint(0, W - W // 20, (1,), generator=g))
        label[n, y0:y0 + H // 20] = 255
        label[n, :, x0:x0 + W // 20] = 255
    ignored = float((label == 255).double().mean())
    label = label.cuda()
    label_long = label.long()
    full_mb = N * C * H * W * 4 / 2 ** 20

    def plain(x):
        """forward + backward of the reference's formulation; returns the loss and the gradient"""
        x = x.detach().requires_grad_()
        loss = F.cross_entropy(F.interpolate(x, (H, W), mode="bilinear", align_corners=True), label_long, ignore_index=255)
        loss.backward()
        return loss.detach(), x.grad

    lines = [f"DeepLab-v1 training loss, N={N} coarse {fh}x{fw} -> labels {H}x{W}, {C} classes, {100 * ignored:.1f} % of the pixels ignored; "
             f"device ms per call: median [min, max] of {args.iters} windows of {args.reps} calls",
             f"one full-size [N, {C}, H, W] f32 tensor: {full_mb:.1f} MB"]
    for dtype, name in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        rows = torch.zeros(M, LD)
        rows[:, :C] = base.permute(0, 2, 3, 1).reshape(M, C)
        rows = rows.to(dtype).cuda()
        nchw = rows[:, :C].float().view(N, fh, fw, C).permute(0, 3, 1, 2).contiguous()    # the same values for the plain path (f32)
        out4, ctx = seg_ce_rows(rows, LD, label, N, fh, fw, H, W, C)
        d = torch.empty(M, LD, device="cuda", dtype=dtype)
        seg_ce_rows_backward(ctx, out=d)
        p_loss, p_grad = plain(nchw)
        rel = abs(float(out4[0]) - float(p_loss)) / abs(float(p_loss))
        gdiff = float((d[:, :C].float().view(N, fh, fw, C).permute(0, 3, 1, 2) - p_grad).abs().max() / p_grad.abs().max())
        assert rel < 1e-5 and gdiff < (1e-4 if dtype == torch.float32 else 1e-2), (rel, gdiff)

        def fwd():
            return seg_ce_rows(rows, LD, label, N, fh, fw, H, W, C)

        def bwd():
            seg_ce_rows_backward(ctx, out=d)

        def both():
            seg_ce_rows_backward(fwd()[1], out=d)

        for fn in (fwd, bwd, both, lambda: plain(nchw)):                              # warm-up of every timed call
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {}
        for _round in range(2):                                                       # the two paths alternate: other work shares the host
            for k, fn in (("hip forward (seg_ce_forward + seg_ce_finish)", fwd), ("hip backward (seg_ce_backward)", bwd),
                          ("hip forward+backward", both), ("plain torch forward+backward (f32)", lambda: plain(nchw))):
                t.setdefault(k, []).append(timed(fn, args.iters, args.reps))
        t = {k: min(v) for k, v in t.items()}                                         # the round with the lower median, [min, max] of that round
        mem_hip, mem_plain = peak_mb(both), peak_mb(lambda: plain(nchw))
        esz = rows.element_size()
        min_bytes = {"hip forward (seg_ce_forward + seg_ce_finish)": M * C * esz + N * H * W * (1 + 4),
                     "hip backward (seg_ce_backward)": M * C * esz + N * H * W * (1 + 4) + M * LD * esz}
        lines.append(f"-- rows in {name} (gradient rows in {name}): loss hip {float(out4[0]):.6f} / plain {float(p_loss):.6f} (rel {rel:.1e}), "
                     f"gradient max diff / max {gdiff:.1e}")
        for k, (med, lo, hi) in t.items():
            extra = ""
            if k in min_bytes:
                extra = (f"   least traffic {min_bytes[k] / 1e6:.1f} MB -> {min_bytes[k] / (med * 1e-3) / 1e12:.3f} TB/s, "
                         f"{100 * min_bytes[k] / (med * 1e-3) / HBM_PEAK:.1f} % of the HBM peak")
            lines.append(f"   {k:46s} {med:8.3f} [{lo:.3f}, {hi:.3f}]{extra}")
        sp = t["plain torch forward+backward (f32)"][0] / t["hip forward+backward"][0]
        lines.append(f"   hip forward+backward is {sp:.1f}x {'faster' if sp > 1 else 'SLOWER'} than plain torch; peak device memory beyond the inputs: "
                     f"hip {mem_hip:.1f} MB ({'below' if mem_hip < full_mb else 'NOT below'} one full-size tensor), plain torch {mem_plain:.1f} MB")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
