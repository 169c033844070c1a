#!/usr/bin/env python
"""The AffinityNet training step (wseg_amd.aff_train.AffTrainer) at the reference's shape, N = 8 at crop 448 (56 x 56 maps), per precision
mode: device ms per step, its split by CUDA events into backbone forward (saved activations) / head + loss (ELU head forward, pair loss
forward and gradient) / head backward / trunk backward with the two taps / SGD, and the peak of torch's allocator.

The split runs the phases of AffTrainer.step with an event between them (same launches, same order; events cost ~10 us each); the whole step
is timed apart, without the inner events.  Medians over `--steps` steps after `--warmup`.

  python scripts/bench_aff_train.py [--steps 10] [--warmup 3] [--out profiles/r14_aff_train.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wseg_amd import aff_loss, aff_train, synth  # noqa: E402
from wseg_amd.engine import AFF_FEAT_C  # noqa: E402
from wseg_amd.resnet38_aff import Net  # noqa: E402

PHASES = ("backbone forward", "head + loss", "head backward", "trunk backward", "SGD")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--N", type=int, default=8)
    ap.add_argument("--crop", type=int, default=448)
    ap.add_argument("--modes", default="bf16,bf16x3,fp32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_aff_train.py measures on the GPU only"
    N, S = args.N, args.crop
    h = w = S // 8
    sd = synth.procedural_aff_state_dict(0)
    img = synth.synthetic_images(N, S, 5).cuda()
    label = torch.stack([synth.synthetic_aff_label_map(h, w, 10 + i, block=7) for i in range(N)]).cuda()
    lines = [f"AffinityNet training step (AffTrainer.step), N={N} at {S}x{S} ({h}x{w} maps, radius 5); device ms, median [min, max] of {args.steps} steps "
             f"after {args.warmup}"]
    for mode in args.modes.split(","):
        model = Net(precision=mode)
        model.load_state_dict(sd, strict=True)
        opt = aff_train.build_optimizer(model, 1e-5, 5e-4, 10 ** 6)
        model.cuda().train()
        tr = aff_train.AffTrainer(model, opt)
        torch.cuda.reset_peak_memory_stats()

        def split_step():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(PHASES) + 1)]
            ev[0].record()
            f9, (h_, w_, r), saved = model.train_forward(img)
            ev[1].record()
            opt.zero_grad()
            out7, lctx = aff_loss.aff_loss_rows(f9, AFF_FEAT_C, AFF_FEAT_C, label, N, h_, w_, r)
            d_f9 = aff_loss.aff_loss_rows_backward(lctx)
            ev[2].record()
            model.train_backward(saved, d_f9, between=ev[3].record)      # (the trainer's own call, with an event between its two phases)
            ev[4].record()
            opt.step()
            ev[5].record()
            return ev, out7

        def whole_step():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out7 = tr.step(img, label)
            e1.record()
            return (e0, e1), out7

        for _ in range(args.warmup):
            whole_step()
            split_step()
        torch.cuda.synchronize()
        whole = [whole_step() for _ in range(args.steps)]
        torch.cuda.synchronize()
        t_whole = [e0.elapsed_time(e1) for (e0, e1), _ in whole]
        peak = torch.cuda.max_memory_allocated() / 2 ** 30
        parts = [split_step() for _ in range(args.steps)]
        torch.cuda.synchronize()
        t_parts = [[ev[i].elapsed_time(ev[i + 1]) for ev, _ in parts] for i in range(len(PHASES))]
        out7 = whole[-1][1].tolist()
        assert all(v == v and abs(v) < 1e30 for v in out7), out7
        med = statistics.median(t_whole)
        lines.append(f"-- {mode}: {med:8.2f} [{min(t_whole):.2f}, {max(t_whole):.2f}] ms per step = {N / med * 1e3:.1f} images/s; "
                     f"peak allocated {peak:.2f} GiB; last scalars " + " ".join(f"{v:.4g}" for v in out7))
        for name, ts in zip(PHASES, t_parts):
            lines.append(f"   {name:18s} {statistics.median(ts):8.2f} [{min(ts):.2f}, {max(ts):.2f}]   {100 * statistics.median(ts) / sum(statistics.median(t) for t in t_parts):5.1f} %")
        del model, opt, tr, whole, parts
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
