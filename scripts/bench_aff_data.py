#!/usr/bin/env python
"""AffinityNet training data: the device path (wseg_amd/aff_data.py DeviceAffData) beside the host chain (wseg_amd/data.py
aff_apply_transforms) at the training shape: N = 8 images of 375 x 500, crop 448, three present planes (background and two classes) in each
of the two CRF score stacks.

Reports
  - device time per batch (HIP events around `--reps` back-to-back calls, medians over `--iters` such windows, after a warm-up): the
    kernels alone (9 launches for the image, 1 for the labels), the label kernel alone, and the whole call with its host-to-device copies
    from page-locked blobs (as a DataLoader with pin_memory=True hands them over) and the host work of filling the descriptors;
  - the host chain's time per image on one core of the same box (decoded arrays in, tensors out: no file reads on either side);
  - the bytes shipped sparse against the bytes the host chain reads (image + two dense float32 [21, H, W] stacks);
  - the label kernel's achieved bytes/s over the bytes it must read (the pasted rectangle of every shipped plane) beside the 6.29 TB/s
    copy rate measured on this GPU.  The repeats re-read the same blobs, which fit the 256 MB last-level cache: the rate is no HBM rate, and at
    this size the launch sets the time as much as the memory system.
The device outputs are compared with the host chain's (image bit for bit; label outside float32 near-ties) before anything is timed.

  python scripts/bench_aff_data.py [--iters 20] [--reps 10] [--out profiles/r13_aff_data.txt]
"""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np
import PIL.Image
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wseg_amd import aff_data as D, data as wdata  # noqa: E402
from wseg_amd.resnet38_contrast import Normalize  # noqa: E402

COPY_RATE = 6.29e12          # bytes / s, the measured device copy rate (MI355X)


def smooth(rng, h, w, c, step):
    low = rng.normal(0, 2.0, (c, h // step + 2, w // step + 2)).astype(np.float32)
    return np.stack([np.asarray(PIL.Image.fromarray(p).resize((w, h), PIL.Image.Resampling.BICUBIC)) for p in low])


def make_inputs(n, h, w, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        img = np.clip(smooth(rng, h, w, 3, 8).transpose(1, 2, 0) * 40 + 128, 0, 255).astype(np.uint8)
        classes = (0, 1 + (5 * i) % 20, 1 + (5 * i + 9) % 20)
        stacks = []
        for shift in (1.0, -1.0):                            # low alpha: more background; high alpha: less
            logits = smooth(rng, h, w, 3, 40)
            logits[0] += shift
            e = np.exp(logits - logits.max(axis=0))
            s = np.zeros((21, h, w), np.float32)
            s[list(classes)] = e / e.sum(axis=0)
            stacks.append(s)
        out.append((img, stacks[0], stacks[1]))
    return out


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--N", type=int, default=8)
    ap.add_argument("--crop", type=int, default=448)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_aff_data.py measures on the GPU only"
    N, crop, H, W = args.N, args.crop, 375, 500
    inputs = make_inputs(N, H, W, 0)
    model_stub = type("M", (), {"normalize": Normalize()})()
    transforms = wdata.aff_train_transform(model_stub, crop)

    # the same draws for both paths
    samples, host = [], []
    for i, (img, la, ha) in enumerate(inputs):
        random.seed(100 + i)
        host.append(wdata.aff_apply_transforms(PIL.Image.fromarray(img), la, ha, transforms))
        random.seed(100 + i)
        samples.append(D.make_aff_sample("b%d" % i, img, la, ha, crop))
    batch = D.aff_collate(samples)
    for k in ("img", "planes", "ids"):
        batch[k] = batch[k].pin_memory()
    dad = D.DeviceAffData("cuda", crop)
    d_img, d_label = dad(batch)
    torch.cuda.synchronize()
    same_img = all(np.array_equal(d_img[i].cpu().numpy(), host[i][0]) for i in range(N))
    diff = sum(int((d_label[i].cpu().numpy() != host[i][1]).sum()) for i in range(N))
    assert same_img, "the device image differs from the host chain's"
    assert diff <= 0.001 * d_label.numel(), f"{diff} label cells differ from the host chain's"

    def full():
        dad(batch)

    def kernels():
        dad.launch_last()

    def label_kernel():
        dad.launch_last(image=False)

    for fn in (full, kernels, label_kernel):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t_full, t_k, t_lab = (timed(fn, args.iters, args.reps) for fn in (full, kernels, label_kernel))

    torch.set_num_threads(1)
    t0 = time.perf_counter()
    rounds = 3
    for _ in range(rounds):
        for img, la, ha in inputs:
            wdata.aff_apply_transforms(PIL.Image.fromarray(img), la, ha, transforms)
    t_host = (time.perf_counter() - t0) / (rounds * N)
    t0 = time.perf_counter()
    for _ in range(rounds):
        D.aff_collate([D.make_aff_sample("b%d" % i, img, la, ha, crop) for i, (img, la, ha) in enumerate(inputs)])
    t_pack = (time.perf_counter() - t0) / (rounds * N)

    shipped, dense = D.dense_bytes(batch)
    lab_bytes = sum(sum(p["np"]) * p["ch"] * p["cw"] * 4 for p in batch["params"]) + d_label.numel()
    lines = [f"AffinityNet training data, N={N} sources {H}x{W} crop {crop}, planes shipped per stack {[p['np'] for p in batch['params']][0]}; "
             f"device ms per batch: median [min, max] of {args.iters} windows of {args.reps} calls",
             f"   device image == host chain bit for bit: {same_img}; label cells differing from the host chain (float32 near-ties): {diff} of {d_label.numel()}",
             f"   kernels only (image 9 launches + labels 1)     {t_k[0]:8.3f} [{t_k[1]:.3f}, {t_k[2]:.3f}]",
             f"   label kernel alone                             {t_lab[0]:8.3f} [{t_lab[1]:.3f}, {t_lab[2]:.3f}]   reads {lab_bytes / 1e6:.1f} MB -> "
             f"{lab_bytes / (t_lab[0] * 1e-3) / 1e12:.3f} TB/s beside the {COPY_RATE / 1e12:.2f} TB/s copy rate ({100 * lab_bytes / (t_lab[0] * 1e-3) / COPY_RATE:.1f} %); "
             f"the repeats re-read the same blobs, which fit the last-level cache: no HBM rate",
             f"   whole call (descriptors, H2D copies, kernels)  {t_full[0]:8.3f} [{t_full[1]:.3f}, {t_full[2]:.3f}]",
             f"   host chain, one core: {t_host * 1e3:.1f} ms per image = {t_host * N * 1e3:.0f} ms per batch of {N} (decoded arrays in; no file reads)",
             f"   what stays on the host for the device path (draws, sparse packing, collate), one core: {t_pack * 1e3:.1f} ms per image",
             f"   bytes per batch: shipped sparse {shipped / 1e6:.1f} MB, dense (image + two float32 [21, H, W] stacks) {dense / 1e6:.1f} MB: {dense / shipped:.1f}x fewer"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
