#!/usr/bin/env python
"""DeepLab-v1 training data: the device path (wseg_amd/seg_data.py DeviceSegData) beside the host chain (wseg_amd/data.py
seg_apply_transforms) at the training shape of experiment/SEAM_deeplabv1_resnet38/config.py: N = 10 images of 375 x 500, crop 448, scale
drawn from [0.5, 1.5], H/S/V offsets from [-10, 10], flip 0.5.

Reports
  - device time per launch (HIP events around `--reps` back-to-back launches, medians over `--iters` such windows, after a warm-up): the HSV
    launch, the two resize passes, the finish launch; the four launches together; and the whole call with its host-to-device copies from
    page-locked blobs (as a DataLoader with pin_memory=True hands them over) and the host work of filling and checking the descriptors;
  - the finish launch's bytes per second over the bytes it must move (the pasted rectangle of the rescaled image and of the label read, the
    float32 planes and the label map written) beside the 6.29 TB/s copy rate measured on this GPU.  The repeats rewrite the same 24 MB, which
    fit the last-level cache: no HBM rate;
  - the host chain's time per image on one core of the same box (decoded arrays in, arrays out: no file reads on either side), and what
    stays on the host for the device path (draws, coefficient and index tables, collate);
  - the largest channel difference of the HSV round trip at zero offsets over all 2^24 colours (the figure tests/test_seg_data_host.py
    holds to its derived bound).
Both device outputs are compared with the host chain's bit for bit before anything is timed.

  python scripts/bench_seg_data.py [--iters 20] [--reps 10] [--out profiles/r24_seg_data.txt]
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

from wseg_amd import data as wdata, seg_data as D  # noqa: E402

COPY_RATE = 6.29e12          # bytes / s, the measured device copy rate (MI355X)


def make_inputs(n, h, w, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        low = rng.normal(0, 2.0, (3, h // 8 + 2, w // 8 + 2)).astype(np.float32)
        planes = np.stack([np.asarray(PIL.Image.fromarray(p).resize((w, h), PIL.Image.Resampling.BICUBIC)) for p in low])
        img = np.clip(planes.transpose(1, 2, 0) * 40 + 128, 0, 255).astype(np.uint8)
        seeds = rng.integers(0, 22, (h // 40 + 2, w // 40 + 2))
        lab = np.array(list(range(21)) + [255], np.uint8)[np.kron(seeds, np.ones((40, 40), np.int64))[:h, :w]]
        out.append((img, lab))
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
    ap.add_argument("--N", type=int, default=10)
    ap.add_argument("--crop", type=int, default=448)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_seg_data.py measures on the GPU only"
    N, crop, H, W = args.N, args.crop, 375, 500
    inputs = make_inputs(N, H, W, 0)

    # the same draws for both paths
    samples, host = [], []
    for i, (img, lab) in enumerate(inputs):
        host.append(wdata.seg_apply_transforms(img, lab, wdata.seg_train_transform(crop, rng=random.Random(100 + i))))
        samples.append(D.make_seg_sample("b%d" % i, img, lab, crop, rng=random.Random(100 + i)))
    batch = D.seg_collate(samples)
    for k in ("u8", "tab"):
        batch[k] = batch[k].pin_memory()
    dsd = D.DeviceSegData("cuda", crop)
    d_img, d_label = dsd(batch)
    torch.cuda.synchronize()
    same_img = all(np.array_equal(d_img[i].cpu().numpy().view(np.int32), host[i][0].view(np.int32)) for i in range(N))
    same_lab = all(np.array_equal(d_label[i].cpu().numpy(), host[i][1]) for i in range(N))
    assert same_img and same_lab, "the device outputs differ from the host chain's"

    fns = dict(full=lambda: dsd(batch), kernels=lambda: dsd.launch_last(), hsv=lambda: dsd.launch_last(D.HSV),
               resize=lambda: dsd.launch_last(D.RESIZE), finish=lambda: dsd.launch_last(D.FINISH))
    for name in ("kernels", "hsv", "resize", "finish", "full"):        # (`full` last: it replaces what launch_last repeats — same batch)
        for _ in range(3):
            fns[name]()
    torch.cuda.synchronize()
    t = {name: timed(fns[name], args.iters, args.reps) for name in ("kernels", "hsv", "resize", "finish", "full")}

    torch.set_num_threads(1)
    rounds = 3
    t0 = time.perf_counter()
    for r in range(rounds):
        for i, (img, lab) in enumerate(inputs):
            wdata.seg_apply_transforms(img, lab, wdata.seg_train_transform(crop, rng=random.Random(100 + i)))
    t_host = (time.perf_counter() - t0) / (rounds * N)
    t0 = time.perf_counter()
    for r in range(rounds):
        D.seg_collate([D.make_seg_sample("b%d" % i, img, lab, crop, rng=random.Random(100 + i)) for i, (img, lab) in enumerate(inputs)])
    t_pack = (time.perf_counter() - t0) / (rounds * N)

    rgb = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([(rgb >> 16) & 255, (rgb >> 8) & 255, rgb & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    trip = int(np.abs(wdata.hsv_jitter(rgb, 0, 0, 0).astype(np.int32) - rgb).max())
    dev_trip = int((dsd.hsv(rgb).cpu().numpy().astype(np.int32) - rgb).__abs__().max())

    params = batch["params"]
    fin_bytes = sum(p["ch"] * p["cw"] * 4 for p in params) + N * crop * crop * 13          # 3 image bytes + 1 label byte in; 12 + 1 bytes out
    px = dict(hsv=sum(p["H"] * p["W"] for p in params), resize=sum(p["H"] * p["rw"] + p["rh"] * p["rw"] for p in params))
    shipped = sum(batch[k].numel() * batch[k].element_size() for k in ("u8", "tab"))
    row = lambda name, label: f"   {label:<52}{t[name][0]:8.3f} [{t[name][1]:.3f}, {t[name][2]:.3f}]"
    rate = fin_bytes / (t["finish"][0] * 1e-3)
    lines = [f"DeepLab-v1 training data, N={N} sources {H}x{W} crop {crop}, scales {[round(p['scale'], 2) for p in params]}, "
             f"flips {[p['flip'] for p in params]}; device ms per batch: median [min, max] of {args.iters} windows of {args.reps} calls",
             f"   device image and label == host chain bit for bit: {same_img and same_lab}",
             f"   kernels per batch: 4 launches (hsv, resize horizontal, resize vertical, finish), each over the whole batch",
             row("hsv", f"hsv launch ({px['hsv'] / 1e6:.2f} Mpixel)"),
             row("resize", f"two resize passes ({px['resize'] / 1e6:.2f} Mpixel written)"),
             row("finish", "finish launch (image + label)") + f"   moves {fin_bytes / 1e6:.1f} MB -> {rate / 1e12:.3f} TB/s beside the "
             f"{COPY_RATE / 1e12:.2f} TB/s copy rate ({100 * rate / COPY_RATE:.1f} %); the repeats rewrite the same buffers, which fit the last-level cache: no HBM rate",
             row("kernels", "the four launches together"),
             row("full", "whole call (checks, descriptors, H2D copies, kernels)") + f"   ships {shipped / 1e6:.1f} MB",
             f"   host chain, one core: {t_host * 1e3:.1f} ms per image = {t_host * N * 1e3:.0f} ms per batch of {N} (decoded arrays in; no file reads)",
             f"   what stays on the host for the device path (draws, coefficient and index tables, collate), one core: {t_pack * 1e3:.2f} ms per image",
             f"   HSV round trip at zero offsets over all 2^24 colours, max |channel difference|: host {trip}, device {dev_trip} "
             f"(bound derived from the quantisation steps in tests/test_seg_data_host.py: 6)"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
