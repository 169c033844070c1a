"""Dense CRF at 375 x 500, (sxy 80, srgb 13), t = 10: ms per image for S = 1 and S = 2 label sets, the split into normalisation /
bilateral filter / Gaussian filter / update, pair evaluations per second, and the one baseline the kernel has to beat: the same exact
computation in plain torch on the same device (chunked f32 exp(-cdist^2 / 2) @ Q — what a user would write without the kernel).
HIP and torch runs alternate; medians and the spread (min .. max) of every series are printed.

    python scripts/bench_crf.py [--reps 5] [--torch_chunk 2048] [--cli_images 6] > profiles/r05_crf.txt
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wseg_amd import _lib as L          # noqa: E402
from wseg_amd import crf, synth         # noqa: E402


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def fmt(ts):
    return f"median {statistics.median(ts):9.3f} ms  (min {min(ts):9.3f}, max {max(ts):9.3f}, n={len(ts)})"


def torch_filter(f, X, chunk, mode):
    """K @ X, K = exp(-|fi - fj|^2 / 2) in f32, rows in chunks (the [chunk, N] block is all that is ever held).  mode "cdist": torch.cdist
    on differences (not the cancelling matrix-product expansion); mode "diff": the squared differences summed feature by feature."""
    out = torch.empty_like(X)
    for s in range(0, f.shape[0], chunk):
        if mode == "cdist":
            d = torch.cdist(f[s:s + chunk], f, compute_mode="donot_use_mm_for_euclid_dist")
            d2 = d * d
        else:
            d2 = (f[s:s + chunk, 0, None] - f[None, :, 0]) ** 2
            for k in range(1, f.shape[1]):
                d2 += (f[s:s + chunk, k, None] - f[None, :, k]) ** 2
        out[s:s + chunk] = torch.exp(-0.5 * d2) @ X
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch_chunk", type=int, default=2048)       # [chunk, N] f32 stays under 2 GiB
    ap.add_argument("--cli_images", type=int, default=6)
    a = ap.parse_args()
    H, W, sxy, srgb = 375, 500, 80.0, 13.0
    N = H * W
    img = synth.synthetic_rgb_image(H, W, 9).cuda()
    cams = synth.synthetic_cam_dict(H, W, [3, 11, 14], 9)
    labs = crf.labels_from_cams(cams, alpha=(4, 32))
    print(f"device {torch.cuda.get_device_name(0)}; image {H}x{W} (N = {N}, N^2 = {N * N:.3e} pairs per application), bilateral ({sxy:g}, {srgb:g}), t = 10")

    # ---- whole inference, S = 1 / S = 2, alternating
    runs = {1: [], 2: []}
    for S in (1, 2):
        crf.crf_inference(img, labs[:S])
    for _ in range(a.reps):
        for S in (1, 2):
            runs[S] += timed(lambda: crf.crf_inference(img, labs[:S]), 1, warm=0)
    for S in (1, 2):
        print(f"crf_inference S={S}: {fmt(runs[S])}   -> {11 * N * N / statistics.median(runs[S]) * 1e3:.3e} pair evaluations / s (11 applications)")

    # ---- the split (S = 2), each kernel on its own
    im = crf._Image(img, 3.0, sxy, srgb)
    f32 = dict(device="cuda", dtype=torch.float32)
    ones = torch.empty(im.npad // 4, 16, 4, **f32); ng = torch.empty(N, **f32); feat = torch.empty_like(im.feat)
    L.crf_prepare(img, H, W, 3.0, feat, ones, ng)
    sums = torch.empty(im.npad, 16, **f32)
    print(f"normalisation pass (16 columns): {fmt(timed(lambda: L.crf_bilateral(feat, ones, sums, N, 16, sxy, srgb), a.reps))}")
    for S in (1, 2):
        NC = L.crf_columns(S, 21)
        Qn = torch.zeros(im.npad // 4, NC, 4, **f32); Qg = torch.empty(S * 21, N, **f32)
        outb = torch.empty(im.npad, NC, **f32); outg = torch.empty_like(Qg); tmp = torch.empty_like(Qg)
        lab = labs[:S].contiguous()
        L.crf_update(lab, None, None, im.nb, im.ng, Qn, Qg, None, None, None, S, 21, N, 0.7, 10.0, 3.0)
        tb = timed(lambda: L.crf_bilateral(feat, Qn, outb, N, NC, sxy, srgb), a.reps)
        print(f"S={S}: bilateral filter ({NC} columns): {fmt(tb)}   -> {N * N / statistics.median(tb) * 1e3:.3e} pairs / s, "
              f"{2.0 * N * N * NC / statistics.median(tb) * 1e-9:.1f} TFLOP/s on the f32 MFMA")
        print(f"S={S}: Gaussian filter ({S * 21} planes):  {fmt(timed(lambda: L.crf_gaussian(Qg, tmp, outg, S * 21, H, W, 3.0), a.reps))}")
        print(f"S={S}: update:                       {fmt(timed(lambda: L.crf_update(lab, outb, outg, im.nb, im.ng, Qn, Qg, None, None, None, S, 21, N, 0.7, 10.0, 3.0), a.reps))}")

    # ---- one bilateral application: HIP against plain torch, alternating (S = 2: 42 columns)
    fb = torch.stack([torch.arange(N, device="cuda") % W / sxy, torch.arange(N, device="cuda") // W / sxy] +
                     [img.reshape(N, 3)[:, c].float() / srgb for c in range(3)], 1).float().contiguous()
    P = torch.softmax(torch.randn(42, H, W, device="cuda"), 0)
    Xc = (P.reshape(42, N) * im.nb).t().contiguous()
    got = crf.bilateral_filter(img, P, sxy, srgb, image_state=im)
    valid = []
    for mode in ("cdist", "diff"):
        ref = (torch_filter(fb, Xc, a.torch_chunk, mode) * im.nb[:, None]).t().reshape(42, H, W)
        diff = float((got - ref).abs().max())
        ok = diff <= 1e-4 * float(got.max())
        print(f"HIP vs plain torch f32 ({mode}), one application, 42 columns: max |diff| {diff:.3e} (HIP values up to {float(got.max()):.3f})"
              + ("" if ok else "   -> this torch form does NOT compute the filter on this device: not timed"))
        if ok:
            valid.append(mode)
    if not valid:
        print("no torch form reproduces the filter on this device: the baseline comparison is NOT made")
    NC = 48
    Qn = torch.zeros(im.npad // 4, NC, 4, **f32); outb = torch.empty(im.npad, NC, **f32)
    hip, tor = [], {m: [] for m in valid}
    for _ in range(a.reps):
        hip += timed(lambda: L.crf_bilateral(feat, Qn, outb, N, NC, sxy, srgb), 1, warm=0)
        for m in valid:
            tor[m] += timed(lambda: torch_filter(fb, Xc, a.torch_chunk, m), 1, warm=0)
    print(f"one application, HIP crf_bilateral:        {fmt(hip)}")
    for m in valid:
        print(f"one application, plain torch f32 ({m:5s}): {fmt(tor[m])}   (chunk {a.torch_chunk})")
    best = min(valid, key=lambda m: statistics.median(tor[m])) if valid else None
    if best is not None:
        print(f"speed-up over the fastest torch form ({best}), medians: {statistics.median(tor[best]) / statistics.median(hip):.2f}x; "
              f"worst HIP {max(hip):.3f} ms vs best torch {min(tor[best]):.3f} ms")

    # ---- CLI: aff_prepare --alpha 4 32 on JPEGs
    if a.cli_images > 0:
        import PIL.Image
        from wseg_amd import aff_prepare
        with tempfile.TemporaryDirectory() as d:
            os.makedirs(os.path.join(d, "VOC2012", "JPEGImages")); os.makedirs(os.path.join(d, "cam"))
            names = [f"2007_{i:06d}" for i in range(a.cli_images)]
            for i, n in enumerate(names):
                PIL.Image.fromarray(synth.synthetic_rgb_image(H, W, 30 + i).numpy()).save(os.path.join(d, "VOC2012", "JPEGImages", n + ".jpg"))
                np.save(os.path.join(d, "cam", n + ".npy"), {k: v.numpy() for k, v in synth.synthetic_cam_dict(H, W, [3, 11, 14], 30 + i).items()})
            with open(os.path.join(d, "list.txt"), "w") as f:
                f.write("\n".join(names) + "\n")
            t0 = time.time()
            aff_prepare.main(["--infer_list", os.path.join(d, "list.txt"), "--voc12_root", os.path.join(d, "VOC2012"), "--cam_dir",
                              os.path.join(d, "cam"), "--out_crf", os.path.join(d, "out"), "--num_workers", "2", "--alpha", "4", "32"])
            dt = time.time() - t0
            print(f"aff_prepare --alpha 4 32: {a.cli_images} images in {dt:.2f} s = {a.cli_images / dt:.2f} images / s (first image includes start-up)")


if __name__ == "__main__":
    main()
