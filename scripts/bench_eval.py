"""The CAM evaluation curve (wseg_amd.eval --curve: 60 background thresholds) on N synthetic 375 x 500 dictionaries (2-3 present classes)
and ground truths, host path against device path on the same box:

  1. `main --curve`            the host path (numpy; 60 passes over the files, one core)
  2. `main --curve --device`   one pass: DataLoader workers read and decode, csrc/eval.hip counts; also timed with the same loaders and NO
                               device work, which is the share of the device CLI that is file reading
  3. DeviceEval in memory      per image on tensors that are already on the device (what contrast_infer --gt_dir does): wall time per add,
                               kernel time by HIP events, bytes/s against the planes and the ground truth read

    python scripts/bench_eval.py [--n 16] [--repeat 16] [--workers 8] [--reps 50] > profiles/r15_eval.txt
"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import PIL.Image
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wseg_amd import eval as weval      # noqa: E402
from wseg_amd import synth              # noqa: E402

H, W = 375, 500


def make_image(i):
    rng = np.random.default_rng(i)
    classes = sorted(rng.choice(20, 2 + i % 2, replace=False).tolist())
    cams = {k: v.numpy() for k, v in synth.synthetic_cam_dict(H, W, classes, 70 + i).items()}
    stack = np.stack([np.full((H, W), 0.3, np.float32)] + [cams[c] for c in classes])
    gt = np.array([0] + [c + 1 for c in classes], np.uint8)[stack.argmax(0)]          # the arg-max at 0.3, so the curve has a peak
    gt[rng.random((H, W)) < 0.03] = 255
    return cams, gt


def quiet_main(argv):
    out = io.StringIO()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(out):
        best = weval.main(argv)
    return time.perf_counter() - t0, best, out.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16, help="files written; the host curve reads each 60 times")
    ap.add_argument("--repeat", type=int, default=16, help="the device CLI's list names every file this many times")
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    print(f"device {torch.cuda.get_device_name(0)}; {a.n} synthetic {H}x{W} dictionaries (2-3 classes) and ground truths; 60 thresholds")
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "cam")); os.makedirs(os.path.join(d, "gt"))
        names = [f"2007_{i:06d}" for i in range(a.n)]
        images = [make_image(i) for i in range(a.n)]
        for n, (cams, gt) in zip(names, images):
            np.save(os.path.join(d, "cam", n + ".npy"), cams, allow_pickle=True)
            PIL.Image.fromarray(gt).save(os.path.join(d, "gt", n + ".png"))
        for fn, rep in (("list.txt", 1), ("long.txt", a.repeat)):
            with open(os.path.join(d, fn), "w") as f:
                f.write("\n".join(names * rep) + "\n")
        argv = ["--predict_dir", os.path.join(d, "cam"), "--gt_dir", os.path.join(d, "gt"), "--type", "npy", "--curve"]
        dev = ["--device", "--num_workers", str(a.workers)]
        quiet_main(["--list", os.path.join(d, "list.txt")] + argv + dev)              # warm-up: library, context, page cache
        t_host, best_h, out_h = quiet_main(["--list", os.path.join(d, "list.txt")] + argv)
        t_dev, best_d, out_d = quiet_main(["--list", os.path.join(d, "list.txt")] + argv + dev)
        print(f"1. host   main --curve          : {t_host:8.2f} s = {t_host / a.n * 1e3:8.1f} ms per image ({a.n} images, 60 passes)")
        print(f"2. device main --curve --device : {t_dev:8.2f} s = {t_dev / a.n * 1e3:8.1f} ms per image ({a.n} images, {a.workers} workers, includes worker start-up)")
        print(f"   printed lines equal: {out_h == out_d}; best {best_h} / {best_d}")
        nl = a.n * a.repeat
        t_long, best_l, _ = quiet_main(["--list", os.path.join(d, "long.txt")] + argv + dev)
        t0 = time.perf_counter()
        loader = torch.utils.data.DataLoader(weval._EvalFiles(names * a.repeat, os.path.join(d, "cam"), os.path.join(d, "gt"), "npy"),
                                             batch_size=None, shuffle=False, num_workers=a.workers, pin_memory=True)
        for _ in loader:
            pass
        t_read = time.perf_counter() - t0
        print(f"   device CLI, {nl} list entries  : {t_long:8.2f} s = {t_long / nl * 1e3:8.2f} ms per image; the same loaders with no device work: "
              f"{t_read:.2f} s = {100 * t_read / t_long:.0f} % of it")
        share = t_read / t_long
        print(f"   per image, host / device CLI: {t_host / a.n / (t_long / nl):.1f}x; file reading and decoding is {100 * share:.0f} % of the device CLI: it is "
              + ("bound by the loaders, not by the GPU" if share > 0.5 else "NOT bound by the loaders: most of its time is device work and hand-over"))

        # ---- 3. in memory
        cams, gt = images[1 % a.n]
        K = len(cams)
        full = torch.zeros(20, H, W, device="cuda")
        for k, v in cams.items():
            full[k] = torch.from_numpy(v).cuda()
        views = {k: full[k] for k in cams}
        gt_dev = torch.from_numpy(gt).cuda()
        pred = torch.from_numpy(gt).cuda()
        ev = weval.DeviceEval("cuda")
        blocker = torch.randn(8192, 8192, device="cuda")
        views20 = {k: full[k] for k in range(20)}          # all 20 classes present: no workgroup histogram, 64-bit global adds per pixel
        for what, fn, nbytes in (("add_cams (%d planes)" % K, lambda: ev.add_cams(views, gt_dev), H * W * (4 * K + 1)),
                                 ("add_cams (20 planes)", lambda: ev.add_cams(views20, gt_dev), H * W * 81),
                                 ("add_masks", lambda: ev.add_masks(pred, gt_dev), H * W * 2)):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            t_enq = (time.perf_counter() - t0) / a.reps
            torch.cuda.synchronize()
            t_wall = (time.perf_counter() - t0) / a.reps
            # kernel time: the host needs longer to enqueue an add than the device to run it, so events around adds on an idle queue would time
            # the host.  Park the queue behind a matrix product of several ms, enqueue `reps` adds between two events meanwhile, and the
            # events then bracket back-to-back kernels.
            ks = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.mm(blocker, blocker)
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record(); e1.synchronize()
                ks.append(e0.elapsed_time(e1) * 1e3 / a.reps)
            med = statistics.median(ks)
            print(f"3. DeviceEval.{what:22s}: enqueue {t_enq * 1e6:7.1f} us, wall {t_wall * 1e6:7.1f} us per image; kernel (back to back, {a.reps} per sample) median "
                  f"{med:6.2f} us (min {min(ks):.2f}, max {max(ks):.2f}) = {nbytes / med * 1e-6:6.3f} TB/s of {nbytes} bytes read")
        t0 = time.perf_counter()
        ev.curve_results()
        print(f"   curve_results (read-back + prefix sums + 60 IoU tables): {(time.perf_counter() - t0) * 1e3:.2f} ms, once per dataset")


if __name__ == "__main__":
    main()
