#!/usr/bin/env python
"""AffinityNet inference timing at 376 x 504 (a 375 x 500 VOC image padded to a multiple of 8; 47 x 63 feature map, radius 5).

Per-image device time (CUDA events, medians over --iters), split into backbone + ELU head, pairs, and walk; the walk both as the HIP
stencil (rw_prepare + random_walk) and as the reference's formulation on the same device and the same affinities (dense matrix,
pow(beta), column normalisation, logt torch.matmul squarings, the product with the 21 pooled planes).  Then whole-CLI images/s of
`python -m wseg_amd.aff_infer` over a synthetic VOC list (JPEG decode, loader, CAM .npy read, png write included).

  python scripts/bench_aff_infer.py [--precision fp32] [--iters 20] [--cli_images 32]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wseg_amd import _lib as L, synth  # noqa: E402
from wseg_amd.resnet38_aff import Net, pair_radius  # noqa: E402


def timed(fn, iters):
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cli_images", type=int, default=32)
    ap.add_argument("--beta", type=int, default=8)
    ap.add_argument("--logt", type=int, default=6)
    args = ap.parse_args()
    m = Net(precision=args.precision)
    m.load_state_dict(synth.procedural_aff_state_dict(0))
    m.eval().cuda()
    x = synth.synthetic_images(1, (376, 504), 64).cuda()
    eng = m._engine.active(x.device)
    res = {"precision": args.precision, "size": [376, 504]}
    aff, (h, w, r) = m.affinities(x)
    assert r == pair_radius(h, w)

    def backbone_head():
        return eng.run_backbone([x])

    for _ in range(3):
        m.affinities(x)
    torch.cuda.synchronize()
    res["forward_ms"] = timed(lambda: m.affinities(x), args.iters)                      # backbone + head + pairs
    res["backbone_ms"] = timed(backbone_head, args.iters)
    f9 = torch.randn(h * w, 448, device="cuda", dtype=torch.float32 if args.precision != "bf16" else torch.bfloat16)
    out = torch.empty_like(aff)
    res["pairs_ms"] = timed(lambda: L.aff_pairs(f9, 448, 448, out, 1, h, w, r), args.iters)
    res["head_ms"] = res["forward_ms"] - res["backbone_ms"] - res["pairs_ms"]
    P, area = aff.shape[1], h * w
    pooled = torch.rand(21, h, w, device="cuda")
    wgt = torch.empty(1, 2 * P, area, device="cuda")
    rsum = torch.empty(1, area, device="cuda")
    cam_rw = torch.empty_like(pooled)

    def hip_walk():
        L.rw_prepare(aff, wgt, rsum, 1, h, w, r, args.beta)
        L.random_walk(wgt, rsum, pooled, cam_rw, 1, 21, h, w, r, args.logt)

    def dense_walk():
        A = torch.empty(area, area, device="cuda")
        L.aff_to_dense(aff, A, h, w, r)
        A = torch.pow(A, args.beta)
        T = A / torch.sum(A, dim=0, keepdim=True)
        for _ in range(args.logt):
            T = torch.matmul(T, T)
        return torch.matmul(pooled.view(21, -1), T)

    hip_walk(); dense_walk(); torch.cuda.synchronize()
    res["walk_hip_ms"] = timed(hip_walk, args.iters)
    res["walk_dense_ms"] = timed(dense_walk, args.iters)
    ref = dense_walk().view(21, h, w)
    hip_walk()
    res["walk_rel_diff"] = float(((cam_rw - ref).abs() / ref.abs().amax(dim=(1, 2), keepdim=True)).max())
    res["walk_speedup"] = res["walk_dense_ms"] / res["walk_hip_ms"]

    if args.cli_images > 0:
        import PIL.Image
        from wseg_amd import aff_infer
        with tempfile.TemporaryDirectory() as d:
            os.makedirs(os.path.join(d, "VOC2012", "JPEGImages"))
            os.makedirs(os.path.join(d, "cam"))
            rng = np.random.default_rng(0)
            names = [f"2007_{i:06d}" for i in range(args.cli_images)]
            for i, n in enumerate(names):
                PIL.Image.fromarray(rng.integers(0, 256, (375, 500, 3), dtype=np.uint8)).save(os.path.join(d, "VOC2012", "JPEGImages", n + ".jpg"))
                cams = {k: v.numpy() for k, v in synth.synthetic_cam_dict(375, 500, [i % 20, (7 * i + 3) % 20], i).items()}
                np.save(os.path.join(d, "cam", n + ".npy"), cams, allow_pickle=True)
            with open(os.path.join(d, "list.txt"), "w") as f:
                f.write("\n".join(f"/JPEGImages/{n}.jpg" for n in names) + "\n")
            argv = ["--weights", "procedural", "--infer_list", os.path.join(d, "list.txt"), "--voc12_root", os.path.join(d, "VOC2012"),
                    "--cam_dir", os.path.join(d, "cam"), "--out_rw", os.path.join(d, "rw"), "--num_workers", "4", "--precision", args.precision]
            t0 = time.perf_counter()
            aff_infer.main(argv)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert len(os.listdir(os.path.join(d, "rw"))) == len(names)
            res["cli_images"] = len(names)
            res["cli_img_per_s"] = len(names) / dt
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
