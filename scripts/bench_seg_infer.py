#!/usr/bin/env python
"""Time of the DeepLab inference stage on one MI355X (wseg_amd/seg_infer.py), one 375 x 500 image, 6 scales x {plain, flipped}:

  * the per-image split: the 6 backbone + head passes (N = 2 each), the fusion launch, the CRF (with --crf);
  * the fused kernel (wseg_seg_fuse) against the chain it replaces, built from what the tree already has: L.resize_planar_fwd twice per
    pass (align=True, flip_x, accumulate), then torch's division, softmax and arg-max — time and bytes moved (counted from the shapes:
    every tensor a launch reads or writes, once); the chain is handed its planar coarse logits for free;
  * the share of the dilation-12 conv_fov launch in a pass, from event brackets around every conv launch (L.PROFILE);
  * images / s of the CLI on synthetic JPEGs of that size.

  python scripts/bench_seg_infer.py [--precision bf16] [--iters 10] [--crf] [--cli_images 8]
"""
import argparse
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wseg_amd import _lib as L  # noqa: E402
from wseg_amd import arch, seg_infer, synth  # noqa: E402
from wseg_amd.deeplabv1_resnet38 import Net  # noqa: E402


def timed(fn, iters, warmup=2):
    """mean milliseconds of fn() on the current stream"""
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32", "bf16x3"])
    ap.add_argument("--size", default=[375, 500], type=int, nargs=2)
    ap.add_argument("--iters", default=10, type=int)
    ap.add_argument("--crf", action="store_true")
    ap.add_argument("--cli_images", default=8, type=int)
    args = ap.parse_args()
    H, W = args.size
    model = Net(precision=args.precision)
    model.load_state_dict(synth.procedural_seg_state_dict(0), strict=True)
    model.eval().cuda()
    img = model.normalize(synth.synthetic_rgb_image(H, W, 1).numpy())
    scaled = [torch.from_numpy(s).cuda() for s in seg_infer.scaled_inputs(img)]
    print(f"{args.precision}, {H} x {W}, scaled inputs {[tuple(s.shape[1:]) for s in scaled]}")

    # ---- the per-image split
    t_pass = timed(lambda: seg_infer.coarse_passes(model, scaled), args.iters)
    passes = seg_infer.coarse_passes(model, scaled)
    dev = passes[0].rows.device
    amax = torch.empty(H, W, device=dev, dtype=torch.uint8)
    prob = torch.empty(21, H, W, device=dev)
    t_fuse = timed(lambda: L.seg_fuse(passes, H, W, 21, amax, None, prob, None), args.iters * 5)
    line = f"per image: {len(passes) // 2} backbone + head passes {t_pass:.2f} ms, fusion {t_fuse:.3f} ms"
    if args.crf:
        from wseg_amd.crf import crf_inference_from_probs
        img_u8 = torch.from_numpy(seg_infer.denormalise_u8(img)).cuda()
        t_crf = timed(lambda: crf_inference_from_probs(img_u8, prob, t=1, return_argmax=True), max(2, args.iters // 3), warmup=1)
        line += f", CRF (1 iteration) {t_crf:.1f} ms"
    print(line)

    # ---- fused kernel against the chain of existing launches
    planar = [p.rows.float().view(-1, p.fh, p.fw, p.ld)[p.img, :, :, :21].permute(2, 0, 1).contiguous() for p in passes]
    tmps = [torch.empty(21, p.ih, p.iw, device=dev) for p in passes]
    acc = torch.empty(21, H, W, device=dev)

    def chain():
        for i, (p, c, tmp) in enumerate(zip(passes, planar, tmps)):
            L.resize_planar_fwd(c, tmp, 21, p.fh, p.fw, p.ih, p.iw, True)
            L.resize_planar_fwd(tmp, acc, 21, p.ih, p.iw, H, W, True, flip_x=p.flip, accumulate=i > 0)
        pr = torch.softmax(acc / len(passes), 0)
        return pr, torch.argmax(pr, 0)

    t_chain = timed(chain, args.iters * 2)
    pr, am = chain()
    torch.cuda.synchronize()
    es = passes[0].rows.element_size()
    out_b = 21 * H * W * 4
    b_fused = sum(p.fh * p.fw * p.ld * es for p in passes) + out_b + H * W
    b_chain = sum(21 * p.fh * p.fw * 4 + 2 * 21 * p.ih * p.iw * 4 + (2 if i else 1) * out_b for i, p in enumerate(passes)) + 4 * out_b + out_b + H * W * 8
    agree = float((am.to(torch.uint8) == amax).float().mean())
    print(f"fused kernel: 1 launch {t_fuse:.3f} ms, {b_fused / 1e6:.1f} MB;  chain: {2 * len(passes) + 3} launches {t_chain:.3f} ms, {b_chain / 1e6:.1f} MB"
          f"  (labels equal on {agree:.4%} of the pixels, max |dprob| {float((pr - prob).abs().max()):.2e})")

    # ---- conv_fov's share of a pass (scale 1.0, N = 2)
    x = torch.stack([scaled[2], scaled[2].flip(2)])
    model.coarse_logits(x)
    L.PROFILE, L.PROFILE_STRIDE = [], 1
    L.profile_begin_step(0)
    model.coarse_logits(x)
    torch.cuda.synchronize()
    rec, L.PROFILE = L.PROFILE, None
    total = sum(e0.elapsed_time(e1) for e0, e1, *_ in rec)
    fov = sum(e0.elapsed_time(e1) for e0, e1, _f, label, _i in rec if f" d{arch.SEG_HEAD_DILATION} " in label)
    print(f"one pass at scale 1.0 (N = 2): {len(rec)} conv launches {total:.2f} ms in event brackets, conv_fov (3x3, dilation 12, K = 36864) "
          f"{fov:.3f} ms = {fov / total:.1%}")

    # ---- the CLI
    if args.cli_images:
        import PIL.Image
        with tempfile.TemporaryDirectory() as tmp:
            os.makedirs(os.path.join(tmp, "VOC2012", "JPEGImages"))
            names = [f"2007_{i:06d}" for i in range(args.cli_images)]
            for i, n in enumerate(names):
                PIL.Image.fromarray(synth.synthetic_rgb_image(H, W, 50 + i).numpy()).save(os.path.join(tmp, "VOC2012", "JPEGImages", n + ".jpg"), quality=95)
            with open(os.path.join(tmp, "list.txt"), "w") as f:
                f.write("\n".join(names) + "\n")
            argv = ["--weights", "procedural", "--infer_list", os.path.join(tmp, "list.txt"), "--voc12_root", os.path.join(tmp, "VOC2012"),
                    "--out_png", os.path.join(tmp, "png"), "--precision", args.precision, "--num_workers", "4"] + (["--crf"] if args.crf else [])
            t0 = time.perf_counter()
            seg_infer.main(argv)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"CLI: {args.cli_images} images in {dt:.2f} s = {args.cli_images / dt:.2f} images / s (model construction and the first image's "
                  f"pack set-up included)")


if __name__ == "__main__":
    main()
