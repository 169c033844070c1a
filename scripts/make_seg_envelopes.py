#!/usr/bin/env python
"""Generate tests/golden/seg_*_env.npz and seg_*_tap64.npz: the REFERENCE's DeepLab-v1 on the CPU in float64, in float32 (three vectorised
orders and one sequential chain), as a split-bf16 sum and in bfloat16, on the inputs of scripts/make_seg_goldens.py's cases.

  python scripts/make_seg_envelopes.py --ref <reference checkout> [--out tests/golden] [--only seg_40x56,...]

Same loader, weights, cases and scaled inputs as make_seg_goldens.py; the seg_*.npz files it wrote are not touched.  Every variant is
the reference's net; what differs is the number format and, for two of them, how an nn.Conv2d with more than 3 input channels sums:

  c64        model.double() on float64 inputs: the yardstick
  f32_a/b/c  float32 with oneDNN on / with torch.backends.mkldnn.flags(enabled=False) / with one thread
  f32_chain  float32, each conv ONE accumulation chain over K in the pack's order (tap outer, channel inner), 4 products per step
             (acc = acc + W[:, s:s+4] @ cols[s:s+4] on the unfolded input): the longest chain a float32 evaluation of this net has
  x3         float64, each conv as conv(xh, wh) + conv(xh, wl) + conv(xl, wh) of the bf16 halves (tests/conv_f64.py:split_bf16), the
             bias added afterwards: the dropped lo.lo term and the bf16 rounding of lo alone, summed exactly
  bf16       model.bfloat16() on bf16 inputs (as oracle/make_goldens.py's step_refbf16_golden does for the contrast net)

<case>_env.npz    <variant>_<i>: the coarse cls_conv logits [21, fh, fw] of pass i as float64; variants, n_pass
<case>_tap64.npz  for the plain pass of the smallest and of the largest scale (tap_passes): tap_<i> = c64's input of conv_fov
                  (relu(bn7(conv6)), a forward pre-hook) on the channels c0::stride as [fh, fw, n_ch] float64, tapmax_<i> = max |tap64|
                  over all 4096 channels, and per variant v of f32_chain / x3 / bf16 the scalars dev_<v>_<i> = max |tap_v - tap64| over
                  all channels, devsub_<v>_<i> the same over the stored channels
Only numeric outputs, seeds and shapes are stored.
"""
import argparse
import contextlib
import copy
import os
import sys
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from make_seg_goldens import CASES, WEIGHT_SEED, load_reference  # noqa: E402
from tests.conv_f64 import split_bf16  # noqa: E402
from wseg_amd import synth  # noqa: E402
from wseg_amd.seg_infer import scaled_inputs  # noqa: E402

VARIANTS = ("c64", "f32_a", "f32_b", "f32_c", "f32_chain", "x3", "bf16")
TAP_VARIANTS = ("f32_chain", "x3", "bf16")
TAP_C0, TAP_STRIDE = 7, 15                 # 273 of the 4096 channels; an odd stride walks every lane position of every 256-wide column tile
CHAIN_STEP = 4


def _chain_forward(self, x):
    """float32 conv as one K chain: K = KH KW IC in the order tap outer, channel inner, CHAIN_STEP products per step"""
    N, C = x.shape[:2]
    kh, kw = self.kernel_size
    cols = F.unfold(x, self.kernel_size, self.dilation, self.padding, self.stride)                   # [N, C kh kw, L], channel outer
    L = cols.shape[-1]
    cols = cols.view(N, C, kh * kw, L).permute(2, 1, 0, 3).reshape(kh * kw * C, N * L).contiguous()
    w = self.weight.permute(0, 2, 3, 1).reshape(self.out_channels, kh * kw * C).contiguous()
    acc = torch.zeros(self.out_channels, N * L, dtype=x.dtype)
    for s in range(0, w.shape[1], CHAIN_STEP):
        acc = acc + w[:, s:s + CHAIN_STEP] @ cols[s:s + CHAIN_STEP]
    oh = (x.shape[2] + 2 * self.padding[0] - self.dilation[0] * (kh - 1) - 1) // self.stride[0] + 1
    out = acc.view(self.out_channels, N, oh, L // oh).permute(1, 0, 2, 3)
    return out if self.bias is None else out + self.bias.view(1, -1, 1, 1)


def _x3_forward(self, x):
    """float64 conv of the bf16 halves without the lo.lo term; the bias afterwards"""
    xh, xl = (t.double() for t in split_bf16(x))
    wh, wl = (t.double() for t in split_bf16(self.weight))
    conv = lambda a, b: F.conv2d(a, b, None, self.stride, self.padding, self.dilation, self.groups)  # noqa: E731
    out = conv(xh, wh) + conv(xh, wl) + conv(xl, wh)
    return out if self.bias is None else out + self.bias.view(1, -1, 1, 1)


def _patched(model, fwd):
    for m in model.modules():
        if isinstance(m, torch.nn.Conv2d) and m.in_channels > 3:
            assert m.groups == 1 and m.padding_mode == "zeros"
            m.forward = types.MethodType(fwd, m)
    return model


@contextlib.contextmanager
def _one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def variants_of(model):
    """{variant: (model, input dtype, context manager factory)}; `model` is the float32 reference net in eval mode"""
    null = contextlib.nullcontext
    return {
        "c64": (copy.deepcopy(model).double(), torch.float64, null),
        "f32_a": (model, torch.float32, lambda: torch.backends.mkldnn.flags(enabled=True)),
        "f32_b": (model, torch.float32, lambda: torch.backends.mkldnn.flags(enabled=False)),
        "f32_c": (model, torch.float32, _one_thread),
        "f32_chain": (_patched(copy.deepcopy(model), _chain_forward), torch.float32, null),
        "x3": (_patched(copy.deepcopy(model).double(), _x3_forward), torch.float64, null),
        "bf16": (copy.deepcopy(model).bfloat16(), torch.bfloat16, null),
    }


def run_variant(model, dtype, ctx, scaled, tap_passes):
    """the passes of test.py's prepare_func (per scale the plain, then the x-flipped image): ([coarse float64 [21, fh, fw]], {pass: tap
    float64 [fh, fw, 4096]})"""
    coarse, taps, state = [], {}, {"i": 0}
    h1 = model.cls_conv.register_forward_hook(lambda m, i, o: coarse.append(o[0].detach().double().numpy().copy()))

    def pre(m, inp):
        if state["i"] in tap_passes:
            taps[state["i"]] = inp[0][0].detach().double().permute(1, 2, 0).numpy().copy()
    h2 = model.conv_fov.register_forward_pre_hook(pre)
    try:
        with torch.no_grad(), ctx():
            for x in scaled:
                x = torch.from_numpy(x)[None].to(dtype)
                for img in (x, torch.flip(x, [3])):
                    model(img)
                    state["i"] += 1
    finally:
        h1.remove()
        h2.remove()
    return coarse, taps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="reference checkout (segmentation/lib/net/deeplabv1.py)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--only", default=None, help="comma-separated case names")
    args = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    model = load_reference(args.ref)
    model.load_state_dict(synth.procedural_seg_state_dict(WEIGHT_SEED), strict=True)
    model.eval()
    nets = variants_of(model)
    only = set(args.only.split(",")) if args.only else None
    for name, H, W, iseed, scales in CASES:
        if only and name not in only:
            continue
        img = synth.synthetic_images(1, (H, W), iseed)[0].permute(1, 2, 0).numpy()
        scaled = scaled_inputs(img, scales)
        tap_passes = (0, 2 * (len(scaled) - 1))
        env = dict(variants=np.array(VARIANTS), n_pass=2 * len(scaled), weight_seed=WEIGHT_SEED, img_seed=iseed)
        tap = dict(tap_passes=np.array(tap_passes), c0=TAP_C0, stride=TAP_STRIDE, tap_variants=np.array(TAP_VARIANTS))
        taps64 = None
        for v in VARIANTS:
            t0 = time.time()
            coarse, taps = run_variant(*nets[v], scaled, tap_passes)
            env.update({f"{v}_{i}": c for i, c in enumerate(coarse)})
            if v == "c64":
                taps64, c64 = taps, coarse
                for i in tap_passes:
                    tap[f"tap_{i}"] = taps[i][:, :, TAP_C0::TAP_STRIDE].copy()
                    tap[f"tapmax_{i}"] = float(np.abs(taps[i]).max())
            elif v in TAP_VARIANTS:
                for i in tap_passes:
                    d = np.abs(taps[i] - taps64[i])
                    tap[f"dev_{v}_{i}"], tap[f"devsub_{v}_{i}"] = float(d.max()), float(d[:, :, TAP_C0::TAP_STRIDE].max())
            dev = max(float(np.abs(c - r).max()) for c, r in zip(coarse, c64))
            print(f"{name} {v}: max |coarse - c64| {dev:.3e}" + "".join(f", tap {i}: {tap[f'dev_{v}_{i}']:.3e}" for i in tap_passes if v in TAP_VARIANTS)
                  + f"  ({time.time() - t0:.1f} s)", flush=True)
        np.savez_compressed(os.path.join(args.out, name + "_env.npz"), **env)
        np.savez_compressed(os.path.join(args.out, name + "_tap64.npz"), **tap)
        print(name, "tap channels", tap[f"tap_{tap_passes[0]}"].shape[-1], "max |tap64|", [tap[f"tapmax_{i}"] for i in tap_passes],
              "bytes", [os.path.getsize(os.path.join(args.out, name + s + ".npz")) for s in ("_env", "_tap64")])


if __name__ == "__main__":
    main()
