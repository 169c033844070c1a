#!/usr/bin/env python
"""Generate tests/golden/seg_*.npz by running the REFERENCE's DeepLab-v1 (ResNet-38) on the CPU (build container only).

  python scripts/make_seg_goldens.py --ref <reference checkout> [--out tests/golden]

Imports the reference's net.deeplabv1 from <ref>/segmentation/lib at run time (absent optional modules stubbed, as
scripts/make_aff_goldens.py does for the AffinityNet) and applies the prepare / collect math of its
experiment/SEAM_deeplabv1_resnet38/test.py in float32 to procedural weights (synth.procedural_seg_state_dict) and to the list of scaled
synthetic images OUR host code makes (seg_infer.scaled_inputs: the reference's cv2 resize is not available offline, so parity is pinned
from that list onward).  Only seeds, names, shapes and the numeric outputs are stored: per pass the coarse cls_conv logits (a forward
hook), the mean logits, the label map, the full top-2 margin map.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from wseg_amd import arch, synth  # noqa: E402
from wseg_amd.seg_infer import TEST_MULTISCALE, scaled_inputs  # noqa: E402

WEIGHT_SEED = 0
# (name, original H, W, image seed, scales)
CASES = [
    ("seg_40x56", 40, 56, 81, TEST_MULTISCALE),          # scaled inputs from 20 x 28 (feature map 3 x 4) to 70 x 98
    ("seg_33x47", 33, 47, 86, TEST_MULTISCALE),          # no side a multiple of 8
    ("seg_100x125", 100, 125, 85, (0.5, 1.0)),           # two scales only: the coarse logits stay small
    # (image seeds: of 81..92 the one with the smallest near-tie share per case — 0.67 %, 0.64 %, 0.89 %)
]
MIN_CLASSES, MIN_SHARE = 4, 0.02                          # every label map: at least 4 classes with >= 2 % of the pixels each
NEAR_TIE_REL, NEAR_TIE_SHARE = 1e-3, 0.01                 # pixels whose margin is below 1e-3 * max|mean logit|: at most 1 %
MEAN_SPLIT = 11                                           # the 100 x 125 mean logits go into two files of <= 11 classes (committed-file limit)


def _stub_absent_modules():
    for name in ["cv2", "tqdm", "pydensecrf", "pydensecrf.densecrf", "pydensecrf.utils", "tensorboardX", "mxnet"]:
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                sys.modules[name] = types.ModuleType(name)


def load_reference(ref):
    sys.path.insert(0, os.path.join(ref, "segmentation", "lib"))
    _stub_absent_modules()
    from net.deeplabv1 import deeplabv1
    cfg = types.SimpleNamespace(MODEL_BACKBONE="resnet38", MODEL_BACKBONE_PRETRAIN=False, MODEL_NUM_CLASSES=21, TRAIN_BN_MOM=0.0003)
    return deeplabv1(cfg)


def reference_collect(model, scaled, H, W):
    """test.py:71-104 on the CPU in float32 (TEST_FLIP on, TEST_CRF off): returns (coarse [n_pass][21, fh, fw], mean [21, H, W], label
    [H, W] uint8, margin [H, W])."""
    coarse, results = [], []
    hook = model.cls_conv.register_forward_hook(lambda m, i, o: coarse.append(o[0].clone()))
    try:
        with torch.no_grad():
            for x in scaled:
                x = torch.from_numpy(x)[None]
                for img in (x, torch.flip(x, [3])):                                   # prepare_func
                    results.append(model(img))
            for i in range(len(results)):                                             # collect_func
                r = F.interpolate(results[i], (H, W), mode='bilinear', align_corners=True)
                results[i] = torch.flip(r, [3]) if i % 2 == 1 else r
            mean = torch.mean(torch.cat(results, dim=0), dim=0, keepdim=True)
            prob = F.softmax(mean, dim=1)[0]
            label = torch.argmax(prob, dim=0)
            top2 = torch.topk(mean[0], 2, dim=0).values
    finally:
        hook.remove()
    return [c.numpy() for c in coarse], mean[0].numpy(), label.numpy().astype(np.uint8), (top2[0] - top2[1]).numpy().astype(np.float32)


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
    keys = list(model.state_dict().keys())
    assert keys == list(arch.seg_state_dict_spec().keys())
    names = {id(p): n for n, p in model.named_parameters()}
    groups = [[names[id(p)] for p in g] for g in model.get_parameter_groups()]
    np.savez_compressed(os.path.join(args.out, "seg_state_dict_keys.npz"), keys=np.array(keys),
                        shapes=np.array([",".join(str(d) for d in model.state_dict()[k].shape) for k in keys]),
                        **{f"group{i}": np.array(g, dtype=str) for i, g in enumerate(groups)})
    print("keys", len(keys), "groups", [len(g) for g in groups])
    only = set(args.only.split(",")) if args.only else None
    for name, H, W, iseed, scales in CASES:
        if only and name not in only:
            continue
        img = synth.synthetic_images(1, (H, W), iseed)[0].permute(1, 2, 0).numpy()          # normalised HWC, as the loader hands it over
        scaled = scaled_inputs(img, scales)
        coarse, mean, label, margin = reference_collect(model, scaled, H, W)
        share = np.bincount(label.reshape(-1), minlength=21) / label.size
        near = float((margin < NEAR_TIE_REL * np.abs(mean).max()).mean())
        print(name, "sizes", [s.shape[1:] for s in scaled], "coarse", [c.shape[1:] for c in coarse][::2], "max|mean|", float(np.abs(mean).max()),
              "classes >= 2 %:", {int(c): round(float(s), 3) for c, s in enumerate(share) if s >= MIN_SHARE}, "near-tie share", near)
        assert (share >= MIN_SHARE).sum() >= MIN_CLASSES, f"{name}: fewer than {MIN_CLASSES} classes with >= {MIN_SHARE:.0%} of the pixels"
        assert near <= NEAR_TIE_SHARE, f"{name}: {near:.2%} of the pixels are near ties"
        rec = dict(H=H, W=W, weight_seed=WEIGHT_SEED, img_seed=iseed, scales=np.array(scales, np.float64), n_pass=len(coarse), label=label,
                   margin=margin, sizes=np.array([s.shape[1:] for s in scaled], np.int64))
        rec.update({f"coarse_{i}": c for i, c in enumerate(coarse)})
        if mean.nbytes > 900_000:
            np.savez_compressed(os.path.join(args.out, name + "_mean_a.npz"), mean=mean[:MEAN_SPLIT])
            np.savez_compressed(os.path.join(args.out, name + "_mean_b.npz"), mean=mean[MEAN_SPLIT:])
        else:
            rec["mean"] = mean
        np.savez_compressed(os.path.join(args.out, name + ".npz"), **rec)


if __name__ == "__main__":
    main()
