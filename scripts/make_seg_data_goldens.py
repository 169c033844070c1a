#!/usr/bin/env python
"""Generate tests/golden/seg_data_chain.npz by running the REFERENCE's own transforms (segmentation/lib/datasets/transform.py) on small
inputs (build container only).

  python scripts/make_seg_data_goldens.py --ref <reference checkout> [--out tests/golden]

transform.py imports cv2 at its top; cv2 is not available, so an EMPTY stand-in module takes the name for the import only.  Only the three
transforms that touch no cv2 are called — RandomFlip, ImageNorm, RandomCrop, in the order of BaseDataset.__weak_augment__ — and never ToTensor
(it uses np.long).  Per case the file records the inputs, the seed, the outputs and the state of `random` afterwards: nothing of the
reference's program text.  RandomHSV and RandomScale need cv2 and stay unpinned.
"""
import argparse
import importlib.util
import os
import random
import sys
import types

import numpy as np

CROP = 16
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)       # experiment/SEAM_deeplabv1_resnet38/config.py
# (H, W, seed): both sides smaller than the crop, both larger, one of each — twice each, so that both outcomes of the flip occur
CASES = [(10, 12, 1), (10, 12, 2), (24, 30, 3), (24, 30, 4), (10, 30, 5), (10, 30, 8), (30, 10, 7), (30, 10, 6), (16, 16, 9), (17, 15, 10)]


def load_transform(ref):
    if "cv2" not in sys.modules:
        sys.modules["cv2"] = types.ModuleType("cv2")          # for the import only: nothing that is called touches it
    path = os.path.join(ref, "segmentation", "lib", "datasets", "transform.py")
    spec = importlib.util.spec_from_file_location("ref_seg_transform", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    args = ap.parse_args()
    T = load_transform(args.ref)
    out = dict(crop=np.int64(CROP), mean=np.asarray(MEAN), std=np.asarray(STD), cases=np.asarray(CASES, np.int64))
    flips = []
    for i, (h, w, seed) in enumerate(CASES):
        g = np.random.default_rng(seed)
        image = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
        seg = g.integers(0, 21, (h, w)).astype(np.uint8)
        seg[g.random((h, w)) < 0.1] = 255
        random.seed(seed)
        sample = {"image": image.copy(), "segmentation": seg.copy()}
        sample = T.RandomFlip(0.5)(sample)
        flips.append(not np.array_equal(sample["segmentation"], seg) or not np.array_equal(sample["image"], image))
        sample = T.ImageNorm(MEAN, STD)(sample)
        sample = T.RandomCrop(CROP)(sample)
        state = random.getstate()
        assert sample["image"].dtype == np.float32 and sample["image"].shape == (CROP, CROP, 3)
        out[f"in_image_{i}"], out[f"in_seg_{i}"] = image, seg
        out[f"out_image_{i}"] = sample["image"]
        out[f"out_seg_{i}"] = sample["segmentation"]           # float32, 255.0 in the padding
        out[f"state_{i}"] = np.asarray(state[1], np.uint64)
        out[f"next_{i}"] = np.float64(random.random())         # the next draw of the generator, a second witness of its state
    assert any(flips) and not all(flips), flips
    out["flipped"] = np.asarray(flips)
    path = os.path.join(args.out, "seg_data_chain.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; flipped:", flips)


if __name__ == "__main__":
    main()
