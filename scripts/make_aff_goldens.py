#!/usr/bin/env python
"""Generate tests/golden/aff_*.npz by running the REFERENCE's AffinityNet on the CPU (build container only).

  python scripts/make_aff_goldens.py --ref <reference checkout> [--out tests/golden]

Imports the reference's network.resnet38_aff at run time (absent optional modules stubbed, `.cuda()` made a no-op, as
oracle/make_goldens.py does for the contrast net) and applies the per-image math of its aff_infer.py to procedural weights
(synth.procedural_aff_state_dict), synthetic images and closed-form CAM dictionaries (synth.synthetic_cam_dict): pad to a multiple
of 8, dense affinity matrix ** beta, column normalisation, logt dense squarings, the 21-plane CAM (bg 0.27) pooled 8x8, the product,
bilinear upsample, arg-max, crop.  Only seeds, class lists and the numeric outputs are stored.
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

BG = 0.27
# (name, original H, W, image seed, CAM seed, classes, store the dense matrix)
CASES = [
    ("aff_40x56", 40, 56, 61, 71, [5], True),             # feature map 5 x 7: the smallest the reference accepts (radius 2)
    ("aff_64x88", 64, 88, 62, 72, [3, 11], True),          # 8 x 11: radius 3
    ("aff_100x125", 100, 125, 63, 73, [0, 7, 14], False),  # sides not multiples of 8 (padded 104 x 128 -> 13 x 16): radius 5
    ("aff_375x500", 375, 500, 64, 74, [4, 14], False),     # a VOC-sized image (376 x 504 -> 47 x 63)
]
NEAR_TIE_STORE = 1e-2      # the 375 x 500 case stores the reference's margins only below this (the full map would exceed the size limit)


def _stub_absent_modules():
    for name in ["cv2", "tensorboardX", "torchvision", "torchvision.transforms", "pydensecrf", "pydensecrf.densecrf",
                 "pydensecrf.utils", "imageio", "tqdm"]:
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                sys.modules[name] = types.ModuleType(name)


def load_reference(ref):
    sys.path.insert(0, ref)
    _stub_absent_modules()
    torch.Tensor.cuda = lambda self, *a, **k: self            # the reference moves index tensors / the dense matrix to the device
    import network.resnet38_aff as R
    return R


def reference_walk(model, img, cams, H, W, beta=8, logt=6):
    """aff_infer.py's per-image math on the CPU (float32).  Returns (aff, aff_mat, cam_rw [21, dh, dw], pred [H, W], margin [H, W])."""
    Hp, Wp = int(np.ceil(H / 8) * 8), int(np.ceil(W / 8) * 8)
    img = F.pad(img, (0, Wp - W, 0, Hp - H))
    dh, dw = Hp // 8, Wp // 8
    with torch.no_grad():
        aff = model(img)
        aff_mat = model(img, True)
        A = torch.pow(aff_mat, beta)
        T = A / torch.sum(A, dim=0, keepdim=True)
        for _ in range(logt):
            T = torch.matmul(T, T)
        full = np.zeros((21, H, W), np.float32)
        for k, v in cams.items():
            full[k + 1] = v
        full[0] = BG
        full = np.pad(full, ((0, 0), (0, Hp - H), (0, Wp - W)), mode='constant')
        pooled = F.avg_pool2d(torch.from_numpy(full), 8, 8)
        cam_rw = torch.matmul(pooled.view(21, -1), T).view(1, 21, dh, dw)
        up = torch.nn.Upsample((Hp, Wp), mode='bilinear')(cam_rw)
        _, pred = torch.max(up, 1)
        top2 = torch.topk(up[0], 2, dim=0).values
    pred = pred[0].numpy().astype(np.uint8)[:H, :W]
    margin = (top2[0] - top2[1]).numpy()[:H, :W].astype(np.float32)
    return aff[0].numpy(), aff_mat.numpy(), cam_rw[0].numpy(), pred, margin


PAIR_SIZES = [(3, 6), (4, 9), (5, 5), (5, 7), (6, 9), (7, 12), (8, 11), (9, 9), (10, 14), (11, 11), (12, 30), (13, 16), (30, 12), (47, 63),
              (56, 56)]


def pair_index_fixture(R, model, out):
    """The radius and the (from, to) index arrays the reference's forward uses for each feature-map size (recorded from its own
    get_indices_of_pairs calls on zero images of 8x the size; 56 x 56 takes the predefined set of its constructor), and whether it fails."""
    rec, calls = {}, []
    orig = R.pyutils.get_indices_of_pairs

    def recorder(radius, size):
        calls.append(radius)
        return orig(radius, size)

    R.pyutils.get_indices_of_pairs = recorder
    try:
        for h, w in PAIR_SIZES:
            calls.clear()
            key = f"{h}x{w}"
            try:
                with torch.no_grad():
                    model(torch.zeros(1, 3, 8 * h, 8 * w))
            except Exception as e:                                  # (tiny maps: radius 1 has no offsets)
                rec[key + "_fails"] = np.array(str(e))
                continue
            radius = calls[0] if calls else model.radius
            ind_from, ind_to = (orig(radius, (h, w)) if calls else (model.ind_from.numpy(), model.ind_to.numpy()))
            rec[key + "_radius"] = np.int64(radius)
            rec[key + "_from"] = ind_from.astype(np.int32)
            rec[key + "_to"] = ind_to.astype(np.int32)
    finally:
        R.pyutils.get_indices_of_pairs = orig
    rec["sizes"] = np.array(PAIR_SIZES, np.int64)
    np.savez_compressed(os.path.join(out, "aff_pair_indices.npz"), **rec)
    print("pair indices:", {k: (v.tolist() if v.ndim == 0 else v.shape) for k, v in rec.items() if not k.endswith(("_from", "_to"))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="reference checkout (network/resnet38_aff.py)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--only", default=None, help="comma-separated case names")
    args = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    R = load_reference(args.ref)
    model = R.Net()
    sd = synth.procedural_aff_state_dict(0)
    model.load_state_dict(sd, strict=True)
    model.eval()
    keys = list(model.state_dict().keys())
    np.savez_compressed(os.path.join(args.out, "aff_state_dict_keys.npz"), keys=np.array(keys),
                        shapes=np.array([",".join(str(d) for d in model.state_dict()[k].shape) for k in keys]))
    assert keys == list(arch.state_dict_spec(arch.AFF_HEAD_CONVS).keys())
    only = set(args.only.split(",")) if args.only else None
    if not only:
        pair_index_fixture(R, model, args.out)
    for name, H, W, iseed, cseed, classes, dense in CASES:
        if only and name not in only:
            continue
        img = synth.synthetic_images(1, (H, W), iseed)
        cams = {k: v.numpy() for k, v in synth.synthetic_cam_dict(H, W, classes, cseed).items()}
        aff, aff_mat, cam_rw, pred, margin = reference_walk(model, img, cams, H, W)
        rec = dict(H=H, W=W, img_seed=iseed, cam_seed=cseed, classes=np.array(classes, np.int64), beta=8, logt=6, aff=aff, cam_rw=cam_rw, pred=pred)
        if dense:
            rec["aff_mat"] = aff_mat
            rec["margin"] = margin
        else:
            idx = np.flatnonzero(margin.reshape(-1) < NEAR_TIE_STORE)
            rec["near_idx"] = idx.astype(np.int64)
            rec["near_margin"] = margin.reshape(-1)[idx]
            rec["near_store"] = NEAR_TIE_STORE
        if name == "aff_375x500":
            # two files of <= 0.5 MB: the affinities, and the walk's outputs
            np.savez_compressed(os.path.join(args.out, name + "_pairs.npz"), **{k: rec[k] for k in ("H", "W", "img_seed", "aff")})
            np.savez_compressed(os.path.join(args.out, name + "_rw.npz"), **{k: v for k, v in rec.items() if k != "aff"})
        else:
            np.savez_compressed(os.path.join(args.out, name + ".npz"), **rec)
        print(name, "aff", aff.shape, "range", float(aff.min()), float(aff.max()), "aff^8 mean", float((aff ** 8).mean()),
              "classes in pred", np.unique(pred).tolist(), "min margin", float(margin.min()))


if __name__ == "__main__":
    main()
