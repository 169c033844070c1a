#!/usr/bin/env python
"""Generate tests/golden/aff_loss_*.npz by running the REFERENCE's label extractor, AffinityNet and training-loss lines on the CPU
(build container only).

  python scripts/make_aff_loss_goldens.py --ref <reference checkout> [--out tests/golden]

Imports the reference at run time as scripts/make_aff_goldens.py does (absent optional modules stubbed, `.cuda()` a no-op).  Two kinds
of fixture, recorded data only:

  aff_loss_labels.npz   voc12.data.ExtractAffinityLabelInRadius(cropsize=s, radius=r) on seeded label maps (synth.synthetic_aff_label_map):
                        the map, its three outputs packed as bits, the three counts — 7x7 r=3, 13x13 r=5, 56x56 r=5
  aff_loss_<h>x<w>.npz  network.resnet38_aff.Net (procedural weights, eval mode, grad enabled) on synthetic images; a forward hook on f9
                        captures its pre-ELU output z (retain_grad); the three loss lines of aff_train.py:111-119 on the returned aff and
                        the extractor's labels of seeded maps; backward.  Stored: z, aff, the seven scalars, dL/dz (whole, or a recorded
                        subset of channels where the whole would exceed the fixture size), the label maps, the seeds, and the worst relative
                        deviation of the float64 restatement (tests/aff_loss_f64.py) from these float32 CPU outputs — the host test's
                        tolerance is twice that.

Every mixed-label case must hold at least MIN_PAIRS pairs of each kind (asserted), so that no term is tested on an empty sum.
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from wseg_amd import synth  # noqa: E402
from wseg_amd.resnet38_aff import pair_offsets  # noqa: E402
from make_aff_goldens import _stub_absent_modules  # noqa: E402

MIN_PAIRS = 10
# (size, radius, label seed)
LABEL_CASES = [(7, 3, 1), (13, 5, 1), (56, 5, 2)]
# (name, image size, N, image seed, label seeds, channels of dL/dz stored (None: all))
LOSS_CASES = [
    ("aff_loss_7x7", 56, 2, 81, (1, 3), None),                       # 7 x 7, radius 3
    ("aff_loss_13x13", 104, 1, 82, (3,), list(range(0, 448, 2))),     # 13 x 13, radius 5
]


def load_reference(ref):
    sys.path.insert(0, ref)
    _stub_absent_modules()
    for name in ("scipy", "scipy.misc"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                import types
                sys.modules[name] = types.ModuleType(name)
    torch.Tensor.cuda = lambda self, *a, **k: self
    import network.resnet38_aff as R
    import voc12.data as D
    return R, D


def extract(D, lab, radius):
    """the reference extractor's three outputs [P, n_from] of a square uint8 map, as numpy, with the MIN_PAIRS assertion"""
    out = [t.numpy() for t in D.ExtractAffinityLabelInRadius(cropsize=lab.shape[0], radius=radius)(lab)]
    counts = [int(o.sum()) for o in out]
    assert min(counts) >= MIN_PAIRS, f"a {lab.shape[0]}x{lab.shape[0]} map at radius {radius} has pair counts {counts}: choose another seed"
    assert out[0].shape == (len(pair_offsets(radius)), (lab.shape[0] - radius + 1) * (lab.shape[0] - 2 * radius + 2))
    return out, counts


def rel_dev(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(np.asarray(b, np.float64)).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="reference checkout (network/resnet38_aff.py, voc12/data.py)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    R, D = load_reference(args.ref)
    from tests import aff_loss_f64 as A                   # the restatement whose deviation from the reference is recorded

    rec = {"cases": np.array([[s, r, seed] for s, r, seed in LABEL_CASES], np.int64)}
    for s, r, seed in LABEL_CASES:
        lab = synth.synthetic_aff_label_map(s, s, seed).numpy()
        out, counts = extract(D, lab, r)
        key = f"{s}x{s}"
        rec[key + "_map"] = lab
        rec[key + "_bits"] = np.packbits(np.stack(out).astype(bool).reshape(3, -1), axis=1)
        rec[key + "_counts"] = np.array(counts, np.int64)
        print("labels", key, "radius", r, "seed", seed, "counts bg/fg/neg", counts, "ignored px", int((lab == 255).sum()))
    np.savez_compressed(os.path.join(args.out, "aff_loss_labels.npz"), **rec)

    model = R.Net()
    model.load_state_dict(synth.procedural_aff_state_dict(0), strict=True)
    model.eval()
    captured = {}

    def hook(_m, _i, out):
        out.retain_grad()
        captured["z"] = out

    model.f9.register_forward_hook(hook)
    for name, size, N, iseed, lseeds, chans in LOSS_CASES:
        img = synth.synthetic_images(N, size, iseed)
        with torch.enable_grad():
            aff = model(img)
            z = captured["z"]
            h, w = z.shape[2:]
            r = {7: 3, 13: 5}[h]
            maps = np.stack([synth.synthetic_aff_label_map(h, w, s).numpy() for s in lseeds])
            labels = [extract(D, m, r)[0] for m in maps]
            bg_label, fg_label, neg_label = (torch.from_numpy(np.stack([l[j] for l in labels])) for j in range(3))
            assert aff.shape == bg_label.shape
            loss, scalars = A.loss_from_aff(aff, (bg_label, fg_label, neg_label))        # aff_train.py:111-119, float32
            model.zero_grad()
            loss.backward()
        out7 = scalars.numpy().astype(np.float32)
        zv, dz = z.detach(), z.grad.detach()
        got = A.restate(F.elu(zv), torch.from_numpy(maps), r)
        dz64 = got["grad"] * A.elu_grad(zv.double())
        dev = {"aff": rel_dev(got["aff"], aff.detach()), "dz": rel_dev(dz64, dz),
               "out7": max(abs(float(got["out7"][i]) - float(out7[i])) / abs(float(out7[i])) for i in range(7))}
        sel = np.arange(448) if chans is None else np.array(chans)
        np.savez_compressed(os.path.join(args.out, name + ".npz"), size=size, N=N, radius=r, img_seed=iseed, label_seeds=np.array(lseeds, np.int64),
                            label=maps, z=zv.numpy(), aff=aff.detach().numpy(), out7=out7, dz=dz.numpy()[:, sel], dz_channels=sel.astype(np.int64),
                            dev_aff=dev["aff"], dev_out7=dev["out7"], dev_dz=dev["dz"])
        print(name, "feature map", (h, w), "radius", r, "out7", out7.tolist(), "| z range", float(zv.min()), float(zv.max()),
              "| |dz| max", float(dz.abs().max()), "| float64 restatement vs these float32 outputs, worst relative deviation:", dev)


if __name__ == "__main__":
    main()
