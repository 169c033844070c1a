#!/usr/bin/env python
"""Generate tests/golden/aff_train_*.npz by running the REFERENCE's AffinityNet in TRAINING mode, its label extractor, the loss lines of
aff_train.py:111-119 and its own PolyOptimizer for two consecutive steps on the CPU (build container only).

  python scripts/make_aff_train_goldens.py --ref <reference checkout> [--out tests/golden] [--probe]

Imports the reference at run time as scripts/make_aff_loss_goldens.py does (absent optional modules stubbed, `.cuda()` a no-op); recorded
data only.  network.resnet38_aff.Net with procedural weights (synth.procedural_aff_state_dict) in .train() mode; its four Dropout2d sites
(b6 / b7 dropout_2b1, dropout_2b2) are replaced by injected masks through forward hooks, as oracle/make_goldens.py does for the contrast
net; voc12.data.ExtractAffinityLabelInRadius labels of synth.synthetic_aff_label_map maps (at least MIN_PAIRS pairs of each kind,
asserted); tool.torchutils.PolyOptimizer built as aff_train.py:72-78 builds it (groups taken before .train()).  Two steps, so that the
momentum buffer's first-step branch and the poly lr both show.

Stored per step s: the seven scalars `s<s>/<name>`, gradient slices and norms `gslice<s>/<key>`, `gnorm<s>/<key>` and the weight slices
after the step `wslice<s>/<key>` of tests/aff_train_ref.GRAD_KEYS (a strided slice of aff_train_ref.SLICE samples), the seeds, and the names
and defaults of aff_train.py's argparse flags (read from its source text: the CLI test compares its own parser with them).

lr: the rule of step_S128_N3_x3: the largest of 3e-2, 3e-3, 3e-4, 3e-5, 3e-6 at which the random procedural weights keep every loss
term alive — after the first update every term of the second step is finite and none has grown beyond twice its first-step value.
`--probe` prints the second step's scalars for each candidate.
"""
import argparse
import ast
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from wseg_amd import synth  # noqa: E402
from make_aff_loss_goldens import MIN_PAIRS, extract, load_reference  # noqa: E402,F401
from tests import aff_train_ref as A  # noqa: E402

LR_CANDIDATES = (3e-2, 3e-3, 3e-4, 3e-5, 3e-6)
WT_DEC, MAX_STEP, STEPS = 5e-4, 10, 2
# (name, image size, N, image seed, mask seed, label seeds per step)
CASES = [
    ("aff_train_64_N2", 64, 2, 91, 93, ((1, 3), (5, 6))),     # 8 x 8 map, radius 3 (below the 2 * 5 + 1 edge rule)
    ("aff_train_104_N1", 104, 1, 92, 95, ((3,), (5,))),         # 13 x 13 map, radius 5
]


def install_masks(model, mask_sets):
    """forward hooks that replace each Dropout2d output by input * injected mask; one mask set per forward of the model"""
    state = {"call": 0}
    for key in A.MASK_SITES:
        blk, site = key.split(".")

        def hook(_m, inp, _out, key=key):
            m = mask_sets[state["call"]][key]
            return inp[0] * m.view(m.shape[0], m.shape[1], 1, 1)
        getattr(getattr(model, blk), site).register_forward_hook(hook)
    model.register_forward_hook(lambda *_a: state.__setitem__("call", state["call"] + 1))


def cli_flags(ref):
    """[(flag, default or None, required)] of the reference's aff_train.py, from its source text"""
    tree = ast.parse(open(os.path.join(ref, "aff_train.py")).read())
    out = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument":
            kw = {k.arg: ast.literal_eval(k.value) for k in node.keywords if k.arg in ("default", "required")}
            out.append((ast.literal_eval(node.args[0]), kw.get("default"), bool(kw.get("required", False))))
    return out


def run_case(R, D, torchutils, case, lr, sd0):
    name, size, N, iseed, mseed, lseeds = case
    model = R.Net()
    model.load_state_dict(sd0, strict=True)
    groups = model.get_parameter_groups()                            # before .train(), as aff_train.py:72
    opt = torchutils.PolyOptimizer([
        {'params': groups[0], 'lr': lr, 'weight_decay': WT_DEC},
        {'params': groups[1], 'lr': 2 * lr, 'weight_decay': 0},
        {'params': groups[2], 'lr': 10 * lr, 'weight_decay': WT_DEC},
        {'params': groups[3], 'lr': 20 * lr, 'weight_decay': 0}], lr=lr, weight_decay=WT_DEC, max_step=MAX_STEP)
    model.train()
    install_masks(model, [A.aff_masks(N, mseed + s_) for s_ in range(STEPS)])
    params = dict(model.named_parameters())
    rec, scal = {}, []
    for s_ in range(STEPS):
        aff = model(synth.synthetic_images(N, size, iseed + s_))
        h = w = size // 8
        r = {8: 3, 13: 5}[h]
        maps = [synth.synthetic_aff_label_map(h, w, ls).numpy() for ls in lseeds[s_]]
        labels = [extract(D, m, r)[0] for m in maps]
        loss, out7 = A.loss_lines(aff, tuple(torch.from_numpy(np.stack([l[j] for l in labels])) for j in range(3)))
        opt.zero_grad()
        loss.backward()
        for k in A.GRAD_KEYS:
            rec[f"gslice{s_}/{k}"] = A.slice_of(params[k].grad).numpy().copy()
            rec[f"gnorm{s_}/{k}"] = np.array(params[k].grad.double().norm().item())
        opt.step()
        for k in A.GRAD_KEYS:
            rec[f"wslice{s_}/{k}"] = A.slice_of(params[k]).numpy().copy()
        for i, k in enumerate(A.STATS):
            rec[f"s{s_}/{k}"] = np.array(float(out7[i]))
        scal.append(out7.tolist())
    for k, p in params.items():                                      # the frozen prefix and every BatchNorm never move
        if k.startswith(("conv1a", "b2.", "b2_1.", "b2_2.")) or "bn" in k:
            assert torch.equal(p.detach(), sd0[k]), k
    rec.update(n=N, size=size, seed=iseed, steps=STEPS, lr=lr, wt_dec=WT_DEC, max_step=MAX_STEP, h=h, w=w, radius=r,
               mask_seeds=np.array([mseed + s_ for s_ in range(STEPS)], np.int64), label_seeds=np.array(lseeds, np.int64),
               lr_final=np.array([g_["lr"] for g_ in opt.param_groups]))
    return rec, scal


def alive(scal):
    s0, s1 = np.array(scal[0][:4]), np.array(scal[1][:4])
    return bool(np.isfinite(s1).all() and (s1 <= 2 * s0).all() and (s1 > 0).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="reference checkout (aff_train.py, network/, voc12/, tool/)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--probe", action="store_true", help="print the second step's scalars per lr candidate and stop")
    args = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    R, D = load_reference(args.ref)
    from tool import torchutils
    sd0 = synth.procedural_aff_state_dict(0)
    lr = None
    for cand in LR_CANDIDATES:
        ok = True
        for case in CASES:
            _rec, scal = run_case(R, D, torchutils, case, cand, sd0)
            print("probe", case[0], "lr", cand, "step 0", [round(v, 5) for v in scal[0][:4]], "step 1", [round(v, 5) for v in scal[1][:4]], "alive", alive(scal))
            ok = ok and alive(scal)
        if ok and lr is None:
            lr = cand
            if not args.probe:
                break
    assert lr is not None, "no lr candidate keeps the loss terms alive"
    print("lr", lr)
    if args.probe:
        return
    flags = cli_flags(args.ref)
    for case in CASES:
        rec, scal = run_case(R, D, torchutils, case, lr, sd0)
        rec.update(cli_flags=np.array([f for f, _d, _r in flags]), cli_defaults=np.array(["" if d is None else repr(d) for _f, d, _r in flags]),
                   cli_required=np.array([r for _f, _d, r in flags]))
        path = os.path.join(args.out, case[0] + ".npz")
        np.savez_compressed(path, **rec)
        print("wrote", path, os.path.getsize(path), "bytes; scalars", scal)


if __name__ == "__main__":
    main()
