"""The DeepLab stage's end-to-end bars, from the reference's own runs (scripts/make_seg_envelopes.py, tests/golden/seg_*_env.npz and
seg_*_tap64.npz): the reference's net on the CPU in float64 (`c64`, the yardstick), in float32 in three vectorised orders and as one
sequential K chain per conv (`f32_a/b/c`, `f32_chain`), as the split-bf16 sum without its lo.lo term in float64 (`x3`), and in bfloat16.

Nothing here is fitted to what our kernels give.  With d(v) = max |v - c64| over the coarse cls_conv logits of every pass, and the same for
the mean logits through tests/seg_f64.py:fuse,
    fp32    SAFETY . max over the four float32 variants of d(v)                    (+ seg_f64.fuse_bar_local on the mean: our f32 collect kernel)
            SAFETY = 2 is tests/f64_bars.py's factor; the envelope holds the longest-chain float32 order of the same math, so a float32
            evaluation in our kernels' order has no reason to leave it
    bf16x3  SAFETY . d(x3) + the fp32 bar: the dropped terms summed exactly, plus float32 accumulation
    bf16    1.0 . d(bf16) on the mean logits, and no more label disagreement with float64 than the reference's bf16 run has: our mode keeps
            float32 accumulators and epilogues where that run rounds every op, so no margin factor
Labels must equal float64's wherever float64's margin is at least twice the mean bar, and the margin map lies within twice that bar.
`judge` is the one statement of these rules: the GPU tests hand it our tensors, the host tests hand it stored variants standing in for a
GPU run.  TEST INFRASTRUCTURE, no tests here."""
import os

import numpy as np
import torch

from tests import seg_f64
from tests.conftest import GOLDEN
from tests.f64_bars import SAFETY

VARIANTS = ("c64", "f32_a", "f32_b", "f32_c", "f32_chain", "x3", "bf16")
F32_ORDERS = ("f32_a", "f32_b", "f32_c")                     # the vectorised float32 orders
F32_VARIANTS = F32_ORDERS + ("f32_chain",)
_envs = {}


def passes_of(z, coarse):
    """[(coarse [21, fh, fw], (ih, iw), flip)] of seg_f64.fuse from a per-pass list, in the reference's order (plain before flipped)"""
    return [(torch.as_tensor(c), tuple(int(v) for v in z["sizes"][i // 2]), i % 2 == 1) for i, c in enumerate(coarse)]


def fuse64(z, coarse):
    return seg_f64.fuse(passes_of(z, coarse), int(z["H"]), int(z["W"]))


def coarse_dev(coarse, ref):
    """per pass max |coarse - ref|"""
    return [float((torch.as_tensor(c).double() - torch.as_tensor(r).double()).abs().max()) for c, r in zip(coarse, ref)]


def load_env(name):
    """The reference's runs of one case and what the bars are made of, computed once from the stored arrays:
      z            the float32 fixture (test_seg_host.load_case)
      coarse[v]    per pass the variant's coarse logits, float64 [21, fh, fw]
      fused[v]     seg_f64.fuse of them: mean, amax, margin ...
      d_pass[v]    per pass max |coarse[v] - coarse[c64]|;  d_coarse[v] its max;  d_mean[v] max |fused[v].mean - fused[c64].mean|
      env32_coarse / env32_mean    the max of d_coarse / d_mean over the four float32 variants
      M            max |c64 coarse logit|;  fuse_bar  seg_f64.fuse_bar_local of an f32 collect on c64's logits (fuse_bar_worst: seg_f64.fuse_bar
                   for any logits bounded by M — 0.3-0.6 x the 1e-3 max |mean logit| line, under which seg_100x125 has 1.09 % of its pixels
                   below twice the bar; the local one is 6-12 x tighter)
      tap          the <case>_tap64.npz file as a dict"""
    if name in _envs:
        return _envs[name]
    from tests.test_seg_host import load_case
    z = load_case(name)
    f = np.load(os.path.join(GOLDEN, name + "_env.npz"))
    n = int(f["n_pass"])
    assert n == int(z["n_pass"]) and tuple(str(v) for v in f["variants"]) == VARIANTS
    assert int(f["weight_seed"]) == int(z["weight_seed"]) and int(f["img_seed"]) == int(z["img_seed"])
    e = dict(z=z, coarse={v: [f[f"{v}_{i}"] for i in range(n)] for v in VARIANTS})
    assert all(c.dtype == np.float64 and c.shape == zc.shape for v in VARIANTS for c, zc in zip(e["coarse"][v], z["coarse"]))
    e["fused"] = {v: fuse64(z, e["coarse"][v]) for v in VARIANTS}
    e["d_pass"] = {v: coarse_dev(e["coarse"][v], e["coarse"]["c64"]) for v in VARIANTS}
    e["d_coarse"] = {v: max(d) for v, d in e["d_pass"].items()}
    e["d_mean"] = {v: float((e["fused"][v]["mean"] - e["fused"]["c64"]["mean"]).abs().max()) for v in VARIANTS}
    e["env32_coarse"] = max(e["d_coarse"][v] for v in F32_VARIANTS)
    e["env32_mean"] = max(e["d_mean"][v] for v in F32_VARIANTS)
    e["M"] = max(float(np.abs(c).max()) for c in e["coarse"]["c64"])
    e["fuse_bar"] = seg_f64.fuse_bar_local(passes_of(z, e["coarse"]["c64"]))
    e["fuse_bar_worst"] = seg_f64.fuse_bar(passes_of(z, e["coarse"]["c64"]), e["M"])
    e["tap"] = dict(np.load(os.path.join(GOLDEN, name + "_tap64.npz")))
    _envs[name] = e
    return e


def bars(e, mode, f32_collect=True):
    """(coarse bar, mean bar) of mode fp32 / bf16x3.  f32_collect: the mean was made by a float32 collect (our kernel) and carries
    seg_f64.fuse_bar_local; a float64 collect of stored arrays does not."""
    coarse, mean = SAFETY * e["env32_coarse"], SAFETY * e["env32_mean"] + (e["fuse_bar"] if f32_collect else 0.0)
    if mode == "bf16x3":
        coarse, mean = SAFETY * e["d_coarse"]["x3"] + coarse, SAFETY * e["d_mean"]["x3"] + mean
    else:
        assert mode == "fp32"
    return coarse, mean


def label_disagreement(e, amax):
    """share of the pixels whose label differs from float64's"""
    return float((torch.as_tensor(np.asarray(amax)).long() != e["fused"]["c64"]["amax"]).double().mean())


def judge(e, mode, coarse, mean, amax, margin, f32_collect=True, say=print):
    """The fp32 / bf16x3 rules on one run (per-pass coarse logits, mean logits [21, H, W], label map, margin map): prints ours, the bar and
    the ratio per pass, returns the list of the rules that fail (empty: the run passes)."""
    ref = e["fused"]["c64"]
    bar_c, bar_m = bars(e, mode, f32_collect)
    d = coarse_dev(coarse, e["coarse"]["c64"])
    for i, di in enumerate(d):
        say(f"  pass {i:2d} {tuple(e['coarse']['c64'][i].shape[1:])}: max |ours - c64| {di:.3e}  bar {bar_c:.3e}  ratio {di / bar_c:.3f}")
    dm = float((torch.as_tensor(mean).double() - ref["mean"]).abs().max())
    dg = float((torch.as_tensor(margin).double() - ref["margin"]).abs().max())
    unsure = ref["margin"] < 2 * bar_m
    wrong = int((torch.as_tensor(np.asarray(amax)).long() != ref["amax"])[~unsure].sum())
    say(f"  coarse {max(d):.3e} / {bar_c:.3e} = {max(d) / bar_c:.3f}   mean {dm:.3e} / {bar_m:.3e} = {dm / bar_m:.3f}   margin {dg:.3e} / "
        f"{2 * bar_m:.3e}   excluded {float(unsure.double().mean()):.3%}   labels wrong outside {wrong}")
    failed = []
    if not max(d) <= bar_c:
        failed.append("coarse")
    if not dm <= bar_m:
        failed.append("mean")
    if not float(unsure.double().mean()) <= 0.01:
        failed.append("excluded share")
    if wrong:
        failed.append("labels")
    if not dg <= 2 * bar_m:
        failed.append("margin")
    return failed


def tap_bar(e, mode, i):
    """the bar on max |our backbone output - tap64| of tapped pass i, from the stored scalar envelopes"""
    t = e["tap"]
    f32 = SAFETY * float(t[f"dev_f32_chain_{i}"])
    return {"fp32": f32, "bf16x3": SAFETY * float(t[f"dev_x3_{i}"]) + f32, "bf16": 1.0 * float(t[f"dev_bf16_{i}"])}[mode]
