"""tests/trunk_f64.py on the CPU: what the float64 stage references are pinned to, and what their bars catch.
  1. restatement pin: the stage functions chained on their own outputs in float64 reproduce oracle.net.backbone in float64 (conv4, conv5, conv6,
     autograd's gradient of every trainable trunk weight, and the gradient that arrives at b5's / b6's raw input with taps on conv4 / conv5) to
     1e-10 relative, with five dropout sites (the contrast net) and with four (the AffinityNet backbone).
  2. honest emulation: the same chain in float32 / split-bf16 / bf16 arithmetic with rounded stores (trunk_f64.Emu) is inside every stage bar
     in every mode; the worst err / bar per stage kind is printed.
  3. planted wiring defects: each one, put into the one stage it concerns, leaves at least one stage bar — and already in float64 (no
     rounding) it differs from the reference by more than the bar, so the procedural state dict and the inputs used tell the two wirings apart."""
import pytest
import torch

from oracle import net as onet
from tests import trunk_f64 as T
from tests.f64_bars import _gen
from wseg_amd import synth

VIEWS = ((40, 24), (24, 16))         # stride-8 maps 5 x 3 and 3 x 2
N = 2
FUSED = {"fp32": (), "bf16x3": (), "bf16": ("b5", "b6", "b7")}      # the blocks whose skip conv rides in the last conv's launch
_cache = {}


def _bf16_values(shape, seed):
    return (torch.rand(shape, generator=_gen(seed)) * 2 - 1).bfloat16().double()


def _masks(n, views, seed, sites=5):
    per_view = [synth.synthetic_dropout_masks(n, seed + i) for i in range(views)]
    keys = list(per_view[0])[:sites]
    return {k: torch.cat([m[k] for m in per_view]).double() for k in keys}


def _inputs():
    """images, dropout tables and the backward's inputs of the emulation runs: D at b7's x_out, taps on b5 and b6 (bf16 values)"""
    if "in" not in _cache:
        xs = [synth.synthetic_images(N, hw, 3 + i) for i, hw in enumerate(VIEWS)]
        dims = {"b5": T.out_dims(VIEWS, 3, 2, 1)}
        for _ in range(2):
            dims["b5"] = T.out_dims(dims["b5"], 3, 2, 1)
        M = sum(N * h * w for h, w in dims["b5"])
        _cache["in"] = dict(xs=xs, masks=_masks(N, len(VIEWS), 40), D=_bf16_values((M, 4096), 50),
                            taps={"b5": _bf16_values((M, 512), 51), "b6": _bf16_values((M, 1024), 52)})
    return _cache["in"]


def _honest(proc_sd, mode):
    """(record of the honest emulation, weights, folds) of a mode, computed once"""
    if mode not in _cache:
        i = _inputs()
        W = T.weights64(T.trunk_params(proc_sd), mode)
        bn = {}
        for name in T.bn_names():
            got, ref, bar = T.fold32(proc_sd, name), T.fold64(proc_sd, name), T.fold_bar(proc_sd, name)
            for g, r, b in zip(got, ref, bar):
                assert bool(((g.double() - r).abs() <= b).all()), name
            bn[name] = tuple(g.double() for g in got)
        rec = T.run_chain(T.Emu(mode), i["xs"], W, bn, i["masks"], fused=FUSED[mode], D=i["D"], taps=i["taps"])
        _cache[mode] = (rec, W, bn)
    return _cache[mode]


# ------------------------------------------------------------------------------------------------------------------ 1. the pin
@pytest.mark.parametrize("sites", [5, 4])
def test_chain_reproduces_the_oracle_in_float64(proc_sd, sites):
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in proc_sd.items()}
    for k in onet.trainable_keys(sd):
        sd[k].requires_grad_(True)
    x = synth.synthetic_images(1, (40, 24), 5).double()
    masks = _masks(1, 1, 60, sites)
    out = onet.backbone(x, sd, masks)
    for k in ("conv4", "conv5"):
        out[k].retain_grad()
    fea = onet._drop(out["conv6"], masks, "dropout7") if sites == 5 else out["conv6"]
    G = {k: torch.rand(out[k].shape, generator=_gen(70 + i), dtype=torch.float64) * 2 - 1 for i, k in enumerate(("conv4", "conv5", "conv6"))}
    (G["conv4"] * out["conv4"]).sum().add((G["conv5"] * out["conv5"]).sum()).add((G["conv6"] * fea).sum()).backward()

    W = {k: v.detach() for k, v in T.trunk_params(sd).items()}
    bn = {name: T.fold64(sd, name) for name in T.bn_names()}
    A = T.Exact()
    fwd = T.run_chain(A, [x], W, bn, masks)
    fea_rows = fwd["b7"]["t_out"]
    dims8 = T.block_dims("b7", fwd["b7"]["dims"])
    D = T.to_rows([G["conv6"]]) * bn["bn7"][0] * (fea_rows > 0)
    if sites == 5:
        D = D * masks["dropout7"][T.img_index(1, dims8)]
    rec = T.run_chain(A, [x], W, bn, masks, D=D, taps={"b5": T.to_rows([G["conv4"]]), "b6": T.to_rows([G["conv5"]])})

    def close(tag, got, ref):
        rel = float((got - ref).abs().max() / ref.abs().max())
        print(f"{tag}: {rel:.2e}")
        assert rel <= 1e-10, (tag, rel)

    close("conv4", rec["b5"]["t"], T.to_rows([out["conv4"].detach()]))
    close("conv5", rec["b6"]["t"], T.to_rows([out["conv5"].detach()]))
    close("conv6", fea_rows, T.to_rows([fea.detach()]))
    for blk, key in (("b5", "conv4"), ("b6", "conv5")):      # dL/dt of the tapped block (autograd: the tap included) through its mask . scale
        t = out[key].detach()
        want = out[key].grad * bn[blk + ".bn_branch2a"][0].view(1, -1, 1, 1) * (t > 0)
        close(f"{blk}.D_in", rec[blk]["D_in"], T.to_rows([want]))
    seen = 0
    for k in onet.trainable_keys(sd):
        if k.split(".")[0] not in T.BLOCKS:
            continue                                           # (the heads' weights)
        blk, conv = k[:-len(".weight")].split(".conv_branch")
        close(k, rec[blk]["dW_" + conv], sd[k].grad)
        seen += 1
    assert seen == 35                                          # every conv of b3 .. b7
    for blk in T.FROZEN:
        assert "D" not in rec[blk]


# ------------------------------------------------------------------------------------------------------------------ 2. the honest emulation
@pytest.mark.parametrize("mode", list(T.MODES))
def test_honest_emulation_is_inside_every_bar(proc_sd, mode):
    rec, W, bn = _honest(proc_sd, mode)
    table = T.judge(mode, rec, W, bn, _inputs()["masks"], N)
    for kind, (ratio, tag) in sorted(T.worst(table).items()):
        print(f"[{mode}] worst {kind:8s} err / bar {ratio:.4f} at {tag}")
    assert len(table) > 100 and all(ok for *_x, ok in table), [row for row in table if not row[3]]
    kinds = {tag.split(".")[-1] for tag, *_x in table}
    assert kinds >= {"t_out", "v", "v1", "v2", "x_out", "du", "du2", "du1", "D_in", "dW_2a", "dW_2b1", "dW_2b2", "dW_1"}
    tags = {tag for tag, *_x in table}                       # b5, b6, b7: the skip conv's output is a stage of its own outside bf16 mode only
    assert {"b4.rpost", "b4.tmp"} <= tags and all((t_ in tags) == (mode != "bf16") for t_ in ("b5.rpost", "b5.tmp", "b6.tmp", "b7.tmp"))


# ------------------------------------------------------------------------------------------------------------------ 3. planted wiring defects
DEFECTS = {      # defect: (block, pass)
    "swap_scale": ("b4_1", "bwd"),                # s_2b1 in place of s_2a in the data gradient (both 512 wide)
    "mask_from_v": ("b4_1", "bwd"),               # (v > 0) in place of (t > 0)
    "tap_after_mask": ("b5", "bwd"),
    "other_dropout": ("b7", "bwd"),               # b6.dropout_2b2's factors (1024 wide) at b7.dropout_2b1
    "residual_before_mask": ("b4_1", "bwd"),
    "short_skip": ("b5", "fwd"),                  # the skip piece of the K-concatenated pack eight input columns short
    "no_skip_wgrad": ("b5", "bwd"),
    "dropout7_twice": ("b7", "fwd"),
}


@pytest.mark.parametrize("mode", list(T.MODES))
@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defect_leaves_a_bar(proc_sd, defect, mode):
    rec, W, bn = _honest(proc_sd, mode)
    masks = _inputs()["masks"]
    blk, which = DEFECTS[defect]
    r = rec[blk]
    fn = T.block_forward if which == "fwd" else T.block_backward
    kw = dict(fused=blk in FUSED[mode], defect=defect)
    bad = fn(T.Emu(mode), blk, r, W, bn, masks, N, r["dims"], **kw)
    table = T.judge(mode, {blk: {**r, **bad}}, W, bn, masks, N, forward=which == "fwd", backward=which == "bwd")
    out = [(tag, ratio) for tag, _e, ratio, ok in table if not ok]
    print(f"[{mode}] {defect}: outside at {out}")
    assert out, (defect, mode, table)
    # the two wirings differ by more than the bar before any rounding: float64 with the defect against the reference and its bar
    ref = fn(T.Ref(mode), blk, r, W, bn, masks, N, r["dims"], fused=blk in FUSED[mode])
    exact = fn(T.Exact(), blk, r, W, bn, masks, N, r["dims"], **kw)
    apart = {st: float(((exact[st] - ref[st][0]).abs() / ref[st][1]).max()) for st in exact}
    print(f"[{mode}] {defect}: float64 distance / bar {({k: round(v, 1) for k, v in apart.items() if v > 1})}")
    assert max(apart.values()) > 1.0
    if defect == "swap_scale":
        s_a, s_b = bn[blk + ".bn_branch2a"][0], bn[blk + ".bn_branch2b1"][0]
        assert float(((s_a - s_b).abs() / s_a.abs()).min()) > 0 and float(((s_a - s_b).abs() / s_a.abs()).median()) > 0.05
