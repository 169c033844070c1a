"""tests/head_f64.py on the CPU: what the float64 stage references of the contrast head are pinned to, and what their bars catch, at the
geometry of tests/test_gpu_head_stages.py (two views 100 x 76 and 44 x 28, N = 2: 308 stride-8 rows, PCM maps 13 x 10 and 6 x 4).
  1. pin: the Exact stages chained on an oracle.net.backbone run in float64 reproduce oracle.net.net_forward(return_lowres=True) per view, and
     the chained backward autograd's gradients of a fixed functional of the four outputs for f9, f8_3, f8_4, fc8, fc_proj and the input of
     bn7 (the conv6 tap), to 1e-10 relative.
  2. honest kernel: the same chain in float32 / split-bf16 / bf16 arithmetic with rounded stores (trunk_f64.Emu) is inside every stage bar in
     every mode; the worst err / bar per tensor is printed.
  3. planted wiring defects: the chain with ONE defect leaves the bar of the stage named and of no stage in front of it.
     The defect that drops Gl from the PCM backward's gate product (bf16 mode) runs under a gradient COMMON TO ALL CLASSES, g_rvd = 1 + noise /
     16: t_ij = sum_c g_ic (G_jc - rvd_ic) / D_i then cancels (the gate's and rvd's 21 classes each sum to 1), which is what the split product
     exists for; Gl's 2^-9 |G| does not cancel, and dFh leaves its bar by a factor of 6.  Under gradients of random sign per class the same
     defect stays inside the bar (0.58 of it, the honest kernel 0.32): there the bar's allowance for the kernel's own bf16 rounding of W,
     2^-8 |t| per pair, is as large as all of Gl.  The honest kernel is judged under the common gradient too.
  4. band and near-tie conditions for the inputs the GPU test uses (the same image and dropout seeds; the values differ from the device's by
     rounding only): the share of PCM pairs inside the gate band stays within BAND_CAP, and cam_gate's kept entries differ from float64's
     at near-ties only (a decision outside the rule is judged outside the bar of G)."""
import pytest
import torch

from oracle import net as onet
from tests import head_f64 as H
from tests import trunk_f64 as T
from tests.f64_bars import _gen
from wseg_amd import synth

VIEWS = ((100, 76), (44, 28))
ONE_VIEW = ((84, 60),)
N = 2
IMG_SEED, MASK_SEED = 7, 40           # view i: synthetic_images(N, size, IMG_SEED + i), synthetic_dropout_masks(N, MASK_SEED + i)
_cache = {}


def _sd64(proc_sd):
    if "sd" not in _cache:
        _cache["sd"] = {k: (v.double() if v.is_floating_point() else v) for k, v in proc_sd.items()}
    return _cache["sd"]


def _rand(shape, seed):
    return torch.rand(shape, generator=_gen(seed), dtype=torch.float64) * 2 - 1


def _base(proc_sd, views):
    """the float64 inputs of the head at `views`: images, masks, fea / conv4 / conv5 rows of an oracle.net.backbone run, s7, drop7, and the
    gradients of the four outputs per view"""
    if views not in _cache:
        sd = _sd64(proc_sd)
        xs = [synth.synthetic_images(N, hw, IMG_SEED + i) for i, hw in enumerate(views)]
        masks = [{k: v.double() for k, v in synth.synthetic_dropout_masks(N, MASK_SEED + i).items()} for i in range(len(views))]
        maps = {"fea": [], "conv4": [], "conv5": []}
        with torch.no_grad():
            for x, m in zip(xs, masks):
                d = onet.backbone(x.double(), sd, m)
                maps["fea"].append(onet._drop(d["conv6"], m, "dropout7")); maps["conv4"].append(d["conv4"]); maps["conv5"].append(d["conv5"])
        dims = [tuple(t.shape[2:]) for t in maps["fea"]]
        g = [(_rand((N, 21) + hw, 80 + 10 * i), _rand((N, 21) + hw, 81 + 10 * i), _rand((N, 128) + d_, 82 + 10 * i), _rand((N, 21) + d_, 83 + 10 * i))
             for i, (hw, d_) in enumerate(zip(views, dims))]
        _cache[views] = dict(xs=xs, masks=masks, dims=dims, g=g, s7=T.fold64(sd, "bn7")[0], drop7=torch.cat([m["dropout7"] for m in masks]),
                             **{k: T.to_rows(v) for k, v in maps.items()})
    return _cache[views]


def common_gradient(g):
    """(g_cam, g_cam_rv, g_fproj, g_rvd) of random values -> the same with g_rvd = 1 + g_rvd / 16 for every class and g_cam_rv / 64 (bf16 values):
    a gradient common to all classes, under which the gate product of the PCM backward cancels"""
    bf = lambda t: t.float().bfloat16().to(t.dtype)
    return (g[0], bf(g[1] / 64), g[2], bf(1 + g[3] / 16))


def _record(proc_sd, views, mode, common=False):
    """the inputs as `mode` holds them: activations rounded to its storage format, gradients of the outputs to f32, bn7's scale the f32 fold"""
    b = _base(proc_sd, views)
    if common:
        b = dict(b, g=[common_gradient(g) for g in b["g"]])
    rnd = (lambda t: t.float().bfloat16().double()) if mode == "bf16" else (lambda t: t.float().double())
    f32 = lambda t: t.float().double()
    return dict(N=N, dims=b["dims"], xs=b["xs"], lowres=False, fea=rnd(b["fea"]), conv4=rnd(b["conv4"]), conv5=rnd(b["conv5"]),
                s7=T.fold32(proc_sd, "bn7")[0].double(), drop7=b["drop7"], g=[tuple(f32(t) for t in gv) for gv in b["g"]])


def _weights(proc_sd, mode):
    return H.weights64({n: proc_sd[n + ".weight"] for n in H.HEAD_CONVS}, mode)


def _honest(proc_sd, mode, views=VIEWS, common=False):
    key = ("honest", mode, views, common)
    if key not in _cache:
        W = _weights(proc_sd, mode)
        _cache[key] = (H.run_chain(T.Emu(mode), _record(proc_sd, views, mode, common), W, mode, backward=True), W)
    return _cache[key]


# ------------------------------------------------------------------------------------------------------------------ 1. the pin
def test_chain_reproduces_the_oracle_in_float64(proc_sd, monkeypatch):
    sd = dict(_sd64(proc_sd))
    for n in H.HEAD_CONVS:
        sd[n + ".weight"] = sd[n + ".weight"].clone().requires_grad_(True)
    b = _base(proc_sd, VIEWS)
    taps, bn0 = [], onet._bn

    def bn(x, sd_, p):                  # the input of bn7 becomes a leaf: autograd's gradient there is the conv6 tap
        if p == "bn7":
            x = x.detach().requires_grad_(True)
            taps.append(x)
        return bn0(x, sd_, p)

    monkeypatch.setattr(onet, "_bn", bn)
    outs, loss = [], 0
    for x, m, g in zip(b["xs"], b["masks"], b["g"]):
        cam, cam_rv, f_proj, rvd, cam_low = onet.net_forward(x.double(), sd, m, return_lowres=True)
        outs.append(dict(cam=cam, cam_rv=cam_rv, f_proj=f_proj, rvd=rvd, cam_low=cam_low))
        loss = loss + (g[0] * cam).sum() + (g[1] * cam_rv).sum() + (g[2] * f_proj).sum() + (g[3] * rvd).sum()
    loss.backward()

    W = {n: sd[n + ".weight"].detach()[:, :, 0, 0] for n in H.HEAD_CONVS}
    r = dict(N=N, dims=b["dims"], xs=b["xs"], lowres=False, g=b["g"], s7=b["s7"], drop7=b["drop7"], fea=b["fea"], conv4=b["conv4"], conv5=b["conv5"])
    rec = H.run_chain(T.Exact(), r, W, "fp32", backward=True)

    def close(tag, got, ref):
        rel = float((got - ref).abs().max() / ref.abs().max())
        print(f"{tag}: {rel:.2e}")
        assert rel <= 1e-10, (tag, rel)

    for i, ((off, n, h, w), o) in enumerate(zip(H.view_rows(N, b["dims"]), outs)):
        for k in ("cam", "cam_rv", "rvd", "cam_low"):
            close(f"{k}.v{i}", rec[k][i], o[k].detach())
        close(f"f_proj.v{i}", H.planes(rec["head"][off:off + n, :128], N, h, w), o["f_proj"].detach())
        assert bool((rec["head"][:, 149:] == 0).all()) and bool((rec["feat"][:, 195:] == 0).all())
    for n in H.HEAD_CONVS:
        close("dW_" + n, rec["dW_" + n], sd[n + ".weight"].grad[:, :, 0, 0])
    assert len(taps) == len(VIEWS)
    close("D", rec["D"], T.to_rows([t.grad for t in taps]))


# ------------------------------------------------------------------------------------------------------------------ 2. the honest kernel
@pytest.mark.parametrize("mode", list(T.MODES))
def test_honest_emulation_is_inside_every_bar(proc_sd, mode):
    rec, W = _honest(proc_sd, mode)
    info = {}
    table = H.judge(mode, rec, W, info=info)
    for k, (ratio, tag) in sorted(H.worst(table).items()):
        print(f"[{mode}] worst {k:12s} err / bar {ratio:.4f} at {tag}")
    print(f"[{mode}] pairs inside the gate band {info['band']} of {info['pairs']}; gate decisions other than float64's {info['gate_differs']} of {info['gate_entries']}")
    assert all(ok for *_x, ok in table), [row for row in table if not row[3]]
    want = {"head", "feat", "cam_low", "cmax", "G", "Fm", "Fh", "nrm", "rvd", "den", "cam", "cam_rv", "d_cam_low", "dr", "d_rvd", "DN", "dFh", "dF",
            "dW_f9", "d_feat", "dW_f8_3", "dW_f8_4", "d_head_rows", "dW_fc_proj", "dW_fc8", "D"} | ({"Fb", "Gb", "Gl", "DNb", "DNl"} if mode == "bf16" else set())
    assert {tag.split(".")[0] for tag, *_x in table} == want


@pytest.mark.parametrize("mode", list(T.MODES))
@pytest.mark.parametrize("views", [VIEWS, ONE_VIEW])
def test_honest_emulation_under_a_gradient_common_to_all_classes(proc_sd, views, mode):
    """the PCM branch of the backward where its gate product cancels (common_gradient): inside every bar, nothing in the gate band"""
    rec, W = _honest(proc_sd, mode, views, common=True)
    info = {}
    table = H.judge(mode, rec, W, forward=False, info=info, only=("d_cam_low", "DN", "dF", "dW_f9", "d_feat", "dW_f8_3", "dW_f8_4"))
    for k, (ratio, tag) in sorted(H.worst(table).items()):
        print(f"[{mode}] worst {k:12s} err / bar {ratio:.4f} at {tag}")
    assert all(ok for *_x, ok in table), [row for row in table if not row[3]]
    assert info["band"] <= H.BAND_CAP * info["pairs"], info


# ------------------------------------------------------------------------------------------------------------------ 3. planted wiring defects
COMMON = ("gate_without_lo",)      # the defects that run under common_gradient
DEFECTS = {      # defect: (the row of the stage table it must fail at, the modes it exists in)
    "G_other_view": ("rvd", T.MODES),                 # view 2's G rows read at view 1's offset
    "f8_4_at_col0": ("feat", T.MODES),                # f8_4 written at column 0 instead of 64
    "xs_align_false": ("feat", T.MODES),              # x_s with align_corners=False
    "f9_no_rotation": ("Fm", T.MODES),                # the f9 forward pack without its rotation
    "no_dw_rot": ("dW_f9", T.MODES),                  # dW_f9 without dw_rot
    "d_feat_ungated": ("d_feat", T.MODES),            # d_feat not gated by feat > 0
    "f8_4_dy_at_col0": ("dW_f8_4", T.MODES),          # dW_f8_4 read from d_feat[:, 0:]
    "D_without_dropout7": ("D", T.MODES),
    "D_without_s7": ("D", T.MODES),
    "head_relu_dropped": ("d_head_rows", T.MODES),    # the ReLU gate of d_head_rows dropped
    "fc_rows_swapped": ("dW_fc8", T.MODES),           # the rows of fc8 and fc_proj swapped in the 149-row block
    "gate_without_lo": ("DN", ("bf16",)),             # the gate product of the PCM backward with Gb alone (no Gl)
}


@pytest.mark.parametrize("defect,mode", [(d, m) for d, (_row, modes) in DEFECTS.items() for m in modes])
def test_planted_defect_leaves_the_bar_of_its_stage(proc_sd, defect, mode):
    """The whole chain runs with the one defect, so every later stage is computed from what the defective stage stored: only the stage named may
    leave its bar."""
    row = DEFECTS[defect][0]
    W = _weights(proc_sd, mode)
    rec = H.run_chain(T.Emu(mode), _record(proc_sd, VIEWS, mode, defect in COMMON), W, mode, backward=True, defects={row: defect})
    upto = H.ROW_ORDER[:H.ROW_ORDER.index(row) + 1]
    table = H.judge(mode, rec, W, only=upto)
    out = [(tag, ratio) for tag, _e, ratio, ok in table if not ok]
    print(f"[{mode}] {defect}: outside at {out}")
    assert out and {H.row_of(tag) for tag, _r in out} == {row}, (defect, mode, out)


# ------------------------------------------------------------------------------------------------------------------ 4. band and near-ties
@pytest.mark.parametrize("mode", list(T.MODES))
@pytest.mark.parametrize("views", [VIEWS, ONE_VIEW])
def test_band_and_gate_conditions_for_the_gpu_seeds(proc_sd, views, mode):
    rec, W = _honest(proc_sd, mode, views)
    info = {}
    table = H.judge(mode, rec, W, info=info, only=("G", "DN"))
    share = info["band"] / info["pairs"]
    print(f"[{mode} {views}] pairs inside the gate band: {info['band']} of {info['pairs']} ({100 * share:.4f} %); "
          f"gate decisions other than float64's: {info['gate_differs']} of {info['gate_entries']}")
    assert share <= H.BAND_CAP, share
    assert all(ok for *_x, ok in table), [row for row in table if not row[3]]
