"""tests/loss_f64.py on the CPU: what the float64 stage references of the loss phase are pinned to, and what their bars catch, at the
geometries of tests/test_gpu_loss_stages.py (case A: 104 x 104 -> 13 x 13 and 128 x 128 -> 16 x 16, N = 2, seventeen classes absent; case B:
160 x 160 -> 20 x 20 and 128 x 128, N = 3, one image with all twenty classes).  The inputs here are the three tensors per view the loss phase
reads — cam_low, rvd >= 0 (what the PCM gives), the head rows — drawn procedurally and rounded as each mode stores them.
  1. pin: the stages chained in float64 reproduce oracle.loss.step_loss on the same forward 4-tuples (cam = upsample(cam_low),
     cam_rv = upsample(rvd), f_proj = relu(head rows), cam_rv_down = rvd): all eight scalars, and autograd's gradients with respect to cam_low,
     rvd and the head rows' pre-activation as d_cam_low, d_rvd and d_head, to 1e-10 relative.  The hard-pixel weights of the pin come from the
     selections the oracle records (sel1 / sel2); the weight stages themselves are pinned to the sampling rule on the same records, both by
     the key rule and by the RNG-parity rule.
  2. honest emulation: the same chain in float32 with rounded stores (split-bf16 record operands and bf16 head rows / d_head where the mode
     has them) is inside every stage bar in every mode.
  3. planted wiring defects: the chain with ONE defect leaves the bar of the stage named and of no stage in front of it.  Not planted: the
     relu flag of the min-pool select_finish — on rvd >= 0 every q is >= 0, the flag changes nothing and no test can see it.
  4. conditions for the GPU test's inputs are checked by that test on the device's own tensors (tests.loss_f64.conditions); here the same
     conditions are asserted for the procedural inputs, so the caps are known to be reachable: undecided rank-band pixels <= 2 % per view,
     pseudo-label and top-32 near-ties leave >= 98 % of every stage judged, no exact tie at the ECR and min-pool thresholds."""
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import loss as oloss
from tests import loss_f64 as LF
from tests.f64_bars import _gen

MODES = ("fp32", "bf16x3", "bf16")
CASES = {"A": dict(N=2, S=(104, 128), labels=[[4], [1, 7, 14]], seed=3),
         "B": dict(N=3, S=(160, 128), labels=[list(range(20)), [2, 9], [0, 5, 11, 17, 19]], seed=5)}
BG = 0.20
_cache = {}


def label_rows(labels):
    lab = torch.zeros(len(labels), 20, dtype=torch.float64)
    for n, cl in enumerate(labels):
        lab[n, cl] = 1.0
    return lab


def _inputs(case, mode):
    """the record's inputs as `mode` stores them (cam_low, rvd, keys f32; head rows bf16 in bf16 mode)"""
    c = CASES[case]
    N, g = c["N"], _gen(c["seed"])
    views, off = [], 0
    for i, S in enumerate(c["S"]):
        h = w = (S + 7) // 8
        # a latent class per stride-8 pixel ties rvd to the head rows, as a trained net does: each class's strongest rvd pixels carry that
        # class's feature pattern, so the prototypes differ and the similarities spread (independent draws give 21 near-equal prototypes
        # and 3 % of the pixels an undecided rank band)
        z = torch.randint(0, 21, (N, h, w), generator=g)
        pattern = torch.randn(21, 128, generator=g)
        head = torch.randn(N * h * w, LF.HEAD_LD, generator=g) * 0.5
        head[:, :128] += pattern[z.view(-1)]
        head = head.clamp_min(0)
        head[:, 149:] = 0
        head = head.bfloat16() if mode == "bf16" else head
        rvd = torch.rand(N, 21, h, w, generator=g) ** 2 * 0.6 + 0.8 * F.one_hot(z, 21).permute(0, 3, 1, 2) * torch.rand(N, 21, h, w, generator=g)
        views.append(dict(S=S, h=h, w=w, off=off, cam_low=(torch.randn(N, 21, h, w, generator=g) * 0.8).double(), rvd=rvd.double(),
                          head=head.double(), rkey=torch.rand(N * 256, generator=g).double()))
        off += N * h * w
    P = N * 256
    tie = torch.topk(torch.full((21, P), 0.2, dtype=torch.float64), 32, dim=-1)[1][0]
    return dict(N=N, label20=label_rows(c["labels"]), bg=BG, tie=tie, M=off, views=views)


def _honest(case, mode):
    if (case, mode) not in _cache:
        _cache[(case, mode)] = LF.run_chain(_inputs(case, mode), torch.float32, mode)
    return _cache[(case, mode)]


def _print(tag, table):
    for k, (ratio, where) in sorted(LF.worst(table).items()):
        print(f"[{tag}] worst {k:24s} err / bar {ratio:.4f} at {where}")


# ------------------------------------------------------------------------------------------------------------------ 1. the pin
def weights_from_selections(y, sel):
    """the hard-pixel weights of one view from the oracle's recorded selections [(class, random positions, rank-band positions)]"""
    yn = y.numpy()
    w = np.zeros(len(yn))
    C = len(np.unique(yn))
    for cls, ridx, lidx in sel:
        members = np.nonzero(yn == cls)[0]
        unit = 1.0 / (2 * (len(members) // 2) * C)
        np.add.at(w, members[ridx.numpy()], unit)
        np.add.at(w, members[lidx.numpy()], unit)
    return torch.from_numpy(w)


@pytest.mark.parametrize("case", ["A", "B"])
def test_chain_reproduces_the_oracle_in_float64(case):
    r = _inputs(case, "fp32")
    N = r["N"]
    leaves, outs = [], []
    for v in r["views"]:
        S, h, w = v["S"], v["h"], v["w"]
        cl, rv = v["cam_low"].clone().requires_grad_(True), v["rvd"].clone().requires_grad_(True)
        # the head rows' pre-activation: head = relu(pre), so d pre = d_head's first 128 columns (gated by head > 0)
        pre = torch.where(v["head"][:, :128] > 0, v["head"][:, :128], torch.full((), -1.0, dtype=torch.float64)).clone().requires_grad_(True)
        fp = F.relu(pre).view(N, h, w, 128).permute(0, 3, 1, 2)
        up = lambda t: F.interpolate(t, size=(S, S), mode="bilinear", align_corners=True)
        leaves.append((cl, rv, pre))
        outs.append((up(cl), up(rv), fp, rv))
    extras = {}
    torch.set_default_dtype(torch.float64)                    # (the oracle allocates its prototypes and label column in the default type)
    try:
        ref = oloss.step_loss(outs[0], outs[1], r["label20"], BG, random.Random(11), extras)
        ref["loss"].backward()
    finally:
        torch.set_default_dtype(torch.float32)
    for v, y, sel in zip(r["views"], (extras["pseudo1"], extras["pseudo2"]), (extras["sel1"], extras["sel2"])):
        v["w_inject"] = weights_from_selections(y, sel)
    LF.run_chain(r, torch.float64, "fp32")

    def close(tag, got, want):
        rel = float((got - want).abs().max() / want.abs().max())
        print(f"{tag}: {rel:.2e}")
        assert rel <= 1e-10, (tag, rel)

    names = ("loss", "loss_cls", "loss_er", "loss_ecr", "loss_nce", "loss_intra_nce", "loss_cross_nce", "loss_cross_nce2")
    for k, name in enumerate(names):
        close(name, r["out8"][k], ref[name].detach().double().reshape(()))
    for i, (v, (cl, rv, pre)) in enumerate(zip(r["views"], leaves)):
        assert torch.equal(v["y"], (extras["pseudo1"], extras["pseudo2"])[i])
        close(f"protos.v{i}", v["protos"], (extras["protos1"], extras["protos2"])[i].double())
        close(f"d_cam_low.v{i}", v["d_cam_low"], cl.grad)
        close(f"d_rvd.v{i}", v["d_rvd"], rv.grad)
        n = N * v["h"] * v["w"]
        rows = r["d_head"][v["off"]:v["off"] + n]
        close(f"d_head.v{i}[:, :128]", rows[:, :128], pre.grad)
        close(f"d_head.v{i}[:, 128:149]", rows[:, 128:149], cl.grad.permute(0, 2, 3, 1).reshape(-1, 21))
        assert bool((rows[:, 149:] == 0).all())


@pytest.mark.parametrize("case", ["A", "B"])
def test_weight_stages_follow_the_sampling_rule(case):
    """both rules of the weight stage on the records of the float32 chain, against the oracle's own selections on the same similarities: the
    RNG-parity rule with the oracle's random stream, the key rule with the same rank band (and a random half of the right size)"""
    r = LF.copy_record(_honest(case, "fp32"))
    LF.run_chain(r, torch.float32, "fp32", rng=random.Random(5), start="weights")
    rng = random.Random(5)
    for i, v in enumerate(r["views"]):
        sim = r[f"sim.v{i}"]
        # the oracle ranks by (f . pos + 1) / 2 of ITS similarities; hand it features whose similarity to the own prototype is the stored record
        rec = []
        y, P = v["y"], v["y"].shape[0]
        protos = torch.eye(21, 128, dtype=torch.float64)
        fo = torch.zeros(P, 128, dtype=torch.float64)
        fo[torch.arange(P), y] = sim
        oloss.intra_view_nce(fo, y, protos, rng, rec)
        want = weights_from_selections(y, rec)
        assert float((v["w_intra"] - want).abs().max()) <= 1e-6 * float(want.max()), i
        keyed = torch.from_numpy(LF.sampling_rule(y.numpy(), sim.numpy(), rkn=v["rkey"].numpy()))
        band = torch.from_numpy(LF.sampling_rule(y.numpy(), sim.numpy(), flags=np.zeros(P, dtype=np.uint8)))
        assert abs(float(keyed.sum()) - float(want.sum())) <= 1e-9 and bool((keyed >= band - 1e-15).all())
        assert torch.equal(_honest(case, "fp32")["views"][i]["w_intra"], keyed.float().double())


# ------------------------------------------------------------------------------------------------------------------ 2. the honest kernel
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ["A", "B"])
def test_honest_emulation_is_inside_every_bar(case, mode):
    r = _honest(case, mode)
    table = LF.judge(r, mode)
    _print(f"{case} {mode}", table)
    assert all(row[3] for row in table), [row for row in table if not row[3]]
    assert {LF.row_of(row[0]) for row in table} == set(LF.ROW_ORDER) - {"acc"}
    assert sum(1 for row in table if ":acc." in row[0]) == 7


# ------------------------------------------------------------------------------------------------------------------ 3. planted wiring defects
DEFECTS = {      # defect: (the row of the stage table it must fail at, the case it runs on)
    "minpool_coef_without_N": ("minpool", "A"),          # N dropped from the min-pool coefficient of select_finish
    "er_coef_without_20": ("prep", "A"),                 # the 20 dropped from er_coef
    "Gr_halves_swapped": ("d_rvd", "A"),                 # Gr[N:] handed to view 1 and Gr[:N] to view 2
    "dlt_directions_swapped": ("prep", "A"),             # each view's rvd map against its OWN view's one-hot CAM
    "st_rv_unmasked": ("stats", "A"),                    # the label mask dropped from the statistics of rvd
    "no_bias_in_d_cam_low": ("d_cam_low", "B"),          # the GAP bias of the classification loss not applied
    "own_other_protos_swapped": ("nce", "B"),            # own / other prototypes swapped in nce_fused
    "coef_intra_cross_exchanged": ("nce", "A"),          # coef_intra and coef_cross exchanged
    "d_head_view2_at_offset_0": ("d_head", "A"),         # view 2's d_head written at row 0
    "d_rvd_into_head_grad": ("d_head", "B"),             # d_rvd handed to head_grad_fused in place of d_cam_low
    "pseudo_from_unresized_rvd": ("R", "B"),             # pseudo-labels from the 20 x 20 rvd read as if it were 16 x 16
    "w_intra_of_view1_for_view2": ("nce", "B"),          # view 1's hard-pixel weights used for view 2
    "k_ecr_rounded": ("ecr", "A"),                       # K_ecr = round(21 npix 0.2) instead of int(...)
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defect_leaves_the_bar_of_its_stage(defect, mode):
    """The chain runs on from the defective stage, so every later stage is computed from what the defective stage stored: only the stage named
    may leave its bar."""
    row, case = DEFECTS[defect]
    r = LF.run_chain(LF.copy_record(_honest(case, mode)), torch.float32, mode, defects=(defect,), start=row)
    upto = LF.ROW_ORDER[:LF.ROW_ORDER.index(row) + 1]
    table = LF.judge(r, mode, only=upto)
    out = [(tag, ratio) for tag, _n, ratio, ok, _d, _l in table if not ok]
    print(f"[{case} {mode}] {defect}: outside at {out}")
    assert out and {LF.row_of(tag) for tag, _r in out} == {row}, (defect, mode, out)


# ------------------------------------------------------------------------------------------------------------------ 4. conditions
def check_conditions(cond, built_ties=False):
    assert max(cond["undecided"]) <= LF.NCE_MAX_EXCLUDED, cond
    assert max(cond["label_near"]) <= 0.02, cond       # (top-32 membership is judged exactly on the stored ncam: a near-tie there leaves nothing out)
    assert built_ties or (cond["ecr_ties"] == 0 and sum(cond["minpool_ties"]) == 0), cond


@pytest.mark.parametrize("case", ["A", "B"])
def test_conditions_hold_for_the_procedural_inputs(case):
    cond = LF.conditions(_honest(case, "fp32"))
    print(case, cond)
    check_conditions(cond)
