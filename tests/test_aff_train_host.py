"""aff_train on the host: the CPU restatement (tests/aff_train_ref.py) against the fixtures the reference produced
(scripts/make_aff_train_goldens.py), and the host-side rules of wseg_amd.aff_train / Net.affinities_train.  The tolerances of the
restatement are the ones tests/test_oracle_golden.py holds for its step fixtures (scalars 5e-6, gradient slices and norms 1e-4, weight
deltas 1e-3 of the largest)."""
import os

import numpy as np
import pytest
import torch

from tests import aff_train_ref as A
from wseg_amd import synth


@pytest.fixture(scope="module")
def aff_sd():
    return synth.procedural_aff_state_dict(0)


@pytest.mark.parametrize("name", A.FIXTURES)
def test_restatement_reproduces_the_reference_steps(golden_dir, aff_sd, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    steps, opt = A.run_steps(g, aff_sd)
    assert len(steps) == 2
    np.testing.assert_allclose([gr["lr"] for gr in opt.groups], g["lr_final"], rtol=1e-12)
    for s_, (out7, grads, weights) in enumerate(steps):
        for i, k in enumerate(A.STATS):
            ref = float(g[f"s{s_}/{k}"])
            assert abs(float(out7[i]) - ref) <= 5e-6 * max(1.0, abs(ref)), (s_, k, float(out7[i]), ref)
        for k in A.GRAD_KEYS:
            ref = g[f"gslice{s_}/{k}"]
            got = A.slice_of(grads[k]).numpy()
            assert np.abs(got - ref).max() / (np.abs(ref).max() + 1e-12) < 1e-4, (s_, k)
            gn = float(g[f"gnorm{s_}/{k}"])
            assert gn > 0 and abs(grads[k].double().norm().item() - gn) < 1e-4 * gn, (s_, k)
            w0 = A.slice_of(aff_sd[k]).double().numpy()
            d_ref, d_got = g[f"wslice{s_}/{k}"].astype(np.float64) - w0, A.slice_of(weights[k]).double().numpy() - w0
            assert np.abs(d_ref).max() > 0 and np.abs(d_got - d_ref).max() <= 1e-3 * np.abs(d_ref).max(), (s_, k)


def test_fixture_geometry(golden_dir):
    """the two cases the fixtures were asked for: an 8 x 8 map at radius 3 (below the 2 * 5 + 1 edge rule), N = 2; a 13 x 13 map at radius 5"""
    a, b = (np.load(os.path.join(golden_dir, n + ".npz")) for n in A.FIXTURES)
    assert (int(a["n"]), int(a["h"]), int(a["w"]), int(a["radius"])) == (2, 8, 8, 3)
    assert (int(b["n"]), int(b["h"]), int(b["w"]), int(b["radius"])) == (1, 13, 13, 5)


def test_cli_flags_equal_the_references(golden_dir):
    """names, defaults and required-ness as recorded from the reference's argparse set; --network points at this package's module,
    --precision is the one additive flag"""
    from wseg_amd import aff_train
    g = np.load(os.path.join(golden_dir, A.FIXTURES[0] + ".npz"))
    ref = {str(f): (str(d), bool(r)) for f, d, r in zip(g["cli_flags"], g["cli_defaults"], g["cli_required"])}
    assert len(ref) == 14
    ours = {a.option_strings[0]: ("" if a.default is None else repr(a.default), a.required)
            for a in aff_train.make_parser()._actions if a.option_strings[0] not in ("-h",)}
    assert set(ours) - set(ref) == {"--precision"}
    for flag, (default, required) in ref.items():
        if flag == "--network":
            assert default == repr("network.resnet38_aff") and ours[flag] == (repr("wseg_amd.resnet38_aff"), False)
        else:
            assert ours[flag] == (default, required), flag


def test_max_step_rule():
    from wseg_amd import aff_train
    assert aff_train.max_step_of(10582, 8, 8) == 10582 // 8 * 8 == 10576
    assert aff_train.max_step_of(6, 2, 1) == 3 and aff_train.max_step_of(7, 4, 3) == 3


def test_optimizer_groups_tile_the_flat_buffer():
    """lr, 2 lr, 10 lr, 20 lr with weight decay on groups 0 and 2; once every trainable weight holds its slice of the flat buffers, the
    non-empty groups' segments tile it exactly (PolyOptimizer._flat_plan: the fused SGD launch)"""
    from wseg_amd import aff_train
    from wseg_amd.resnet38_aff import Net
    model = Net(precision="fp32")
    opt = aff_train.build_optimizer(model, 0.01, 5e-4, 100)
    assert [g["lr"] for g in opt.param_groups] == [0.01, 0.02, 0.1, 0.2]
    assert [g["weight_decay"] for g in opt.param_groups] == [5e-4, 0, 5e-4, 0]
    assert len(opt.param_groups[2]["params"]) == 4 and not opt.param_groups[1]["params"] and not opt.param_groups[3]["params"]
    model.train()
    eng = model._engine.ensure_flat(torch.device("cpu"))
    assert opt._flat_plan() is None                                     # no gradients yet
    eng.attach_grads()
    plan = opt._flat_plan()
    assert plan is not None and plan[0] is eng
    segs = plan[1]
    head0 = eng.offsets["f8_3.weight" if "f8_3.weight" in eng.offsets else "f8_3"][0]
    assert [(s[0], s[1]) for s in segs] == [(0, head0), (head0, eng.flat_w.numel())]
    assert [s[2] for s in segs] == [0.01, 0.1] and [s[3] for s in segs] == [5e-4, 5e-4]


def test_affinities_train_refuses_eval_mode_and_cpu_tensors():
    from wseg_amd.resnet38_aff import Net
    model = Net(precision="fp32")
    x = torch.zeros(1, 3, 64, 64)
    model.eval()
    with pytest.raises(RuntimeError, match="training mode"):
        model.affinities_train(x)
    model.train()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.affinities_train(x)
    with pytest.raises(RuntimeError, match="inference-only"):           # forward keeps refusing training mode
        model(x)
