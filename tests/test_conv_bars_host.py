"""The derived bars of the convolution tests (tests/conv_f64.py) judged on the CPU, over every case tests/test_gpu_conv_f64.py runs on the GPU:
the honest emulation (float32 accumulation + the kernel's store) lies inside the bar on EVERY element of every output, and each planted
defect — truncating bf16 store, result x (1 + 2^-8), one product dropped per output, the lo.hi term of split-bf16 dropped, one pixel dropped
from the weight gradient — puts some element outside it on every case whose `judges` claims it.  A bar loosened later (a safety factor on
the storage rounding, a wider accumulation term) fails here before it reaches a kernel."""
import pytest
import torch

from tests import conv_f64 as X

CASES = X.CONV_CASES + X.epi_cases() + X.STEM_CASES
_out = lambda got, ref, bar: (got - ref).abs() > bar


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_conv_bars(c):
    p = X.conv_problem(c)
    honest = X.emulate_conv(p)
    assert set(honest) == set(p.refs)
    for name, (ref, bar) in p.refs.items():
        r = ((honest[name] - ref).abs() / bar).max()
        print(f"{c.name} {name}: honest max err/bar {float(r):.3f}")
        assert bool(torch.isfinite(bar).all()) and float(r) <= 1.0
    for defect in sorted(c.judges):
        bad = X.emulate_conv(p, defect)
        frac = {name: float(_out(bad[name], ref, bar).double().mean()) for name, (ref, bar) in p.refs.items()}
        print(f"{c.name} {defect}: outside the bar {frac}")
        assert all(f > 0 for f in frac.values()), (defect, frac)


def test_every_family_and_store_has_a_rounding_judge():
    """a truncating bf16 store is judged (and seen, test_conv_bars) by at least one case with K <= 576 on every kernel family, forward and data
    gradient, and by the stem.  f32 storage has no storage rounding to get wrong: the accumulator is stored as it is (tests/conv_f64.py)."""
    judged = set()
    for c in CASES:
        if "trunc" in c.judges and c.K <= 576:
            judged |= {(c.kind, bm) for bm in c.fams}
    for bm in (64, 128, 224, 256, 259):
        assert ("fwd", bm) in judged, bm
    for bm in (128, 224, 256, 259):
        assert ("dgrad", bm) in judged, bm
    assert any(c.opset == "stem" and "trunc" in c.judges for c in CASES)


@pytest.mark.parametrize("c", list(X.WGRAD_CASES.values()), ids=lambda c: c.name)
def test_wgrad_bars(c):
    p = X.wgrad_problem(c)
    first = X.emulate_wgrad(p)
    for splits, prior in ((1, None), (3, first)):
        ref, bar = X.wgrad_bar(p, splits, prior)
        r = ((X.emulate_wgrad(p, prior=prior) - ref).abs() / bar).max()
        print(f"{c.name} splits {splits}: honest max err/bar {float(r):.4f}")
        assert float(r) <= 1.0
        for defect in sorted(c.judges):
            frac = float(_out(X.emulate_wgrad(p, defect, prior), ref, bar).double().mean())
            print(f"{c.name} splits {splits} {defect}: outside the bar {frac:.3f}")
            assert frac > 0, defect


def test_cases_plan_onto_the_family_they_name():
    """every forward / data-gradient run of tests/test_gpu_conv_f64.py asks the planner (pure host arithmetic) for the kernel family and the
    row order its case names, and every weight-gradient run for its kernel: a case cannot drift onto another kernel unnoticed"""
    from wseg_amd import _lib as L
    from tests import test_gpu_conv_f64 as G
    for c, bm in G.CONV_RUNS:
        p = G._problem(c)
        plan = L.conv_plan(**G._launch_kw(p, bm, "cpu"))
        fam = G._family(c, bm)
        assert plan.family in (fam if isinstance(fam, tuple) else (fam,)), (c.name, bm, plan)
        assert bm not in c.perm or plan.perm == c.perm[bm], (c.name, bm, plan)
    for c, hint in G.WGRAD_RUNS:
        p = G._problem(c)
        pipe = hint == 256 and c.dt == "bf16" and c.IC >= 256 and c.OC >= 256
        plan = L.wgrad_plan(tile_hint=hint, dtype={"f32": L.F32, "bf16": L.BF16, "x3": L.F32X3}[c.dt], **G._wgrad_kw(p))
        assert plan.family == (G.WGRAD_PIPE if pipe else G.WGRAD_128), (c.name, hint, plan)
