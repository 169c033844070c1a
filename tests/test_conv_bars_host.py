"""The derived bars of the convolution tests (tests/conv_f64.py) judged on the CPU, over every case tests/test_gpu_conv_f64.py runs on the GPU:
the honest emulation (float32 accumulation + the kernel's store) lies inside the bar on EVERY element of every output, and each planted
defect — truncating bf16 store, result x (1 + 2^-8), one product dropped per output, the lo.hi term of split-bf16 dropped, one pixel dropped
from the weight gradient, and the weight gradient's address defects (seam, image wrap, border, last K-tile, column rotation) — puts some
element outside it on every case whose `judges` claims it.  The plan queries (host arithmetic) show that every run lands on the kernel,
the staging variant and the split count its case names, and a table check that no staging path is left without a judge of a feature.  A bar loosened later (a safety factor on
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
    # the explicit gather the address defects are planted in IS the weight gradient when nothing is planted
    gather = sum(X._wgrad_gather(c, i, x.double(), dy.double()) for i, (x, dy) in enumerate(zip(p.xs, p.dys)))
    plain = X._wgrad(c, p.xs, p.dys, torch.float64)
    assert float((torch.roll(gather[:c.OC_dw, :, :c.IC_dw], c.dw_rot, dims=2) - plain).abs().max()) <= 1e-12 * float(p.A.max())
    first = X.emulate_wgrad(p)
    for splits, prior in ((c.nsplit or 1, None), (3, first)):
        ref, bar = X.wgrad_bar(p, splits, prior)
        r = ((X.emulate_wgrad(p, prior=prior) - ref).abs() / bar).max()
        print(f"{c.name} splits {splits}: honest max err/bar {float(r):.4f}")
        assert bool(torch.isfinite(bar).all()) and float(r) <= 1.0
        for defect in sorted(c.judges):
            frac = float(_out(X.emulate_wgrad(p, defect, prior), ref, bar).double().mean())
            print(f"{c.name} splits {splits} {defect}: outside the bar {frac:.3f}")
            assert frac > 0, defect


def _wgrad_plans():
    """(case, hint, plan of the first launch) of every weight-gradient run of tests/test_gpu_conv_f64.py, the pair grids included"""
    from wseg_amd import _lib as L
    from tests import test_gpu_conv_f64 as G
    out = []
    for c, hint in G.WGRAD_RUNS:
        out.append((c, hint, L.wgrad_plan(split_k=c.split_k, **G._wgrad_launch_kw(c, hint))))
    for name in X.PAIR_CASES:
        c, cd = X.WGRAD_CASES[name], next(k for k in X.CONV_CASES if k.name == name + "_dgrad")
        fused, dg, wg = L.conv_pair_plan(G._wgrad_kw(c), **G._launch_kw(G._problem(cd), 0, "cpu"))
        assert fused == 1 and dg.family in G.TILE_256, (name, fused, dg, wg)
        out.append((c, 256, wg))
    return out


def test_cases_plan_onto_the_family_they_name():
    """every forward / data-gradient run of tests/test_gpu_conv_f64.py asks the planner (pure host arithmetic) for the kernel family and the
    row order its case names, and every weight-gradient run for its kernel, its staging variant (unit) and its split count (nwg where the
    case states it): a case cannot drift onto another kernel, another stager or another block map unnoticed"""
    from wseg_amd import _lib as L
    from tests import test_gpu_conv_f64 as G
    for c, bm in G.CONV_RUNS:
        p = G._problem(c)
        plan = L.conv_plan(**G._launch_kw(p, bm, "cpu"))
        fam = G._family(c, bm)
        assert plan.family in (fam if isinstance(fam, tuple) else (fam,)), (c.name, bm, plan)
        assert bm not in c.perm or plan.perm == c.perm[bm], (c.name, bm, plan)
    for c, hint, plan in _wgrad_plans():
        pipe = X.wgrad_pipe(c, hint)
        assert plan.family == (G.WGRAD_PIPE if pipe else G.WGRAD_128), (c.name, hint, plan)
        assert plan.unit == (c.unit if pipe else 0), (c.name, hint, plan)
        assert c.nsplit is None or plan.nsplit == c.nsplit, (c.name, hint, plan)
        assert c.nwg is None or plan.nwg == c.nwg, (c.name, hint, plan)
        if c.split_k == 8:                           # the nsplit % 8 == 0 block map, with a short last split
            assert plan.nsplit == 8 and c.n_pix - 7 * 64 == 32, (c.name, plan)
        if c.tiny_seg is not None:                   # the header's own rule (wgrad_plan: simple_adv) for the segment named
            OH, OW = c.osizes[c.tiny_seg]
            assert X.WGRAD_PK[c.dt] // OW + 1 > OH and 64 // OW + 1 > OH, (c.name, OH, OW)
        elif pipe and c.unit == 0:                   # StageGeneral by geometry, not by a tiny map: the branch-free advance
            assert all(64 // ow + 1 <= oh for oh, ow in c.osizes) and (c.s != 1 or c.sizes != c.osizes), c.name
    # what the seam cases state about their seam
    c = X.WGRAD_CASES["wgp_seg2_unit"]
    M1, M = c.N * c.osizes[0][0] * c.osizes[0][1], c.n_pix
    assert (M1, M) == (240, 384) and -(-M1 // 64) == 4 and -(-(M - M1) // 64) == 3 and c.seg2[1] != c.W and c.d * (c.k // 2) > 0
    assert L.wgrad_plan(split_k=3, **G._wgrad_launch_kw(c, 256)).nsplit == 3           # [0,128) [128,256) [256,384): the second crosses at 240
    for name, seam in (("wg_seg2_bf16", 240), ("wg_seg2_f32", 240), ("wg_seg2_s2", 220), ("wgp_seg2_s2", 220), ("wgp_seg2_tiny", 240)):
        c = X.WGRAD_CASES[name]
        assert c.N * c.osizes[0][0] * c.osizes[0][1] == seam and seam % X.WGRAD_PK[c.dt], name
    c = X.WGRAD_CASES["pair_seg2"]
    assert c.N * c.osizes[0][0] * c.osizes[0][1] == 29750 and 29750 % 64 != 0


def test_every_wgrad_path_has_a_judge_of_every_feature():
    """for each of the three staging paths of conv_wgrad_kernels.h (128-tile kernel, pipe kernel with StageUnit, with StageGeneral) some
    run of tests/test_gpu_conv_f64.py has each feature the path supports; the 128-tile kernel's dw_rot and strided views in bf16 and f32.
    StageUnit is stride 1 on maps that are not tiny by definition, and the pipe kernel has no dw_rot."""
    have = {"128": {}, "unit": {}, "general": {}}
    for c, hint, _plan in _wgrad_plans():
        path = ("unit" if c.unit else "general") if X.wgrad_pipe(c, hint) else "128"
        for f in X.wgrad_features(c, hint):
            have[path].setdefault(f, set()).add(c.dt)
    common = {"1x1", "dilated", "seam", "split8", "ctail", "extents"}
    want = {"128": common | {"stride2", "tiny", "rot", "views"}, "unit": common | {"views"}, "general": common | {"stride2", "tiny"}}
    for path, feats in want.items():
        assert feats <= set(have[path]), (path, feats - set(have[path]))
    for f in ("rot", "views", "stride2", "tiny", "seam"):
        assert {"bf16", "f32"} <= have["128"][f], (f, have["128"][f])
    # every address defect is claimed (and, test_wgrad_bars, seen) on every path that has the feature it breaks
    claimed = {"128": set(), "unit": set(), "general": set()}
    for c, hint, _plan in _wgrad_plans():
        claimed[("unit" if c.unit else "general") if X.wgrad_pipe(c, hint) else "128"] |= c.judges
    for path in claimed:
        assert {"seam_pixel", "wrap_pixel", "pad_wrap", "drop_tail", "drop_pixel", "scale"} <= claimed[path], (path, claimed[path])
    assert "rot_off" in claimed["128"]
