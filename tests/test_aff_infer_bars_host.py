"""The derived bars of the AffinityNet inference tests (tests/aff_infer_f64.py) judged on the CPU, over every case
tests/test_gpu_aff_infer_kernels.py runs on the GPU: the honest float32 emulation of each kernel lies inside the bar on EVERY element, and
every planted defect a case claims to judge puts some element outside it, so a bar loosened later fails here before it reaches a kernel.
Also: the identity the stencil walk rests on (dense power = stencil walk, both in float64), the cap on the unjudged pixels of the arg-max
cases for the reference alone, and the argument refusals of the six C entry points (they run before any device call: the library loads
without a GPU, and a refused call returns -1 with its message where a launch on this host could only return -2)."""
import ctypes as C

import numpy as np
import pytest

from tests import aff_infer_f64 as X
from wseg_amd import _lib as L

_id = lambda c: c.name


def _outside(got, ref, bar):
    with np.errstate(invalid="ignore"):
        return ~(np.abs(got.astype(np.float64) - ref) <= bar)             # (inf and NaN are outside)


def _honest(tag, got, ref, bar):
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1), np.where(err > 0, np.inf, 0))))
    print(f"{tag}: honest max err {float(err.max()):.3e}, max err/bar {ratio:.3f}")
    assert np.isfinite(bar).all() and not _outside(got, ref, bar).any(), tag


def _judged(tag, defect, bad):
    print(f"{tag} {defect}: outside the bar {float(bad.mean()):.4f}")
    assert bad.any(), (tag, defect)


@pytest.mark.parametrize("c", X.PAIR_CASES, ids=_id)
def test_pairs_bars(c):
    p = X.pair_problem(c)
    got = X.emulate_pairs(p)
    _honest(c.name, got, p.ref, p.bar)
    same = p.m == 0
    assert bool(same.any()) == c.dup and (got[same] == 1.0).all()
    for d in sorted(c.judges):
        _judged(c.name, d, _outside(X.emulate_pairs(p, d), p.ref, p.bar))


@pytest.mark.parametrize("name,h,w,r", [("aff_40x56", 5, 7, 2), ("aff_64x88", 8, 11, 3)])
def test_dense_scatter_is_the_reference_matrix(golden_dir, name, h, w, r):
    """dense_ref (what the GPU file holds aff_to_dense to, bit for bit) against the reference's own dense matrix"""
    import os
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    np.testing.assert_array_equal(X.dense_ref(g["aff"], X.geo(r, h, w)), g["aff_mat"])


@pytest.mark.parametrize("c", X.PREPARE_CASES, ids=_id)
def test_prepare_bars(c):
    g = X.geo(c.r, c.h, c.w)
    aff = X.rand_aff(7, c.N, g)
    assert (aff == 0).any() and (aff == 1).any() or g.n_from * g.P * c.N < 60
    pr = X.prepare_ref(aff, g, c.beta)
    wgt, rsum = X.emulate_prepare(aff, g, c.beta)
    _honest(c.name + " wgt", wgt, pr.wgt, pr.bar_w)
    _honest(c.name + " rsum", rsum, pr.rsum, pr.bar_r)
    assert (wgt[pr.exact] == pr.wgt[pr.exact]).all()
    assert pr.exact.all() == (c.beta == 0) or not pr.edge.any()
    for d in sorted(c.judges):
        bw, br = X.emulate_prepare(aff, g, c.beta, d)
        _judged(c.name, d, np.concatenate([_outside(bw, pr.wgt, pr.bar_w).ravel(), _outside(br, pr.rsum, pr.bar_r).ravel()]))


@pytest.mark.parametrize("c", X.WALK_CASES, ids=_id)
def test_walk_bars(c):
    p = X.walk_problem(c)
    assert c.model == ("worst" if (1 << c.logt) * (2 * p.g.P + 1) * X.U32 <= X.WALK_WORST_MAX else "chain")
    _honest(f"{c.name} ({c.model})", X.emulate_walk(p.wgt, p.rsum, p.v, p.g, c.logt), p.ref, p.bar)
    if c.N > 1:
        assert not np.array_equal(p.wgt[0], p.wgt[1])
    for d in sorted(c.judges):
        _judged(c.name, d, _outside(X.emulate_walk(p.wgt, p.rsum, p.v, p.g, c.logt, d), p.ref, p.bar))


@pytest.mark.parametrize("c", X.POOL_CASES, ids=_id)
def test_pool_bars(c):
    p = X.pool_problem(c)
    _honest(c.name, X.emulate_pool(p.cams, c.src, c.bg, c.H, c.W), p.ref, p.bar)
    for d in sorted(c.judges):
        _judged(c.name, d, _outside(X.emulate_pool(p.cams, c.src, c.bg, c.H, c.W, d), p.ref, p.bar))


@pytest.mark.parametrize("c", X.FINISH_CASES, ids=_id)
def test_finish_bars(c):
    p = X.finish_problem(c)
    r = p.ref
    got = X.emulate_finish(p.cam, c.H, c.W)
    print(f"{c.name}: unjudged share of the reference {r.unjudged:.5f}, emulation differs on {int((got != r.arg).sum())} pixels")
    if c.kind == "equal":
        assert (got == 0).all()
        return
    assert r.unjudged <= X.FINISH_UNJUDGED_MAX
    assert (got[r.judged] == r.arg[r.judged]).all()
    if c.kind == "dup":
        assert r.judged.all() and (r.arg == c.dup[0]).all()
    for d in sorted(c.judges):
        bad = X.emulate_finish(p.cam, c.H, c.W, d)
        _judged(c.name, d, (bad != r.arg) & r.judged)


@pytest.mark.parametrize("c", X.COMPOSED_CASES, ids=_id)
def test_composed_bars(c):
    p = X.composed_problem(c)
    cam, pred = X.emulate_composed(p)
    _honest(c.name + " cam_rw", cam, p.cam, p.bar_cam)
    print(f"{c.name}: unjudged share of the reference {p.fin.unjudged:.5f}")
    assert p.fin.unjudged <= X.FINISH_UNJUDGED_MAX
    assert (pred[p.fin.judged] == p.fin.arg[p.fin.judged]).all()


def test_every_kernel_has_a_judge_for_every_listed_defect():
    listed = {"pairs": ({"mean_ld", "drop_group"}, X.PAIR_CASES), "prepare": ({"no_diag", "beta_plus1", "to_plus", "batch0"}, X.PREPARE_CASES),
              "walk": ({"logt_steps", "slot_minus", "batch0"}, X.WALK_CASES), "pool": ({"count_div"}, X.POOL_CASES),
              "finish": ({"align_true", "last_max"}, X.FINISH_CASES)}
    for kernel, (defects, cases) in listed.items():
        for d in defects:
            assert any(d in c.judges for c in cases), (kernel, d)
    for cases in (X.PREPARE_CASES, X.WALK_CASES):
        assert any("batch0" in c.judges and c.N >= 2 for c in cases)
    # what the GPU file must exercise: radius 2..6, N > 1, ld > C, bf16, C < 64 and C = 512, a partial last workgroup, area 8192, planes
    for cases in (X.PAIR_CASES, X.PREPARE_CASES, X.WALK_CASES):
        assert {c.r for c in cases} == {2, 3, 4, 5, 6} and {c.N for c in cases} == {1, 3}
    assert {c.C for c in X.PAIR_CASES} == {8, 24, 448, 512} and {c.dt for c in X.PAIR_CASES} == {"f32", "bf16"}
    assert any(c.ld > c.C and c.dt == dt for c in X.PAIR_CASES for dt in ("f32", "bf16"))
    assert any((c.N * X.geo(c.r, c.h, c.w).n_from) % 4 for c in X.PAIR_CASES)
    assert {c.beta for c in X.PREPARE_CASES} == {0, 1, 8}
    assert {c.h * c.w for c in X.WALK_CASES} == {35, 88, 130, 2961, L.RW_MAX_PLANE}
    assert {c.planes for c in X.WALK_CASES} == {1, 5, 21} and {c.logt for c in X.WALK_CASES} == {0, 1, 3, 6}
    assert {c.model for c in X.WALK_CASES} == {"worst", "chain"}
    assert {c.planes for c in X.FINISH_CASES} >= {1, 2, 21, 32} and any(c.dh == 1 for c in X.FINISH_CASES)


@pytest.mark.parametrize("r", [2, 3, 4, 5, 6])
def test_stencil_walk_is_the_dense_power_in_float64(r):
    """the identity the walk kernel rests on: A^beta, column normalisation, logt squarings, v . T  ==  2^logt stencil applications"""
    h, w = X.MAPS[r]
    g = X.geo(r, h, w)
    assert g.P == L.aff_num_offsets(r)
    rng = np.random.default_rng(r)
    aff = (0.2 + 0.8 * rng.random((g.P, g.n_from))).astype(np.float32)
    v = rng.random((3, g.area)).astype(np.float32) * 2 - 0.5
    for beta in (1, 8):
        for logt in (0, 3):
            a, b = X.dense_walk64(aff, g, beta, logt, v), X.stencil_walk64(aff, g, beta, logt, v)
            dev = float((np.abs(a - b).max(axis=1) / np.abs(a).max(axis=1)).max())
            print(f"r={r} {h}x{w} beta={beta} logt={logt}: dense vs stencil {dev:.2e}")
            assert dev <= 1e-12


# ------------------------------------------------------------------------------------------------------------------ refusals
PTR = C.c_void_p(L._ANY)               # a stand-in address nobody dereferences: every call below is refused before any device call
NULL = C.c_void_p(None)
SRC = (C.c_int * 21)(*([-1] * 21))
SRC_CLASS = (C.c_int * 21)(*([-1] * 20 + [0]))


def _pairs(ld=448, Cc=448, N=1, h=13, w=16, r=5, dtype=L.F32):
    return L.lib.wseg_aff_pairs(PTR, ld, Cc, PTR, N, h, w, r, dtype, None)


def _dense(h=13, w=16, r=5):
    return L.lib.wseg_aff_to_dense(PTR, PTR, h, w, r, None)


def _prepare(N=1, h=13, w=16, r=5, beta=8):
    return L.lib.wseg_rw_prepare(PTR, PTR, PTR, N, h, w, r, beta, None)


def _walk(N=1, planes=21, h=13, w=16, r=5, logt=6):
    return L.lib.wseg_random_walk(PTR, PTR, PTR, PTR, N, planes, h, w, r, logt, None)


def _pool(cams=PTR, src=SRC, H=93, W=130, dh=12, dw=17):
    return L.lib.wseg_rw_pool(cams, src, C.c_float(0.27), PTR, H, W, dh, dw, None)


def _finish(planes=21, dh=12, dw=17, H=93, W=130):
    return L.lib.wseg_rw_finish(PTR, PTR, planes, dh, dw, H, W, None)


GEOMETRY = [(dict(r=1), "radius 1 outside [2, 6]"), (dict(r=7), "radius 7 outside [2, 6]"),
            (dict(h=4, w=16), "a 4x16 map has no 'from' pixel at radius 5"), (dict(h=13, w=8), "a 13x8 map has no 'from' pixel at radius 5")]
REFUSALS = [(call, kw, text) for call in (_pairs, _dense, _prepare, _walk) for kw, text in GEOMETRY] + [
    (_pairs, dict(Cc=12, ld=16), "aff_pairs: C=12 ld=16"),
    (_pairs, dict(Cc=520, ld=520), "aff_pairs: C=520 ld=520"),
    (_pairs, dict(ld=440), "aff_pairs: C=448 ld=440"),
    (_pairs, dict(ld=452), "aff_pairs: C=448 ld=452"),
    (_pairs, dict(dtype=3), "aff_pairs: bad dtype 3"),
    (_pairs, dict(dtype=-1), "aff_pairs: bad dtype -1"),
    (_pairs, dict(N=0), "aff_pairs: null pointer / empty batch"),
    (_prepare, dict(beta=-1), "rw_prepare: beta=-1"),
    (_walk, dict(logt=-1), "random_walk: logt=-1 outside [0, 20]"),
    (_walk, dict(logt=21), "random_walk: logt=21 outside [0, 20]"),
    (_walk, dict(h=3, w=2731, r=2), "random_walk: a 3x2731 map (8193 pixels) exceeds the LDS plane limit of 8192 pixels"),
    (_walk, dict(planes=0), "random_walk: null pointer / empty batch"),
    (_dense, dict(h=256, w=257), "aff_to_dense: a 65792x65792 dense matrix is too large"),
    (_pool, dict(dh=11), "rw_pool: 11x17 is not the pooled size of 93x130"),
    (_pool, dict(dh=13), "rw_pool: 13x17 is not the pooled size of 93x130"),
    (_pool, dict(dw=16), "rw_pool: 12x16 is not the pooled size of 93x130"),
    (_pool, dict(cams=NULL, src=SRC_CLASS), "rw_pool: class planes without a CAM buffer"),
    (_finish, dict(planes=0), "rw_finish: bad arguments"),
    (_finish, dict(planes=33), "rw_finish: bad arguments"),
    (_finish, dict(dh=11), "rw_finish: 11x17 upsampled x8 does not cover 93x130"),
]


@pytest.mark.parametrize("call,kw,text", REFUSALS, ids=[f"{f.__name__[1:]}-{'-'.join(f'{k}={v}' for k, v in kw.items() if k not in ('cams', 'src'))}"
                                                        f"{'-nullcams' if 'cams' in kw else ''}" for f, kw, _t in REFUSALS])
def test_entry_points_refuse_bad_arguments(call, kw, text):
    assert call(**kw) == -1                                    # -1: refused by a check; a launch (or a memset) would have returned -2 or 0
    assert text in L.lib.wseg_last_error().decode(), L.lib.wseg_last_error().decode()


def test_limits_of_the_walk_are_the_documented_ones():
    assert L.RW_MAX_PLANE == 8192 and [L.aff_num_offsets(r) for r in range(1, 8)] == [-1, 4, 12, 22, 34, 54, -1]
    assert max(L.aff_num_offsets(r) for r in range(2, 7)) <= 64                        # WSEG_AFF_MAX_OFFSETS
