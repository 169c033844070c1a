"""The AffinityNet inference kernels (csrc/affinity.hip) one at a time through the C ABI (wseg_amd._lib) against the float64 references of
tests/aff_infer_f64.py, every element of every output inside the bar DERIVED there (tests/test_aff_infer_bars_host.py shows on the CPU what
those bars catch); no network and no goldens.  Outputs start as NaN with a sentinel guard behind them.  Each test prints max error and
max error / bar per case (table of an MI355X run: profiles/README.md).  The cases name what they exercise: radius 2..6 (r2..r6), batches
(N3), a row stride (ld > C), bf16, the 8192-pixel plane limit (64x128), in-place walking (in_place)."""
import numpy as np
import pytest
import torch

from tests import aff_infer_f64 as X

pytestmark = pytest.mark.gpu

GUARD, NG = -12345.0, 256
_id = lambda c: c.name
_problems = {}


def _problem(make, c):
    """inputs, references and bars of a case: computed once on the CPU, never written to"""
    key = (make.__name__, c.name)
    if key not in _problems:
        _problems[key] = make(c)
    return _problems[key]


def _out(n, dtype=torch.float32):
    """n elements of NaN with NG sentinels behind them"""
    buf = torch.full((n + NG,), float("nan"), device="cuda", dtype=dtype)
    buf[n:] = GUARD
    return buf


def _guard_ok(buf, n):
    return bool((buf[n:] == GUARD).all())


def _np(t):
    return t.detach().cpu().numpy()


def _check(tag, got, ref, bar):
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))
    print(f"{tag}: max err {float(np.nanmax(err)):.3e}, max err/bar {float(np.nanmax(ratio)):.3f}")
    assert bool((err <= bar).all()), tag               # (a NaN left in the output fails here)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------------------ pairs
@pytest.mark.parametrize("c", X.PAIR_CASES, ids=_id)
def test_aff_pairs(c):
    """every radius on the one-from-pixel maps and on a map per radius, C 8 / 24 / 448 / 512, rows wider than C with NaN in the padding, f32
    and bf16, batches, item counts that leave the last workgroup partial; identical rows give exactly 1; the guard stays; two runs and the
    dtype code of split-bf16 (f32 data) are bit-identical"""
    from wseg_amd import _lib as L
    p = _problem(X.pair_problem, c)
    g = p.g
    feat = _cuda(p.rows)
    if c.dt == "bf16":
        feat = feat.to(torch.bfloat16)                 # exact: the rows hold bf16 values (and NaN padding)
    n = c.N * g.P * g.n_from
    buf = _out(n)
    L.aff_pairs(feat, c.ld, c.C, buf, c.N, c.h, c.w, c.r)
    got = _np(buf[:n]).reshape(c.N, g.P, g.n_from)
    _check(f"pairs {c.name}", got, p.ref, p.bar)
    assert _guard_ok(buf, n)
    same = p.m == 0
    assert bool(same.any()) == c.dup and bool((got[same] == 1.0).all())
    again = _out(n)
    L.aff_pairs(feat, c.ld, c.C, again, c.N, c.h, c.w, c.r)
    assert torch.equal(again[:n], buf[:n])
    if c.dt == "f32":
        x3 = _out(n)
        L.check(L.lib.wseg_aff_pairs(L._v(feat), c.ld, c.C, L._v(x3), c.N, c.h, c.w, c.r, L.F32X3, L._s()), "wseg_aff_pairs")
        assert torch.equal(x3[:n], buf[:n]) and _guard_ok(x3, n)


# ------------------------------------------------------------------------------------------------------------------ dense
@pytest.mark.parametrize("r,hw", [(r, m[r]) for m in (X.MINIMAL, X.MAPS) for r in range(2, 7)] + [(5, (47, 63))],
                         ids=lambda v: f"r{v}" if isinstance(v, int) else f"{v[0]}x{v[1]}")
def test_aff_to_dense(r, hw):
    """a scatter: bit equality with both orientations plus the unit diagonal, whatever the matrix held before"""
    from wseg_amd import _lib as L
    g = X.geo(r, *hw)
    aff = X.rand_aff(3, 1, g)[0]
    n = g.area * g.area
    buf = _out(n)
    buf[:n] = -3.0
    L.aff_to_dense(_cuda(aff), buf, g.h, g.w, r)
    ok = np.array_equal(_np(buf[:n]).reshape(g.area, g.area), X.dense_ref(aff, g))
    print(f"dense r{r}_{g.h}x{g.w}: bit-equal {ok}")
    assert ok and _guard_ok(buf, n)


# ------------------------------------------------------------------------------------------------------------------ prepare
@pytest.mark.parametrize("c", X.PREPARE_CASES, ids=_id)
def test_rw_prepare(c):
    """wgt and rsum per image (the images differ), beta 0 / 1 / 8, affinities with exact zeros and ones: the exact values bit for bit"""
    from wseg_amd import _lib as L
    g = X.geo(c.r, c.h, c.w)
    aff = X.rand_aff(7, c.N, g)
    pr = X.prepare_ref(aff, g, c.beta)
    nw, nr = c.N * 2 * g.P * g.area, c.N * g.area
    wgt, rsum = _out(nw), _out(nr)
    L.rw_prepare(_cuda(aff), wgt, rsum, c.N, c.h, c.w, c.r, c.beta)
    gw, gr = _np(wgt[:nw]).reshape(pr.wgt.shape), _np(rsum[:nr]).reshape(pr.rsum.shape)
    _check(f"prepare {c.name} wgt", gw, pr.wgt, pr.bar_w)
    _check(f"prepare {c.name} rsum", gr, pr.rsum, pr.bar_r)
    assert bool((gw[pr.exact] == pr.wgt[pr.exact]).all())
    assert _guard_ok(wgt, nw) and _guard_ok(rsum, nr)


# ------------------------------------------------------------------------------------------------------------------ walk
@pytest.mark.parametrize("c", X.WALK_CASES, ids=_id)
def test_random_walk(c):
    """2^logt stencil steps against float64 on the same f32 weights; batches walk on their own image's weights; at logt 6 also in place
    (v_in aliasing v_out), bit for bit the out-of-place result; a plane of constants stays constant within the bar"""
    from wseg_amd import _lib as L
    p = _problem(X.walk_problem, c)
    g = p.g
    wgt, rsum, v = _cuda(p.wgt), _cuda(p.rsum), _cuda(p.v)
    n = p.v.size
    out = _out(n)
    L.random_walk(wgt, rsum, v, out, c.N, c.planes, c.h, c.w, c.r, c.logt)
    got = _np(out[:n]).reshape(p.v.shape)
    _check(f"walk {c.name} ({c.model})", got, p.ref, p.bar)
    assert _guard_ok(out, n) and torch.equal(v, _cuda(p.v))
    const = float(p.v[0, 0, 0])
    assert np.abs(got[0, 0] - const).max() <= p.bar[0, 0].max() + np.abs(p.ref[0, 0] - const).max()
    if c.logt == 6:
        buf = _out(n)
        buf[:n] = v.reshape(-1)
        L.random_walk(wgt, rsum, buf, buf, c.N, c.planes, c.h, c.w, c.r, c.logt)
        same = torch.equal(buf[:n], out[:n])
        print(f"walk {c.name} in_place: bit-equal {same}")
        assert same and _guard_ok(buf, n)


# ------------------------------------------------------------------------------------------------------------------ pool
@pytest.mark.parametrize("c", X.POOL_CASES, ids=_id)
def test_rw_pool(c):
    """the bg plane over the image, class planes from repeated sources, zero planes, zero padding; a null CAM buffer when no plane needs one"""
    from wseg_amd import _lib as L
    p = _problem(X.pool_problem, c)
    n = 21 * c.dh * c.dw
    pooled = _out(n)
    L.rw_pool(_cuda(p.cams) if c.ncam else None, c.src, c.bg, pooled, c.H, c.W, c.dh, c.dw)
    got = _np(pooled[:n]).reshape(21, c.dh, c.dw)
    _check(f"pool {c.name}", got, p.ref, p.bar)
    assert _guard_ok(pooled, n)
    zero = [k for k in range(1, 21) if c.src[k] < 0]
    assert bool((got[zero] == 0).all())


# ------------------------------------------------------------------------------------------------------------------ finish
def _judge_argmax(tag, pred, fin):
    diff = pred != fin.arg
    print(f"{tag}: unjudged share {fin.unjudged:.5f}, arg-max differs on {int(diff.sum())} pixels, {int((diff & fin.judged).sum())} of them judged")
    assert fin.unjudged <= X.FINISH_UNJUDGED_MAX
    assert not (diff & fin.judged).any(), tag


@pytest.mark.parametrize("c", X.FINISH_CASES, ids=_id)
def test_rw_finish(c):
    """planes 1 / 2 / 20 / 21 / 32, dh = 1, sides that are and are not multiples of 8: the arg-max agrees wherever the float64 margin exceeds
    twice the value bar; bitwise-equal planes holding the maximum return the lower index on every pixel; all planes equal return 0"""
    from wseg_amd import _lib as L
    p = _problem(X.finish_problem, c)
    n = c.H * c.W
    pred = torch.full((n + NG,), 255, device="cuda", dtype=torch.uint8)
    L.rw_finish(_cuda(p.cam), pred, c.planes, c.dh, c.dw, c.H, c.W)
    got = _np(pred[:n]).reshape(c.H, c.W)
    assert bool((pred[n:] == 255).all())
    if c.kind == "equal":
        print(f"finish {c.name}: all planes equal -> {int(got.max())}")
        assert (got == 0).all()
        return
    _judge_argmax(f"finish {c.name}", got, p.ref)
    if c.kind == "dup":
        assert (got == c.dup[0]).all()


# ------------------------------------------------------------------------------------------------------------------ composed
@pytest.mark.parametrize("c", X.COMPOSED_CASES, ids=_id)
def test_pool_prepare_walk_finish_composed(c):
    """rw_pool -> rw_prepare -> random_walk -> rw_finish on one image against the float64 chain with the summed bars (radius 4 and 5)"""
    from wseg_amd import _lib as L
    p = _problem(X.composed_problem, c)
    g = p.g
    n = 21 * g.area
    pooled, cam = _out(n), _out(n)
    wgt, rsum = _out(2 * g.P * g.area), _out(g.area)
    pred = torch.full((c.H, c.W), 255, device="cuda", dtype=torch.uint8)
    L.rw_pool(_cuda(p.cams), c.src, 0.27, pooled, c.H, c.W, p.dh, p.dw)
    L.rw_prepare(_cuda(p.aff), wgt, rsum, 1, p.dh, p.dw, c.r, c.beta)
    L.random_walk(wgt, rsum, pooled, cam, 1, 21, p.dh, p.dw, c.r, c.logt)
    L.rw_finish(cam, pred, 21, p.dh, p.dw, c.H, c.W)
    _check(f"composed {c.name} pooled", _np(pooled[:n]).reshape(21, -1), p.pooled, p.bar_pool)
    _check(f"composed {c.name} cam_rw", _np(cam[:n]).reshape(21, -1), p.cam, p.bar_cam)
    _judge_argmax(f"composed {c.name} pred", _np(pred), p.fin)
    assert _guard_ok(pooled, n) and _guard_ok(cam, n) and len(np.unique(p.fin.arg)) >= 3
