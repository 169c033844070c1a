"""The DeepLab head's conv launches (Engine.run_seg_head) through the C ABI against float64, with the references and the DERIVED bars of
tests/conv_f64.py (storage rounding + accumulation + epilogue arithmetic; nothing fitted).  conv_fov is the project's first launch at
dilation 12, and its K = 9 x 4096 = 36864 is four times the longest K any other launch walks:
  * 3x3, dilation 12, pad 12 at IC 128 on maps 5 x 7 (only the centre tap ever in range), 13 x 16 (+-12 reaches one row / column) and
    28 x 31 (both sides in range), N = 2, on every tile family the planner can choose for the dtype, with the folded-BatchNorm + ReLU
    epilogue written to `out2` only, as the engine launches it;
  * once per dtype at the real IC = 4096, OC = 512 on 5 x 7 (the planner's choice);
  * cls_conv's pack zero-padded to 24 rows: 1x1, 512 -> 24, the bias as `shift` with no scale and relu_out2 = 0.
Every element of every output is compared; outputs start as NaN."""
import pytest
import torch

from tests import conv_f64 as X
from tests.test_gpu_conv import CONV_FAMILY, ROWS_64_128, _conv

pytestmark = pytest.mark.gpu

FAMS = {"bf16": (64, 128, 224, 256), "f32": (64, 128), "x3": (64, 128, 224, 256)}
MAPS = [(5, 7), (13, 16), (28, 31)]
DIL = 12


def _cases():
    out = []
    for dt in ("bf16", "f32", "x3"):
        for (h, w) in MAPS:
            out.append((X._case(f"fov_{h}x{w}_{dt}", "fwd", dt, 2, h, w, 128, 256, 3, 1, DIL, FAMS[dt]), "bn_relu"))
        out.append((X._case(f"fov_real_{dt}", "fwd", dt, 1, 5, 7, 4096, 512, 3, 1, DIL, (0,)), "bn_relu"))
        for (h, w) in MAPS[:2]:
            out.append((X._case(f"cls_{h}x{w}_{dt}", "fwd", dt, 2, h, w, 512, 24, 1, 1, 1, (0,)), "bias"))
    return out


RUNS = [(c, kind, bm) for c, kind in _cases() for bm in c.fams]
_problems = {}


def _problem(c, kind):
    """operands, float64 reference and bar of a case, computed once and shared by the families that run it; the epilogue is the head's:
    out2 only — relu(v * scale + shift) (a folded BatchNorm) or v + shift (cls_conv's bias: no scale, no ReLU)"""
    if c.name not in _problems:
        p = X.conv_problem(c)
        shift = X.rand((c.out_ch,), 7)
        if kind == "bn_relu":
            p.ep.update(scale=X.rand((c.out_ch,), 6) + 1.5, shift=shift, relu_out2=1, want_out=False, want_out2=True)
        else:
            p.ep.update(scale=torch.ones(c.out_ch), shift=shift, relu_out2=0, want_out=False, want_out2=True)
        p.refs = X.epilogue(p, p.y, p.e0, torch.float64)
        assert set(p.refs) == {"out2"}
        _problems[c.name] = p
    return _problems[c.name]


def test_geometry_of_the_cases():
    """what the three maps are chosen for: the share of output pixels that have an off-centre tap in range"""
    for (h, w), want in zip(MAPS, ("none", "some", "both")):
        ys, xs = torch.arange(h), torch.arange(w)
        up, down, left, right = ys - DIL >= 0, ys + DIL < h, xs - DIL >= 0, xs + DIL < w
        if want == "none":
            assert not (up.any() or down.any() or left.any() or right.any())
        elif want == "some":
            assert int(up.sum()) == int(down.sum()) == 1 and int(left.sum()) == int(right.sum()) == 4 and not (up & down).any()
        else:
            assert bool((up & down).any()) and bool((left & right).any()) and int(up.sum()) == h - DIL and int(left.sum()) == w - DIL


@pytest.mark.parametrize("c,kind,bm", RUNS, ids=[f"{c.name}-{bm}" for c, _k, bm in RUNS])
def test_head_conv_f64(c, kind, bm):
    from wseg_amd import _lib as L
    p, dev = _problem(c, kind), "cuda"
    tdt = X.TORCH_DT[c.dt]
    (h, w), = c.sizes
    kw = dict(N=c.N, IH=h, IW=w, IC=c.in_ch, OH=h, OW=w, OC=c.out_ch, KH=c.k, KW=c.k, stride=1, dil=c.d, pad=c.d * (c.k // 2), bm_hint=bm,
              relu_out2=p.ep["relu_out2"], shift=p.ep["shift"].to(dev), dtype=L.F32X3 if c.dt == "x3" else None)
    if kind == "bn_relu":
        kw["scale"] = p.ep["scale"].to(dev)
    wp = p.w.permute(0, 2, 3, 1).reshape(c.out_ch, -1).contiguous().to(dev)
    if c.dt == "x3":
        w32, wp = wp, torch.empty_like(wp)
        L.pack_x3(w32, wp)
    inp = X.rows(p.xs[0]).contiguous().to(dev)
    out2 = torch.full((p.M, c.out_ch), float("nan"), device=dev, dtype=tdt)
    _conv(CONV_FAMILY[bm] if bm else ROWS_64_128 + (3, 4), inp, wp, None, out2, **kw)
    ref, bar = p.refs["out2"]
    err = (out2.double().cpu() - ref).abs()
    print(f"{c.name} bm={bm}: max err {float(err.max()):.3e}, max err/bar {float((err / bar).max()):.3f}, K = {c.K}")
    assert bool((err <= bar).all())
    if kind == "bn_relu":
        assert 0.2 < float((ref > 0).double().mean()) < 0.95          # the ReLU cuts some and passes some
