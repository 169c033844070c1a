"""The operand sets a gradient tap adds to the backbone's backward (Engine.run_trunk_backward): `r_pre` on the two-source data gradients of b5
and b6 (bf16 mode) and on the epilogue-0 data gradient of the skip conv (fp32 / split-bf16 modes), alone and through wseg_conv_bwd_pair.

Judged as tests/test_gpu_conv_f64.py judges every conv launch: float64 reference and derived bar of tests/conv_f64.py (accumulation over
K = IC KH KW + IC2, then the epilogue's roundings in the kernels' order: the tap's addition first, then scale and mask), every element
compared.  The shapes are the network's channel counts on maps of 99 rows (one partial tile, a row tail) and 286 rows (a tile boundary);
the intended kernel is asserted through the plan queries.  In bf16 the paired launch is made to take the joint grid (tile_hint = 256 on its
weight gradient: at these row counts the planner would otherwise fall back to two launches); in the f32 modes the pair entry point runs the
two ordinary launches, which is what the engine's callers get there.
"""
from types import SimpleNamespace

import pytest
import torch

from tests import conv_f64 as X
from tests.test_gpu_conv import ROWS_64_128, TILE_256, WGRAD_128, WGRAD_PIPE
from tests.test_gpu_conv_f64 import _check, _launch_kw, _weights

pytestmark = pytest.mark.gpu

# name: (dtype, Cin, Cout of the conv whose data gradient is launched, k, IC2, epilogue, (cin, cout) of the skip conv c1 of the pair, which
# operand is c1's dY).  b5: d_t = dgrad_3x3(du 512; W_2a) + D 1024 . W_branch1; b6: d_t = D 2048 . W_branch1 + du1 512 . W_branch2a
SHAPES = {
    "b5_two_source": ("bf16", 512, 512, 3, 1024, 1, (512, 1024), "in2"),
    "b6_two_source": ("bf16", 1024, 2048, 1, 512, 1, (1024, 2048), "in"),
    "c1_epi0_f32": ("f32", 512, 1024, 1, 0, 0, (512, 1024), "in"),
    "c1_epi0_x3": ("x3", 512, 1024, 1, 0, 0, (512, 1024), "in"),
}
MAPS = [(1, 9, 11), (2, 13, 11)]
RUNS = [(s, m) for s in SHAPES for m in MAPS]
_problems = {}


def _problem(shape, N, H, W):
    """operands, the float64 reference and bar with a random tap, and the pair's weight-gradient reference: computed once, never written to"""
    key = (shape, N, H, W)
    if key in _problems:
        return _problems[key]
    dt, Cin, Cout, k, IC2, epi, (c1_in, c1_out), dy_of = SHAPES[shape]
    c = X._case(f"{shape}_{N}x{H}x{W}", "dgrad", dt, N, H, W, Cin, Cout, k, 1, 1, (0,), IC2=IC2)
    p = X.conv_problem(c)
    tdt = X.TORCH_DT[dt]
    ep = dict(epi=epi, relu_out2=1, relu_lt=0, want_out=True, want_out2=False)
    if epi == 1:
        ep.update(scale=X.rand((c.out_ch,), 6) + 1.5, mask=X.rand((p.M, c.out_ch), 9).to(tdt))
    p.ep_plain = dict(ep)
    p.tap = X.rand((p.M, c.out_ch), 5).to(tdt)
    p.ep = dict(ep, r_pre=p.tap)
    p.refs = X.epilogue(p, p.y, p.e0, torch.float64)
    # the pair: the skip conv's weight gradient dW[oc][ic] = sum_m D[m, oc] t[m, ic] (1x1) of the same D
    p.t = X.rand((p.M, c1_in), 21).to(tdt)
    p.D = torch.cat([X.rows(x) for x in (p.x2s if dy_of == "in2" else p.xs)]).contiguous()
    assert p.D.shape == (p.M, c1_out)
    w = SimpleNamespace(c=SimpleNamespace(dt=dt), n_pix=p.M, ref=(p.D.double().t() @ p.t.double()).reshape(c1_out, 1, c1_in),
                        A=(p.D.double().abs().t() @ p.t.double().abs()).reshape(c1_out, 1, c1_in))
    p.wg = w
    p.wkw = dict(N=N, IH=H, IW=W, IC=c1_in, OH=H, OW=W, OC=c1_out, KH=1, KW=1)
    _problems[key] = p
    return p


@pytest.mark.parametrize("shape,geo", RUNS, ids=[f"{s}-{n}x{h}x{w}" for s, (n, h, w) in RUNS])
def test_tap_operand_set(shape, geo):
    from wseg_amd import _lib as L
    p, dev = _problem(shape, *geo), "cuda"
    c = p.c
    tdt = X.TORCH_DT[c.dt]
    two_src, bf16 = c.IC2 > 0, c.dt == "bf16"
    family = TILE_256 if two_src else ROWS_64_128
    inp = torch.cat([X.rows(x) for x in p.xs]).contiguous().to(dev)
    wt = _weights(p, dev)

    def launch(ep, pair=None):
        p_ = SimpleNamespace(**{**vars(p), "ep": ep})
        kw = _launch_kw(p_, 0, dev)
        out = torch.full((p.M, c.out_ch), float("nan"), device=dev, dtype=tdt)
        if pair is None:
            plan = L.conv_plan(inp, wt, out, None, **kw)
            assert plan.family in family, (plan, family)
            L.conv_igemm(inp, wt, out, None, **kw)
        else:
            fused, dg, wg = L.conv_pair_plan(pair[3], inp, wt, out, None, **kw)
            assert dg.family in family and fused == int(bf16), (fused, dg, wg)
            assert wg.family == (WGRAD_PIPE if bf16 else WGRAD_128), wg
            L.conv_igemm(inp, wt, out, None, pair_wgrad=pair, **kw)
            return out, wg.nsplit
        return out

    plain = launch(p.ep_plain)
    zero = launch(dict(p.ep_plain, r_pre=torch.zeros_like(p.tap)))
    assert torch.equal(plain, zero), "an all-zero tap must leave the launch's result bit for bit"
    alone = launch(p.ep)
    _check(f"{c.name} tap, alone", alone, *p.refs["out"])
    # through wseg_conv_bwd_pair: the same dX, and the skip conv's weight gradient beside it
    wkw = dict(p.wkw, dtype=L.F32X3 if c.dt == "x3" else None, **(dict(tile_hint=256) if bf16 else {}))
    dw = torch.zeros(p.wg.ref.shape, device=dev, dtype=torch.float32)
    D_dev = p.D.to(dev)
    paired, nsplit = launch(p.ep, pair=(p.t.to(dev), D_dev, dw, wkw))
    assert torch.equal(paired, alone), "the paired launch's dX must equal the stand-alone launch's bit for bit"
    _check(f"{c.name} pair dw ({nsplit} splits)", dw, *X.wgrad_bar(p.wg, nsplit))
