"""The contrast net's head passes (Engine.run_forward behind _run_trunk, Engine.run_backward in front of _trunk_backward) stage by stage against
float64 in every precision mode.  Each stored tensor — head, feat, cam_low / cmax, G, Fm, Fh / nrm, Fb / Gb / Gl, rvd / den, cam / cam_rv; in
the backward d_cam_low / d_rvd, DN / dFh, dF, d_feat, d_head_rows, D and the five head weight gradients — is compared AT EVERY ELEMENT with the
float64 statement of its stage (tests/head_f64.py, written from oracle/net.py and pinned to it by tests/test_head_host.py), computed from the
tensors the device stored for that stage's inputs, inside the bars the kernel tests derive.  No bar is fitted.

The Recorder wraps _Pass.conv / dgrad / wgrad, L.conv_wgrad and the head entry points the engine calls through L (a monkeypatch, undone at the
end of the test) and keeps references to the tensors of every call.  ONLY ROLES are read from it: which device tensor is head, feat, G, Fm ...,
and that a per-view launch was handed the rows of ITS view (storage offsets).  The weights are the module's parameters rounded as the mode
stores them (never the packs), s7 is P["bn"]["bn7"] once judged against the float64 fold, dropout7 is S["masks"] (the injected tables), the
weight-gradient splits are L.wgrad_plan's.  The PCM branch of the backward runs on its own stream: everything is read after a synchronize.

Geometry: the trunk test's.  Two views 100 x 76 and 44 x 28, N = 2, procedural weights: 308 stride-8 rows, PCM maps 13 x 10 (hw = 130, a partial
tile) and 6 x 4 (one partial tile), neither a multiple of 4, view 2 at row offset 260; the autograd entry runs one view 84 x 60.  The dropout
tables are injected (synthetic_dropout_masks), so tests/test_head_host.py checks the band and near-tie conditions for the same inputs.

Cost.  Measured per case on an MI355X host (16 cores), pytest's call time: 0.8 - 0.9 s for the first case of a mode, which builds that mode's
net (2.3 s for the first of the run), and 1.2 s for the first autograd case of the run; every other case 0.01 - 0.06 s (the fused backward
entry 0.06 s, the autograd entry 0.04 - 0.05 s, the inference path 0.01 - 0.02 s), of which the float64 references take 0.01 - 0.03 s
(M = 308 rows: the head is small beside the trunk).  The per-stage table of that run: profiles/r26_head_stages_f64.txt."""
import time

import pytest
import torch

from tests import head_f64 as H
from tests import trunk_f64 as T
from tests.f64_bars import _gen
from tests.test_gpu_trunk_stages import DEV, MODES, ONE_VIEW, TDT, VIEWS, _net
from tests.test_head_host import IMG_SEED, MASK_SEED, common_gradient
from wseg_amd import synth

pytestmark = pytest.mark.gpu
N = 2
L_ENTRIES = ("head_split", "cam_gate", "pcm_xs", "l2norm_forward", "l2norm_backward", "to_bf16", "split_bf16", "pcm_forward", "pcm_forward_bf16",
             "pcm_backward", "pcm_backward_bf16", "resize_planar_fwd", "resize_planar_bwd", "head_grad_rows")


def _is_rows_of(t, base, elems):
    """t starts `elems` elements into base's storage"""
    return t.untyped_storage().data_ptr() == base.untyped_storage().data_ptr() and t.storage_offset() == base.storage_offset() + elems


def _same(a, b):
    """the same device tensor: one object, or two views of the same elements (G[0:] is G)"""
    if a is b:
        return True
    return torch.is_tensor(a) and torch.is_tensor(b) and a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.dtype == b.dtype and a.stride() == b.stride()


class Recorder:
    def __init__(self, monkeypatch, eng):
        from wseg_amd import _lib as L, engine as E
        self.eng, self.convs, self.dgrads, self.wgrads, self.calls, self.launches = eng, {}, {}, {}, {k: [] for k in L_ENTRIES}, {}
        self.S = self.trunk_tap = None
        conv0, dgrad0, wgrad0, wg0, rb0, tb0 = E._Pass.conv, E._Pass.dgrad, E._Pass.wgrad, L.conv_wgrad, E.Engine.run_backward, E.Engine._trunk_backward
        rec = self

        def conv(ps, c, inp, out, out2=None, **kw):
            rec.convs[c.name] = (inp, out, out2)
            return conv0(ps, c, inp, out, out2, **kw)

        def dgrad(ps, c, dy, out, pair=None, **kw):
            rec.dgrads[c.name] = (dy, out)
            return dgrad0(ps, c, dy, out, pair=pair, **kw)

        def wgrad(ps, c, x, dy, **kw):
            rec.wgrads[c.name] = (x, dy)
            return wgrad0(ps, c, x, dy, **kw)

        def conv_wgrad(x, dy, dw, **kw):
            if dw.untyped_storage().data_ptr() == eng.flat_g.untyped_storage().data_ptr():
                rec.launches.setdefault(dw.storage_offset(), []).append((x, dy, L.wgrad_plan(x, dy, dw, **kw).nsplit))
            return wg0(x, dy, dw, **kw)

        def run_backward(self_, S, grads, d_head_rows=None):
            rec.S = S
            return rb0(self_, S, grads, d_head_rows)

        def trunk_backward(self_, ps, S, taps):
            rec.trunk_tap = taps["conv6"]
            return tb0(self_, ps, S, taps)

        def entry(name, fn0):
            def f(*a, **kw):
                rec.calls[name].append(a)
                return fn0(*a, **kw)
            return f

        monkeypatch.setattr(E._Pass, "conv", conv)
        monkeypatch.setattr(E._Pass, "dgrad", dgrad)
        monkeypatch.setattr(E._Pass, "wgrad", wgrad)
        monkeypatch.setattr(L, "conv_wgrad", conv_wgrad)
        monkeypatch.setattr(E.Engine, "run_backward", run_backward)
        monkeypatch.setattr(E.Engine, "_trunk_backward", trunk_backward)
        for name in L_ENTRIES:
            monkeypatch.setattr(L, name, entry(name, getattr(L, name)))

    # ---- roles
    def forward_record(self, xs, lowres, bf16, save):
        """the device tensors of the forward's stages, by the launches' names and arguments"""
        c, k = self.convs, self.calls
        dims = [(x.shape[2] // 8 + (x.shape[2] % 8 > 0), x.shape[3] // 8 + (x.shape[3] % 8 > 0)) for x in xs]
        r = dict(N=N, dims=dims, xs=xs, lowres=lowres, fea=c["head"][0], head=c["head"][1], conv4=c["f8_3"][0], conv5=c["f8_4"][0],
                 feat=c["f8_3"][1], Fm=c["f9"][1], cam_low=[], cmax=[], rvd=[], den=[], cam=[], cam_rv=[])
        M = sum(n for _o, n, _h, _w in H.view_rows(N, dims))
        assert r["fea"].shape == (M, 4096) and r["head"].shape == (M, H.HEAD_LD) and r["feat"].shape == (M, H.FEAT_LD) and r["Fm"].shape == (M, 192)
        assert _same(c["f9"][0], r["feat"]) and _is_rows_of(c["f8_4"][1], r["feat"], 64)
        assert _same(r["fea"], c["b7.conv_branch2b2" if "b7.conv_branch2b2" in c else "b7.skip_fused"][2])       # relu(bn7(conv6)) . dropout7 of the trunk
        assert _same(r["conv4"], c["b5.conv_branch2a"][0]) and _same(r["conv5"], c["b6.conv_branch2a"][0])
        views = H.view_rows(N, dims)
        assert all(len(k[n]) == len(xs) for n in ("head_split", "cam_gate", "pcm_xs"))
        r["G"] = k["cam_gate"][0][2]
        assert r["G"].shape == (M, 32)
        for i, (off, n, h, w) in enumerate(views):
            hs, cg, px = k["head_split"][i], k["cam_gate"][i], k["pcm_xs"][i]
            assert _is_rows_of(hs[0], r["head"], off * H.HEAD_LD) and hs[1:3] == (H.HEAD_LD, 128) and hs[5:] == (N, h * w)
            r["cam_low"].append(hs[3]); r["cmax"].append(hs[4])
            assert _same(cg[0], hs[3]) and _same(cg[1], hs[4]) and _is_rows_of(cg[2], r["G"], off * 32) and cg[3:] == (N, h * w)
            assert px[0].data_ptr() == xs[i].data_ptr() and _is_rows_of(px[1], r["feat"], off * H.FEAT_LD) and px[2:] == (H.FEAT_LD, 192, H.FEAT_LD, N) + tuple(xs[i].shape[2:]) + (h, w)
        (l2,) = k["l2norm_forward"]
        assert _same(l2[0], r["Fm"]) and l2[1] == 192 and l2[4] == M
        r["Fh"], r["nrm"] = l2[2], l2[3]
        Fp, Gp, fwd = r["Fh"], r["G"], k["pcm_forward"]
        if bf16:
            (fb,) = [a for a in k["to_bf16"] if _same(a[0], r["Fh"])]
            r["Fb"] = Fp = fb[1]
            if save:
                (sp,) = [a for a in k["split_bf16"] if _same(a[0], r["G"])]
                r["Gb"], r["Gl"] = sp[1], sp[2]
            else:
                (gb,) = [a for a in k["to_bf16"] if _same(a[0], r["G"])]
                r["Gb"] = gb[1]
            Gp, fwd = r["Gb"], k["pcm_forward_bf16"]
            assert not k["pcm_forward"]
        else:
            assert not k["pcm_forward_bf16"] and not [a for a in k["to_bf16"] if _same(a[0], r["Fh"])]
        assert len(fwd) == len(xs)
        for (off, n, h, w), a in zip(views, fwd):
            assert _is_rows_of(a[0], Fp, off * 192) and _is_rows_of(a[1], Gp, off * 32) and a[4:] == (N, h * w)
            r["rvd"].append(a[2]); r["den"].append(a[3])
        if not lowres:
            rs = k["resize_planar_fwd"]
            assert len(rs) == 2 * len(xs)
            for i, x in enumerate(xs):
                a, b = rs[2 * i], rs[2 * i + 1]
                assert _same(a[0], r["cam_low"][i]) and _same(b[0], r["rvd"][i]) and a[2:] == b[2:] == (N * 21,) + dims[i] + tuple(x.shape[2:]) + (True,)
                r["cam"].append(a[1]); r["cam_rv"].append(b[1])
        else:
            assert not k["resize_planar_fwd"]
        return r

    def backward_record(self, r, grads, d_head_rows, bf16):
        """adds the backward's tensors to the forward record r: the PCM backward's operands as IT was handed them, the gradients read from flat_g"""
        eng, k, S = self.eng, self.calls, self.S
        views = H.view_rows(N, r["dims"])
        M = r["fea"].shape[0]
        assert _same(S["fea"], r["fea"]) and _same(S["feat"], r["feat"]) and _same(S["head"], r["head"]) and _same(S["conv4"], r["conv4"]) and _same(S["conv5"], r["conv5"])
        fwd_rvd, fwd_den = r["rvd"], r["den"]
        r.update(d_cam_low=[], dr=[], d_rvd=[], rvd=[], den=[])
        if not r["lowres"]:
            rb = k["resize_planar_bwd"]
            assert len(rb) == 2 * len(views)
            for i, (g_cam, g_cam_rv, _gf, _gr) in enumerate(grads):
                a, b = rb[2 * i], rb[2 * i + 1]
                assert torch.equal(a[0], g_cam) and torch.equal(b[0], g_cam_rv)
                r["d_cam_low"].append(a[1]); r["dr"].append(b[1])
            r["g"] = grads
        pb = k["pcm_backward_bf16" if bf16 else "pcm_backward"]
        assert len(pb) == len(views) and not k["pcm_backward" if bf16 else "pcm_backward_bf16"]
        for i, ((off, n, h, w), a) in enumerate(zip(views, pb)):
            if bf16:
                Fb, Gb, Gl, dr, rvd, den, DN, DNb, DNl, dFh = a[:10]
                assert _is_rows_of(Fb, r["Fb"], off * 192) and _is_rows_of(Gb, r["Gb"], off * 32) and _is_rows_of(Gl, r["Gl"], off * 32)
            else:
                Fh, G, dr, rvd, den, DN, dFh = a[:7]
                assert _is_rows_of(Fh, r["Fh"], off * 192) and _is_rows_of(G, r["G"], off * 32)
            assert a[-2:] == (N, h * w)
            if i == 0:
                r["DN"], r["dFh"] = DN, dFh
                if bf16:
                    r["DNb"], r["DNl"] = DNb, DNl
            assert _is_rows_of(DN, r["DN"], off * 32) and _is_rows_of(dFh, r["dFh"], off * 192)
            assert not bf16 or (_is_rows_of(DNb, r["DNb"], off * 32) and _is_rows_of(DNl, r["DNl"], off * 32))
            assert torch.equal(rvd, fwd_rvd[i]) and torch.equal(den, fwd_den[i])          # (a clone outside the stride-8 form)
            r["d_rvd"].append(dr); r["rvd"].append(rvd); r["den"].append(den)
        assert r["DN"].shape == (M, 32) and r["dFh"].shape == (M, 192)
        (lb,) = k["l2norm_backward"]
        assert _same(lb[0], r["Fm"]) and _same(lb[2], r["dFh"]) and _same(lb[3], r["nrm"]) and (lb[1], lb[5], lb[6]) == (192, 192, M)
        r["dF"] = lb[4]
        assert _same(self.wgrads["f9"][0], r["feat"]) and _same(self.wgrads["f9"][1], r["dF"]) and _same(self.dgrads["f9"][0], r["dF"])
        r["d_feat"] = self.dgrads["f9"][1]
        assert r["d_feat"].shape == (M, H.FEAT_LD)
        assert _same(self.wgrads["f8_3"][0], r["conv4"]) and _same(self.wgrads["f8_3"][1], r["d_feat"])
        assert _same(self.wgrads["f8_4"][0], r["conv5"]) and _is_rows_of(self.wgrads["f8_4"][1], r["d_feat"], 64)
        r["d_head_rows"], r["D"] = self.dgrads["head"]
        if d_head_rows is not None:
            assert _same(r["d_head_rows"], d_head_rows) and not k["head_grad_rows"]
        else:
            assert len(k["head_grad_rows"]) == len(views)
            for (off, n, h, w), a, dc in zip(views, k["head_grad_rows"], r["d_cam_low"]):
                assert _same(a[1], dc) and _is_rows_of(a[2], r["head"], off * H.HEAD_LD) and _is_rows_of(a[3], r["d_head_rows"], off * H.HEAD_LD)
        assert _same(self.trunk_tap, r["D"])                       # the conv6 tap handed to _trunk_backward: the judged D
        r["splits"] = {}
        for name, (co, ci) in (("f9", (192, 195)), ("f8_3", (64, 512)), ("f8_4", (128, 1024)), ("fc_proj", (128, 4096)), ("fc8", (21, 4096))):
            r["dW_" + name] = eng.grad_slice(name).view(co, ci)
            if name != "fc8":                                 # (fc8's rows ride in fc_proj's launch)
                (launch,) = self.launches[eng.offsets[name][0]]
                r["splits"][name] = launch[2]
        (hx, hdy, _n), = self.launches[eng.offsets["fc_proj"][0]]
        assert _same(hx, r["fea"]) and _same(hdy, r["d_head_rows"]) and eng.offsets["fc8"][0] == eng.offsets["fc_proj"][0] + 128 * 4096
        return r


def _cpu(r):
    conv = lambda v: v.detach().double().cpu() if torch.is_tensor(v) else v
    out = {}
    for key, v in r.items():
        if isinstance(v, list) and v and isinstance(v[0], tuple):
            out[key] = [tuple(conv(t) for t in g) for g in v]
        elif isinstance(v, list):
            out[key] = [conv(t) for t in v]
        else:
            out[key] = conv(v)
    return out


def _setup(mode, views, train):
    net = _net("contrast", mode)
    net.train() if train else net.eval()
    dev = torch.device(DEV, torch.cuda.current_device())
    eng = net._engine.active(dev)
    masks = [synth.synthetic_dropout_masks(N, MASK_SEED + i) for i in range(len(views))]
    eng.injected_masks = list(masks) if train else None
    xs = [synth.synthetic_images(N, hw, IMG_SEED + i).cuda() for i, hw in enumerate(views)]
    W = H.weights64({n: eng.conv_param(n) for n in H.HEAD_CONVS}, mode)
    return net, eng, xs, masks, W


def _operands(net, eng, mode, S, masks, r):
    """s7 from P["bn"]["bn7"], judged against the float64 fold; dropout7 from S["masks"], which must be the injected tables"""
    from wseg_amd.engine import DT_OF
    P = eng.ensure_packs(torch.device(DEV, torch.cuda.current_device()), DT_OF[mode])
    sd = net.state_dict()
    s7 = P["bn"]["bn7"][0].double().cpu()
    assert bool(((s7 - T.fold64(sd, "bn7")[0]).abs() <= T.fold_bar(sd, "bn7")[0]).all())
    d7 = S["masks"]["dropout7"].double().cpu()
    assert torch.equal(d7, torch.cat([m["dropout7"] for m in masks]).double()) and bool(((d7 == 0) | (d7 == 2)).all())
    r.update(s7=s7, drop7=d7)


def _report(tag, mode, table, info, seconds):
    for kind, (ratio, where) in sorted(H.worst(table).items()):
        print(f"[{tag} {mode}] worst {kind:12s} err / bar {ratio:.4f} at {where}")
    if "pairs" in info:
        print(f"[{tag} {mode}] pairs inside the gate band: {info['band']} of {info['pairs']}")
    if "gate_entries" in info:
        print(f"[{tag} {mode}] gate decisions other than float64's: {info['gate_differs']} of {info['gate_entries']}")
    print(f"[{tag} {mode}] {len(table)} stored tensors judged, float64 reference {seconds:.2f} s")
    bad = [row for row in table if not row[3]]
    assert not bad, bad
    assert info.get("band", 0) <= H.BAND_CAP * info.get("pairs", 1), info


def _mk(shape, seed, dtype):
    """random values in [-1, 1) that bf16 holds: one functional in all modes"""
    return (torch.rand(shape, generator=_gen(seed)) * 2 - 1).bfloat16().to(dtype).cuda()


@pytest.mark.parametrize("mode", MODES)
def test_head_forward_two_views(monkeypatch, mode):
    """training mode, run_forward(xs, save=True, lowres=True): every forward stage of both views at every element"""
    net, eng, xs, masks, W = _setup(mode, VIEWS, True)
    rec = Recorder(monkeypatch, eng)
    with torch.no_grad():
        outs, S = eng.run_forward(xs, save=True, lowres=True)
    torch.cuda.synchronize()
    r = rec.forward_record(xs, True, mode == "bf16", True)
    assert r["dims"] == [(13, 10), (6, 4)] and H.view_rows(N, r["dims"])[1][0] == 260 and r["fea"].shape[0] == 308
    for i, o in enumerate(outs):                              # what the pass returns is what was judged
        assert _same(o[0], r["cam_low"][i]) and _same(o[1], r["rvd"][i]) and _is_rows_of(o[3], r["head"], H.view_rows(N, r["dims"])[i][0] * H.HEAD_LD)
    assert _same(S["G"], r["G"]) and _same(S["Fh"], r["Fh"]) and _same(S["Fm"], r["Fm"]) and _same(S["nrm"], r["nrm"]) and _same(S["Gl"], r.get("Gl"))
    t0, info = time.perf_counter(), {}
    table = H.judge(mode, _cpu(r), W, backward=False, info=info)
    _report("head forward", mode, table, info, time.perf_counter() - t0)
    tags = {row[0].split(".")[0] for row in table}
    assert tags == {"head", "feat", "cam_low", "cmax", "G", "Fm", "Fh", "nrm", "rvd", "den"} | ({"Fb", "Gb", "Gl"} if mode == "bf16" else set())
    assert bool((r["head"][:, 149:] == 0).all()) and bool((r["feat"][:, 195:] == 0).all())


@pytest.mark.parametrize("mode", MODES)
def test_head_backward_fused_entry(monkeypatch, mode):
    """the production entry run_backward(S, [(None, d_rvd, None, None)] * 2, d_head_rows=...): every backward stage and all five head weight
    gradients, the conv6 tap handed to the trunk's backward"""
    net, eng, xs, masks, W = _setup(mode, VIEWS, True)
    rec = Recorder(monkeypatch, eng)
    with torch.no_grad():
        _outs, S = eng.run_forward(xs, save=True, lowres=True)
        r = rec.forward_record(xs, True, mode == "bf16", True)
        M = r["fea"].shape[0]
        d_rvd = [_mk((N, 21, h, w), 93 + i, torch.float32) for i, (h, w) in enumerate(r["dims"])]
        dhr = _mk((M, H.HEAD_LD), 95, TDT[mode])
        dhr[:, 149:] = 0
        eng.attach_grads()
        eng.flat_g.zero_()
        eng.run_backward(S, [(None, d, None, None) for d in d_rvd], d_head_rows=dhr)
    torch.cuda.synchronize()
    assert rec.S is S
    rec.backward_record(r, None, dhr, mode == "bf16")
    assert all(_same(a, b) for a, b in zip(r["d_rvd"], d_rvd))
    _operands(net, eng, mode, S, masks, r)
    t0, info = time.perf_counter(), {}
    table = H.judge(mode, _cpu(r), W, forward=False, info=info)
    _report("head backward, fused entry", mode, table, info, time.perf_counter() - t0)
    tags = {row[0].split(".")[0] for row in table}
    assert tags == {"DN", "dFh", "dF", "dW_f9", "d_feat", "dW_f8_3", "dW_f8_4", "dW_fc_proj", "dW_fc8", "D"} | ({"DNb", "DNl"} if mode == "bf16" else set())


@pytest.mark.parametrize("mode", MODES)
def test_head_autograd_entry_one_view(monkeypatch, mode):
    """net(x) under autograd, one view 84 x 60, gradients on all four outputs: adds cam, cam_rv, d_cam_low, d_rvd (dr + g_rvd) and d_head_rows
    by head_grad_rows to the stages above.  The gradient of rvd is common to all classes (test_head_host.common_gradient): the gate product of the
    PCM backward cancels, and in bf16 mode dFh leaves its bar when Gl does not reach it (the planted defect of tests/test_head_host.py)."""
    net, eng, xs, masks, W = _setup(mode, (ONE_VIEW,), True)
    eng.attach_grads()
    eng.flat_g.zero_()
    rec = Recorder(monkeypatch, eng)
    outs = net(xs[0])
    r = rec.forward_record(xs, False, mode == "bf16", True)
    assert r["dims"] == [(11, 8)] and all(o.data_ptr() == t[0].data_ptr() for o, t in zip((outs[0], outs[1], outs[3]), (r["cam"], r["cam_rv"], r["rvd"])))
    (h, w), HW = r["dims"][0], ONE_VIEW
    grads = [common_gradient((_mk((N, 21) + HW, 96, torch.float32), _mk((N, 21) + HW, 97, torch.float32), _mk((N, 128, h, w), 98, torch.float32),
                              _mk((N, 21, h, w), 99, torch.float32)))]
    torch.autograd.backward(list(outs), list(grads[0]))
    torch.cuda.synchronize()
    S = rec.S
    assert S is not None and not S["lowres"]
    rec.backward_record(r, grads, None, mode == "bf16")
    _operands(net, eng, mode, S, masks, r)
    t0, info = time.perf_counter(), {}
    table = H.judge(mode, _cpu(r), W, info=info)
    _report("head, autograd entry", mode, table, info, time.perf_counter() - t0)
    tags = {row[0].split(".")[0] for row in table}
    assert tags >= {"cam", "cam_rv", "d_cam_low", "dr", "d_rvd", "d_head_rows", "DN", "dFh", "dF", "D", "dW_f9", "dW_f8_3", "dW_f8_4", "dW_fc_proj", "dW_fc8"}


@pytest.mark.parametrize("mode", MODES)
def test_inference_path_matches_saved_path(monkeypatch, mode):
    """net.eval(): run_forward(save=False) and run_forward(save=True) give bit-identical outputs; in bf16 mode to_bf16(G) is the hi of split_bf16(G)"""
    net, eng, xs, _masks, _W = _setup(mode, VIEWS, False)
    res = []
    for save in (False, True):
        rec = Recorder(monkeypatch, eng)
        with torch.no_grad():
            outs, _S = eng.run_forward(xs, save=save, lowres=False)
        torch.cuda.synchronize()
        r = rec.forward_record(xs, False, mode == "bf16", save)
        res.append(([t.clone() for o in outs for t in o], r.get("Gb"), r.get("Gl")))
        monkeypatch.undo()
    (o0, gb0, gl0), (o1, gb1, gl1) = res
    bits = lambda t: t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
    assert len(o0) == len(o1) == 8 and all(a.dtype == b.dtype and torch.equal(bits(a), bits(b)) for a, b in zip(o0, o1))
    if mode == "bf16":
        assert gl0 is None and gl1 is not None and torch.equal(bits(gb0), bits(gb1))
    else:
        assert gb0 is None and gb1 is None
