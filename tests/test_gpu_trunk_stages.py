"""The engine's trunk (conv1a and the 17 blocks: Engine._run_blocks, Engine._trunk_backward) stage by stage against float64 in every precision
mode.  Each stored tensor — the stem's output, every block's v / v1 / v2, the stored skip output, x_out, t_out; in the backward du / du2 /
du1, the stored skip gradient tmp, D_in and every weight gradient — is compared AT EVERY ELEMENT with the float64 statement of its stage
(tests/trunk_f64.py, written from oracle/net.py and pinned to it by tests/test_trunk_host.py), computed from the tensors the device stored for
that stage's inputs, under the device's own stored ReLU / dropout decisions, inside the bars derived in tests/conv_f64.py.  No bar is fitted.

The Recorder wraps _Pass.conv / dgrad / wgrad and L.stem_conv_kc (a monkeypatch, undone at the end of the test) and keeps, per call, the
conv's name and references to its input and output tensors.  ONLY ROLES are read from it: which tensor is a block's t, v, x_out, D, du, tmp.
Which BatchNorm, mask, tap and residual belong to a stage comes from the definition, the weights from the module's parameters rounded as
the mode stores them (never from the packs), the folded BatchNorms from P["bn"] once judged against the float64 fold; the dropout tables are
the ones the device drew (each value 0 or 1 / (1 - p)).  L.conv_wgrad and L.conv_igemm are wrapped for one thing: the plan query of the
launch they are about to make, which gives the count of weight-gradient splits the bar takes.

bf16 mode: b5, b6 and b7 run as one two-source launch forward and backward (asserted; b3 and b4 do not), and the weight gradients ride in the
data-gradient launches.  At these sizes conv_pair_plan does not fuse the pair into one grid (it needs more than 32768 pixels; what it reports
is printed): the engine's pair OPERANDS are judged here through the weight gradients, the fused grid itself by test_conv_bwd_pair_f64.

Cost.  The GPU work of a case is milliseconds; the float64 references on the CPU are the cost.  Measured per mode on the 16 cores of an
MI355X host (on 8 cores: 2.0 s and 4.7 s for the first two): contrast forward (100 x 76 + 44 x 28, N = 2, 308 stride-8 pixels) 1.2 - 1.3 s,
contrast backward 4.3 - 4.6 s, AffinityNet backbone forward and backward (84 x 60, N = 2) 3.5 - 3.8 s (with b3 frozen too: 3.2 - 3.5 s), eval forward (84 x 60, N = 1) 0.2 s.
The per-stage table of an MI355X run: profiles/r25_trunk_stages_f64.txt."""
import time

import pytest
import torch

from tests import trunk_f64 as T
from tests.f64_bars import U32, _gen
from wseg_amd import arch, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ["fp32", "bf16x3", "bf16"]
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "bf16x3": torch.float32}
VIEWS = ((100, 76), (44, 28))         # stride-4 maps 25 x 19 and 11 x 7 (odd sides), stride-8 maps 13 x 10 and 6 x 4: at 6 x 4 most taps of the dilation-4 convs are padding
ONE_VIEW = (84, 60)                   # 11 x 8 at stride 8
_NETS, _W = {}, {}


def _net(kind, mode):
    if (kind, mode) not in _NETS:
        if kind == "contrast":
            from wseg_amd.resnet38_contrast import Net
            m = Net(precision=mode)
            m.load_state_dict(synth.procedural_state_dict(0), strict=True)
        else:
            from wseg_amd.resnet38_aff import Net
            if kind == "aff_b3":                              # the AffinityNet with b3 frozen too: b3_1 is the first trainable block
                Net = type("NetB3Frozen", (Net,), {"FROZEN_BLOCKS": arch.FROZEN_BLOCKS + ("b3",)})
            m = Net(precision=mode)
            m.load_state_dict(synth.procedural_aff_state_dict(0), strict=True)
        _NETS[(kind, mode)] = m.cuda()
    return _NETS[(kind, mode)]


def _trunk_conv_names():
    return ["conv1a"] + [c[0] for b in arch.BLOCKS for c in arch.block_convs(b)]


def _weights(kind, eng, mode):
    """the trunk's weights from the module's parameters, rounded as the mode stores them (fp32 and bf16x3 store the same f32 values)"""
    key = (kind[:3], "bf16" if mode == "bf16" else "f32")             # ("aff" and "aff_b3" load the same state dict)
    if key not in _W:
        while len(_W) >= 2:                                   # (0.8 GB of float64 each)
            del _W[next(iter(_W))]
        _W[key] = T.weights64({n: eng.conv_param(n) for n in _trunk_conv_names()}, mode)
    return _W[key]


def _folds(net, eng, mode):
    """P["bn"] judged against the float64 fold of the module's state, then taken as the operand"""
    from wseg_amd.engine import DT_OF
    P = eng.ensure_packs(torch.device(DEV, torch.cuda.current_device()), DT_OF[mode])
    sd = net.state_dict()
    bn = {}
    for name in T.bn_names():
        got = tuple(g.double().cpu() for g in P["bn"][name])
        for g, r, b in zip(got, T.fold64(sd, name), T.fold_bar(sd, name)):
            assert bool(((g - r).abs() <= b).all()), name
        bn[name] = got
    return bn


class Recorder:
    def __init__(self, monkeypatch, eng):
        from wseg_amd import _lib as L, engine as E
        self.eng, self.convs, self.dgrads, self.wgrads, self.stems, self.pairs = eng, {}, {}, {}, [], []
        self.splits = {}                                      # flat-gradient offset of a dw -> atomics per element, summed over its launches
        conv0, dgrad0, wgrad0, stem0, wg0, ig0 = E._Pass.conv, E._Pass.dgrad, E._Pass.wgrad, L.stem_conv_kc, L.conv_wgrad, L.conv_igemm
        rec = self

        def conv(ps, c, inp, out, out2=None, **kw):
            assert c.name not in rec.convs, c.name
            rec.convs[c.name] = (inp, out, out2)
            return conv0(ps, c, inp, out, out2, **kw)

        def dgrad(ps, c, dy, out, pair=None, **kw):
            assert c.name not in rec.dgrads, c.name
            rec.dgrads[c.name] = (dy, out)
            if pair is not None:                              # a weight gradient of the same dY, in this launch or behind it
                rec.wgrads[pair[0].name] = (pair[1], pair[2])
            return dgrad0(ps, c, dy, out, pair=pair, **kw)

        def wgrad(ps, c, x, dy, **kw):
            rec.wgrads[c.name] = (x, dy)
            return wgrad0(ps, c, x, dy, **kw)

        def stem(x, w_kc, scale, shift, raw, act, *a):
            rec.stems.append((x, act))
            return stem0(x, w_kc, scale, shift, raw, act, *a)

        def conv_wgrad(x, dy, dw, **kw):
            rec._split(dw, L.wgrad_plan(x, dy, dw, **kw))
            return wg0(x, dy, dw, **kw)

        def conv_igemm(inp, w, out=None, out2=None, *, pair_wgrad=None, **kw):
            if pair_wgrad is not None:
                fused, dg, wg = L.conv_pair_plan(pair_wgrad[3], inp, w, out, out2, **kw)
                rec.pairs.append((fused, dg, wg))
                rec._split(pair_wgrad[2], wg)
            return ig0(inp, w, out, out2, pair_wgrad=pair_wgrad, **kw)

        monkeypatch.setattr(E._Pass, "conv", conv)
        monkeypatch.setattr(E._Pass, "dgrad", dgrad)
        monkeypatch.setattr(E._Pass, "wgrad", wgrad)
        monkeypatch.setattr(L, "stem_conv_kc", stem)
        monkeypatch.setattr(L, "conv_wgrad", conv_wgrad)
        monkeypatch.setattr(L, "conv_igemm", conv_igemm)

    def _split(self, dw, plan):
        assert dw.untyped_storage().data_ptr() == self.eng.flat_g.untyped_storage().data_ptr()
        self.splits[dw.storage_offset()] = self.splits.get(dw.storage_offset(), 0) + plan.nsplit

    # ---- roles
    def forward_record(self, xs):
        """{"stem": .., block: {t, x, v | v1, v2, rpost, x_out, t_out, dims}} of device tensors, by the convs' names"""
        N = xs[0].shape[0]
        dims = [tuple(x.shape[2:]) for x in xs]
        t0 = self.convs["b2.conv_branch2a"][0]
        assert len(self.stems) == len(xs) and all(a.untyped_storage().data_ptr() == t0.untyped_storage().data_ptr() for _x, a in self.stems)
        assert all(sx is x for (sx, _a), x in zip(self.stems, xs))
        rec = {"stem": dict(x=[x.double().cpu() for x in xs], t_out=t0, dims=dims)}
        t_prev, x_prev = t0, None
        for b in arch.BLOCKS:
            name, kind = b[0], b[1]
            assert T.block_dims(name, dims) == arch.block_out_dims(b, dims)
            c = {k.split(".")[1]: v for k, v in self.convs.items() if k.split(".")[0] == name}
            r = dict(t=c["conv_branch2a"][0], dims=dims)
            assert r["t"] is t_prev, name                     # a block reads the t_out of the block before it
            if kind == "res":
                r["v"] = c["conv_branch2a"][2]
                last = c.get("conv_branch2b1") or c["skip_fused"]
            else:
                r["v1"], r["v2"] = c["conv_branch2a"][2], c["conv_branch2b1"][2]
                last = c.get("conv_branch2b2") or c["skip_fused"]
            if "conv_branch1" in c:
                r["rpost"] = c["conv_branch1"][1]
            if arch.block_same_shape(b):
                assert x_prev is not None, name
                r["x"] = x_prev
            if last[1] is not None:
                r["x_out"] = last[1]
            r["t_out"] = last[2]
            assert set(c) <= {"conv_branch2a", "conv_branch2b1", "conv_branch2b2", "conv_branch1", "skip_fused"} and ("skip_fused" in c) != (
                ("conv_branch1" in c) or arch.block_same_shape(b)), (name, sorted(c))
            rec[name] = r
            t_prev, x_prev, dims = r["t_out"], r.get("x_out"), T.block_dims(name, dims)
        assert rows_of(N, dims) == t_prev.shape[0]
        return rec

    def backward_record(self, rec, S, D, taps):
        """adds D, tap, du | du2, du1, tmp, D_in and the weight gradients (read from the flat gradient buffer) to the trainable blocks' records;
        returns the splits {block: {stage: n}}"""
        eng, splits = self.eng, {}
        frozen = eng.net.FROZEN_BLOCKS
        first = arch.BLOCKS[len(frozen)][0]                   # the first trainable block: weight gradients only
        for b in reversed(arch.BLOCKS):
            name, kind = b[0], b[1]
            if name in frozen:
                assert not any(k.split(".")[0] == name for k in self.dgrads)
                continue
            r = rec[name]
            g = {k.split(".")[1]: v for k, v in self.dgrads.items() if k.split(".")[0] == name}
            sv = S[name]
            assert sv["t"] is r["t"] and all(sv[k] is r[k] for k in ("v", "v1", "v2") if k in sv)      # the decisions are the stored activations
            if kind == "res":
                r["D"], r["du"] = g["conv_branch2b1"]
            else:
                r["D"], r["du2"] = g["conv_branch2b2"]
                assert g["conv_branch2b1"][0] is r["du2"]
                r["du1"] = g["conv_branch2b1"][1]
            assert r["D"] is D, name                           # the D of a block is the D_in of the block behind it
            if name in taps:
                r["tap"] = taps[name]
            if "conv_branch1" in g:
                r["tmp"] = g["conv_branch1"][1]
            last = g.get("skip_fused") or g.get("conv_branch2a")
            if name == first:
                assert last is None and "tmp" not in r
            else:
                r["D_in"] = D = last[1]
            splits[name] = {}
            dua = r["du"] if kind == "res" else r["du1"]
            want = {"2a": (r["t"], dua), "2b1": (r["v"], r["D"]) if kind == "res" else (r["v1"], r["du2"]), "1": (r["t"], r["D"])}
            if kind != "res":
                want["2b2"] = (r["v2"], r["D"])
            for (cname, ci, co, k, _s, _d) in arch.block_convs(b):
                st = "dW_" + cname.split(".conv_branch")[1]
                assert all(a is w_ for a, w_ in zip(self.wgrads[cname], want[st[3:]])), cname      # dW = x^T dY of the definition's x and dY
                r[st] = eng.grad_slice(cname).view(co, k, k, ci).permute(0, 3, 1, 2)
                splits[name][st] = self.splits[eng.offsets[cname][0]]
        return splits


def rows_of(N, dims):
    return sum(N * h * w for h, w in dims)


def _cpu(rec):
    return {blk: {k: (v.double().cpu() if torch.is_tensor(v) else v) for k, v in r.items()} for blk, r in rec.items()}


def _check_masks(S, sites):
    masks = {}
    for key, c, p in S_SPECS[:sites]:
        m = S["masks"][key].double().cpu()
        keep = 1.0 / (1.0 - p)
        kept = (m - keep).abs() <= 2 * U32 * keep               # (the f32 value of 1 / (1 - p))
        assert m.shape[1] == c and bool(((m == 0) | kept).all()) and bool(kept.any()) and bool((m == 0).any()), key
        masks[key] = m
    if sites == 4:
        assert S["masks"]["dropout7"] is None
    return masks


S_SPECS = (("b6.dropout_2b1", 512, 0.3), ("b6.dropout_2b2", 1024, 0.3), ("b7.dropout_2b1", 1024, 0.5), ("b7.dropout_2b2", 2048, 0.5),
           ("dropout7", 4096, 0.5))         # network/resnet38d.py:64,68 and resnet38_contrast.py:14
assert all(T.DROP_P[k] == p for k, _c, p in S_SPECS)


def _report(tag, mode, table, seconds):
    for kind, (ratio, where) in sorted(T.worst(table).items()):
        print(f"[{tag} {mode}] worst {kind:8s} err / bar {ratio:.4f} at {where}")
    print(f"[{tag} {mode}] {len(table)} stored tensors judged, float64 reference {seconds:.1f} s")
    bad = [row for row in table if not row[3]]
    assert not bad, bad


def _structure(mode, names):
    """bf16: b5, b6, b7 as one two-source launch, b3 and b4 not; the other modes: none"""
    fused = {n.split(".")[0] for n in names if n.endswith(".skip_fused")}
    assert fused == ({"b5", "b6", "b7"} if mode == "bf16" else set()), (mode, fused)


def _run(kind, mode, monkeypatch, views, N, train, backward):
    """one case: the forward (and backward) under the recorder; returns what the judges need"""
    net = _net(kind, mode)
    net.train() if train else net.eval()
    dev = torch.device(DEV, torch.cuda.current_device())
    eng = net._engine.active(dev)
    eng.injected_masks = None
    torch.manual_seed(20 + MODES.index(mode))                  # the dropout tables are drawn on the device: the same ones in every run
    W, bn = _weights(kind, eng, mode), _folds(net, eng, mode)
    xs = [synth.synthetic_images(N, hw, 7 + i).cuda() for i, hw in enumerate(views)]
    rec = Recorder(monkeypatch, eng)
    with torch.no_grad():
        if kind != "contrast":
            _st, _ps, S = eng.run_backbone(xs, save=True)
        else:
            _st, _ps, S = eng._run_trunk(xs, train, eng.MASK_SPECS if train else None, keep_frozen=train)
    record = rec.forward_record(xs)
    _structure(mode, rec.convs)
    masks = _check_masks(S, 5 if kind == "contrast" else 4) if train else None
    if not train:
        assert S["masks"] is None
    splits = None
    if backward:
        M = S["M"]
        mk = lambda c, seed: (torch.rand(M, c, generator=_gen(seed)) * 2 - 1).bfloat16().to(TDT[mode]).cuda()      # bf16 values: one functional in all modes
        D, taps = mk(4096, 90), {"b5": mk(512, 91), "b6": mk(1024, 92)}
        eng.attach_grads()
        eng.flat_g.zero_()
        with torch.no_grad():
            eng.run_trunk_backward(S, D, taps)
        splits = rec.backward_record(record, S, D, taps)
        _structure(mode, rec.dgrads)
        for fused, dg, wg in rec.pairs:
            print(f"[{kind} {mode}] paired data gradient: fused {fused}, {dg}, weight gradient {wg}")
        assert (len(rec.pairs) > 0) == (mode == "bf16")
        for n in _trunk_conv_names():                           # the frozen prefix gets no gradient, nor does any BatchNorm
            frozen = n == "conv1a" or n.split(".")[0] in net.FROZEN_BLOCKS
            assert (n in eng.offsets) != frozen and (eng.conv_param(n).grad is None) == frozen, n
        for n in T.bn_names():
            bnm = eng.bn_module(n)
            assert bnm.weight.grad is None and bnm.bias.grad is None, n
    torch.cuda.synchronize()
    return _cpu(record), W, bn, masks, splits, net.FROZEN_BLOCKS


def _judge(tag, mode, data, N, forward, backward):
    record, W, bn, masks, splits, frozen = data
    t0 = time.perf_counter()
    table = T.judge(mode, record, W, bn, masks, N, splits=splits, forward=forward, backward=backward, frozen=frozen)
    _report(tag, mode, table, time.perf_counter() - t0)
    return table


@pytest.mark.parametrize("mode", MODES)
def test_contrast_trunk_forward(monkeypatch, mode):
    """training mode, two views, N = 2, the five dropout tables drawn on the device, the frozen blocks kept: the stem and all 17 blocks"""
    data = _run("contrast", mode, monkeypatch, VIEWS, 2, True, False)
    dims = list(VIEWS)
    for b in arch.BLOCKS:
        dims = arch.block_out_dims(b, dims)
        if b[0] == "b3":
            assert dims == [(25, 19), (11, 7)]
    assert dims == [(13, 10), (6, 4)]
    table = _judge("contrast forward", mode, data, 2, True, False)
    tags = {row[0] for row in table}
    assert "stem.t_out" in tags and all(f"{b[0]}.t_out" in tags for b in arch.BLOCKS)


@pytest.mark.parametrize("mode", MODES)
def test_contrast_trunk_backward(monkeypatch, mode):
    """run_trunk_backward on the same kind of context: random D, taps on b5 and b6; every stage of b7 down to b3 and all 35 weight gradients"""
    data = _run("contrast", mode, monkeypatch, VIEWS, 2, True, True)
    table = _judge("contrast backward", mode, data, 2, False, True)
    tags = [row[0] for row in table]
    assert sum(".dW_" in t_ for t_ in tags) == 35 and "b3_1.D_in" in tags and "b3.D_in" not in tags and "b3.du" in tags


@pytest.mark.parametrize("mode", MODES)
def test_aff_backbone(monkeypatch, mode):
    """the AffinityNet backbone (run_backbone(save=True): four dropout sites, dropout7 None), forward and run_trunk_backward with taps, one view"""
    data = _run("aff", mode, monkeypatch, (ONE_VIEW,), 2, True, True)
    table = _judge("aff backbone", mode, data, 2, True, True)
    assert sum(".dW_" in row[0] for row in table) == 35


@pytest.mark.parametrize("mode", MODES)
def test_aff_backbone_longer_prefix(monkeypatch, mode):
    """the same pass with another prefix, read from the net: b3 frozen too.  b3_1, a same-shape block, is then the first trainable one: weight
    gradients only (its 256 -> 256 3x3 conv_branch2a's on its own launch), no D_in, and nothing of b3 runs backward or has a gradient slot
    (_run asserts the offsets and the .grad of every conv against the net's FROZEN_BLOCKS)."""
    data = _run("aff_b3", mode, monkeypatch, (ONE_VIEW,), 2, True, True)
    assert data[5] == ("b2", "b2_1", "b2_2", "b3")
    table = _judge("aff backbone, b3 frozen", mode, data, 2, True, True)
    tags = {row[0] for row in table}
    assert sum(".dW_" in t_ for t_ in tags) == 32              # 35 less b3's three
    assert {"b3_1.du", "b3_1.dW_2a", "b3_1.dW_2b1", "b3_2.D_in"} <= tags and "b3_1.D_in" not in tags
    assert not any(t_.split(".")[0] == "b3" and t_.split(".")[1] in T.BWD_STAGES for t_ in tags)


@pytest.mark.parametrize("mode", MODES)
def test_eval_forward(monkeypatch, mode):
    """inference allocation path: one view, N = 1, nothing saved, no masks; x_out exists only in front of a same-shape block"""
    data = _run("contrast", mode, monkeypatch, (ONE_VIEW,), 1, False, False)
    record = data[0]
    for i, b in enumerate(arch.BLOCKS):
        nxt_same = i + 1 < len(arch.BLOCKS) and arch.block_same_shape(arch.BLOCKS[i + 1])
        assert ("x_out" in record[b[0]]) == nxt_same, b[0]
    _judge("eval forward", mode, data, 1, True, False)
