"""The launch sequence of the engine's paths, pinned: every launching call of wseg_amd._lib in call order, with its scalars, its
tensor operands (dtype and element offset within the storage: a wrong column slice such as feat.view(-1)[64:] shows) and the role of
the stream it is enqueued on, compared as a whole list against tests/golden/engine_launches_<case>.json.  A host-side refactor of
engine.py must leave every one of them as it is: the fixtures are written once, at the commit BEFORE such a change,
  python tests/test_gpu_engine_launches.py --write [case ...]
and are not regenerated after it.  The committed ones: contrast_step, net_autograd, aff_train, contrast_infer, aff_infer at ae4165a, before
the trunk / heads split of the engine; seg_infer and seg_head_train (the DeepLab head, which those predate) at 4989fae, with this file's
cases run on that commit's wseg_amd/, before the frozen prefix moved into the net classes and the head passes were shared.
Shapes: the smallest that still take every branch of both block loops (same and non-same ResBlocks,
fused and unfused skip, bottleneck blocks, taps on b5 and b6, two row segments of odd, unequal stride-8 maps 13x9 and 5x7)."""
import inspect
import json
import os
import random
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu

NOT_LAUNCHES = {"check", "conv_plan", "wgrad_plan", "conv_pair_plan", "debug_stamps", "debug_set_diag"}      # go through check() but enqueue nothing


def launching_functions(L):
    """the public callables of wseg_amd._lib that launch: every function that goes through _call / check"""
    out = []
    for name, fn in sorted(vars(L).items()):
        if name.startswith("_") or name in NOT_LAUNCHES or not inspect.isfunction(fn) or fn.__module__ != L.__name__:
            continue
        src = inspect.getsource(fn)
        if "_call(" in src or "check(" in src:
            out.append(name)
    return out


def _enc(v):
    if isinstance(v, torch.Tensor):
        return ["T", str(v.dtype).replace("torch.", ""), int(v.storage_offset())]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (list, tuple)):
        return [_enc(x) for x in v]
    if isinstance(v, dict):
        return {str(k): _enc(x) for k, x in v.items() if x is not None}
    if hasattr(v, "item"):
        return v.item()
    return "<" + type(v).__name__ + ">"


class Recorder:
    """Wraps the launching functions (monkeypatch: undone at the end of the test) and lists their calls.  Keywords left at their default,
    and keywords of a ** catch-all that are None, are not written."""

    def __init__(self, monkeypatch, engines):
        from wseg_amd import _lib as L
        self.calls, self.engines = [], engines
        self.main = torch.cuda.current_stream()
        for name in launching_functions(L):
            monkeypatch.setattr(L, name, self._wrap(name, getattr(L, name)))

    def _role(self):
        cur = torch.cuda.current_stream()
        if cur == self.main:
            return "main"
        for eng in self.engines:
            for role, st in eng._streams.items():
                if st == cur:
                    return role
        return "late"

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)

        def wrapper(*args, **kw):
            ba = sig.bind(*args, **kw)
            rec = {"f": name, "stream": self._role()}
            for pname, val in ba.arguments.items():
                par = sig.parameters[pname]
                if par.kind == par.VAR_KEYWORD:
                    rec.update({k: _enc(v) for k, v in val.items() if v is not None})
                elif par.default is par.empty or isinstance(val, torch.Tensor) or val != par.default:
                    rec[pname] = _enc(val)
            self.calls.append(rec)
            return fn(*args, **kw)
        return wrapper


# ---------------------------------------------------------------------------------------------------------------- the cases
VIEWS = ((104, 72), (40, 56))


def _contrast_net(prec, train):
    from wseg_amd import synth
    from wseg_amd.resnet38_contrast import Net
    m = Net(precision=prec)
    m.load_state_dict(synth.procedural_state_dict(0))
    m.cuda()
    return m.train() if train else m.eval()


def _aff_net(prec, train):
    from wseg_amd import synth
    from wseg_amd.resnet38_aff import Net
    m = Net(precision=prec)
    m.load_state_dict(synth.procedural_aff_state_dict(0))
    m.cuda()
    return m.train() if train else m.eval()


def contrast_step(rec_of, prec):
    """(a) the fused contrast training step, N = 2, two views"""
    from wseg_amd import loss_hip, synth
    n, seed = 2, 7
    m = _contrast_net(prec, True)
    m.set_dropout_masks([synth.synthetic_dropout_masks(n, seed * 2), synth.synthetic_dropout_masks(n, seed * 2 + 1)])
    a, b = (synth.synthetic_images(n, hw, seed + j).cuda() for j, hw in enumerate(VIEWS))
    loss_hip._WVEC.clear()                             # (a per-process cache: its first use per map size launches)
    rec = rec_of(m._engine)
    loss_hip.step(m, a, b, synth.synthetic_labels(n, seed).cuda(), 0.20, random.Random(3), True, loss_hip.cpu_tie_pattern(n * 256, 32), zero_grads=True)
    return rec


def net_autograd(rec_of, prec):
    """(b) Net.forward at full resolution and its autograd backward (_NetFunction), one view"""
    from wseg_amd import synth
    m = _contrast_net(prec, True)
    m.set_dropout_masks([synth.synthetic_dropout_masks(1, 5)])
    x = synth.synthetic_images(1, 64, 9).cuda()
    rec = rec_of(m._engine)
    cam, cam_rv, f_proj, _rvd = m(x)
    (cam.sum() + cam_rv.sum() + f_proj.sum()).backward()
    return rec


def aff_train(rec_of, prec):
    """(c) AffinityNet train_forward + train_backward, N = 2"""
    from tests import aff_train_ref as A
    from wseg_amd import synth
    m = _aff_net(prec, True)
    m.set_dropout_masks([A.aff_masks(2, 19)])
    x = synth.synthetic_images(2, 64, 17).cuda()
    rec = rec_of(m._engine)
    f9, _geo, saved = m.train_forward(x)
    g = torch.Generator().manual_seed(23)
    m.train_backward(saved, (torch.rand(f9.shape, generator=g) * 2 - 1).cuda())
    return rec


def contrast_infer(rec_of, prec):
    """(d) the inference forward over two batched views, nothing saved"""
    from wseg_amd import synth
    m = _contrast_net(prec, False)
    a, b = (synth.synthetic_images(1, hw, 11 + j).cuda() for j, hw in enumerate(VIEWS))
    eng = m._engine.active(a.device)
    rec = rec_of(eng)
    with torch.no_grad():
        eng.run_forward([a, b], save=False)
    return rec


def aff_infer(rec_of, prec):
    """(d) Net.affinities"""
    from wseg_amd import synth
    m = _aff_net(prec, False)
    x = synth.synthetic_images(1, 64, 13).cuda()
    rec = rec_of(m._engine)
    m.affinities(x)
    return rec


def _seg_net(prec, train):
    from wseg_amd import synth
    from wseg_amd.deeplabv1_resnet38 import Net
    m = Net(precision=prec)
    m.load_state_dict(synth.procedural_seg_state_dict(0))
    m.cuda()
    return m.train() if train else m.eval()


def seg_infer(rec_of, prec):
    """(e) DeepLab Net.coarse_logits: the backbone and the eval head, one image"""
    from wseg_amd import synth
    m = _seg_net(prec, False)
    x = synth.synthetic_images(1, 64, 29).cuda()
    rec = rec_of(m._engine)
    m.coarse_logits(x)
    return rec


def seg_head_train(rec_of, prec):
    """(f) the DeepLab head's training forward and its backward with the bn7-ReLU operands, N = 2 on an 8 x 8 map"""
    from wseg_amd import seg_head, synth
    from wseg_amd.engine import DT_OF
    from wseg_amd import _lib as L
    N, h, w = 2, 8, 8
    m = _seg_net(prec, True)
    g = torch.Generator().manual_seed(31)
    tdt = L.TORCH_DTYPE[DT_OF[prec]]
    t = torch.relu(torch.randn(N * h * w, 4096, generator=g)).to(tdt).cuda()
    d_rows = torch.zeros(N * h * w, 24)
    d_rows[:, :21] = torch.rand(N * h * w, 21, generator=g) * 2 - 1
    scale = (torch.rand(4096, generator=g) + 0.5).cuda()
    rec = rec_of(m._engine)
    _rows, ctx = seg_head.seg_head_forward(m, t, N, h, w, synth.dropout_key(3, h))
    seg_head.seg_head_backward(ctx, d_rows.cuda(), scale=scale, mask=t)
    return rec


CASES = [("contrast_step", contrast_step, "bf16"), ("contrast_step", contrast_step, "bf16x3"), ("net_autograd", net_autograd, "fp32"),
         ("aff_train", aff_train, "bf16"), ("aff_train", aff_train, "fp32"), ("contrast_infer", contrast_infer, "bf16"),
         ("aff_infer", aff_infer, "bf16"), ("seg_infer", seg_infer, "bf16"), ("seg_head_train", seg_head_train, "fp32"),
         ("seg_head_train", seg_head_train, "bf16")]


def _path(name, prec):
    return os.path.join(GOLDEN, f"engine_launches_{name}_{prec}.json")


def _run(case, prec, monkeypatch):
    rec = case(lambda eng: Recorder(monkeypatch, [eng]), prec)
    torch.cuda.synchronize()
    return json.loads(json.dumps(rec.calls))           # (as the fixture holds them: tuples are lists)


@pytest.mark.parametrize("name,case,prec", CASES, ids=[f"{n}-{p}" for n, _c, p in CASES])
def test_launch_sequence_is_the_pinned_one(monkeypatch, name, case, prec):
    want = json.load(open(_path(name, prec)))
    got = _run(case, prec, monkeypatch)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"launch {i} of {len(want)} differs:\n  got    {g}\n  pinned {w}"
    assert len(got) == len(want), f"{len(got)} launches, pinned {len(want)}; first extra: {(got + want)[min(len(got), len(want))]}"
    assert got == want


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--write"], "usage: python tests/test_gpu_engine_launches.py --write [case ...]   (at the commit BEFORE an engine change)"
    only = sys.argv[2:]                                # new cases alone: the fixtures of the others stay as they were written
    assert set(only) <= {n for n, _c, _p in CASES}, only
    for name, case, prec in CASES:
        if only and name not in only:
            continue
        with pytest.MonkeyPatch.context() as mp:
            calls = _run(case, prec, mp)
        with open(_path(name, prec), "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in calls) + "\n]\n")
        print(f"{name} [{prec}]: {len(calls)} launches -> {os.path.relpath(_path(name, prec), ROOT)}")
