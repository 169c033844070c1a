"""The DeepLab training loss's yardstick judged on the CPU, as tests/test_conv_bars_host.py judges the convolution bars: the float64
restatement (tests/seg_loss_f64.py) equals torch's own float64 F.interpolate + F.cross_entropy + autograd on every shape the GPU test runs;
the same chain evaluated in float32 lies inside the derived f32 bars on every shape; and each constructed wrong variant — evaluated in
float64, so that nothing but the defect separates it from the restatement — falls outside them.  A bar loosened later fails here before it
reaches a kernel.  The sweeps include the shape past 256 forward workgroups and the class counts 9, 16, 25, 32 of the GPU test; a loss whose
sums stop after the first 256 partials is one of the wrong variants.  Also what needs no device: the entry points exist, refuse bad arguments before any device call, and refuse CPU tensors."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import seg_loss_f64 as S
from wseg_amd import _lib as L

HOST_SHAPES = S.SHAPES + [((2, 3), (11, 13), 2)]             # a batch of two with unequal valid counts: where a per-image count shows
N_CLS = (21, 2)
# the GPU sweep's cases (the shape past 256 partials at 21 classes only), the host's own batch of two, and the class counts of two and four chunks
HOST_CASES = S.CLASS_CASES + [(HOST_SHAPES[-1], n) for n in N_CLS] + [(s, n) for s in S.NC8_SHAPES for n in S.NC8_COUNTS]
HOST_SWEEP = [pytest.param(s, n, id=f"{S.shape_id(s)}-{n}") for s, n in HOST_CASES]


def _torch_chain(coarse, label, dtype, align=True):
    """(loss, lse, grad) of the reference's two lines in `dtype` on the CPU"""
    x = coarse.detach().clone().to(dtype).requires_grad_()
    z = F.interpolate(x, label.shape[1:], mode="bilinear", align_corners=align)
    lab = label.long()
    lab = torch.where(lab >= coarse.shape[1], torch.full_like(lab, S.IGNORE), lab)
    loss = F.cross_entropy(z, lab, ignore_index=S.IGNORE)
    loss.backward()
    return dict(loss=loss.detach(), lse=torch.logsumexp(z.detach(), 1), grad=x.grad)


@pytest.mark.parametrize("shape,n_cls", HOST_SWEEP)
def test_restatement_equals_torch_float64(shape, n_cls):
    coarse, label = S.make_case(shape, n_cls, torch.float32, 11)
    ref, t = S.restate(coarse, label), _torch_chain(coarse, label, torch.float64)
    tol = 1e-12 * max(1.0, float(coarse.abs().max()))
    assert S.within(t["loss"], ref["loss"], tol) and S.within(t["lse"], ref["lse"], tol) and S.within(t["grad"], ref["grad"], tol)
    assert int(ref["count"]) == int((label < n_cls).sum()) and int(ref["oor"]) == 0


@pytest.mark.parametrize("n_cls", N_CLS)
def test_all_ignored_batch_is_torchs_answer(n_cls):
    coarse, label = S.make_case(((5, 7), (33, 47), 1), n_cls, torch.float32, 12)
    label[:] = S.IGNORE
    ref, t = S.restate(coarse, label), _torch_chain(coarse, label, torch.float64)
    assert S.nan_equal(t["loss"], ref["loss"]) and S.within(t["loss"], ref["loss"], 0.0)
    assert S.within(t["grad"], ref["grad"], 0.0) and int(ref["count"]) == 0


@pytest.mark.parametrize("shape,n_cls", HOST_SWEEP)
def test_float32_chain_passes_the_bars(shape, n_cls):
    for dtype in (torch.float32, torch.bfloat16):                 # bf16: the VALUES are bf16-representable, the arithmetic stays f32
        coarse, label = S.make_case(shape, n_cls, dtype, 13)
        ref = S.restate(coarse, label)
        verdict = S.judge(_torch_chain(coarse, label, torch.float32), ref, coarse)
        print(S.shape_id(shape), n_cls, dtype, {k: f"{r:.3f}" for k, (_ok, r) in verdict.items()})
        assert all(ok for ok, _r in verdict.values()), verdict


# ---------------------------------------------------------------------------------------------- constructed wrong variants, in float64
def _drop_last_i1(Wm):
    """the i1 tap of the last input position dropped (a bounds guard one too strict): only the output position that lands on it exactly keeps it"""
    Wm = Wm.clone()
    if Wm.shape[1] > 1:
        last = Wm[:, -1]
        Wm[:, -1] = torch.where(last < 1.0, torch.zeros_like(last), last)
    return Wm


def _variant(name, coarse, label):
    N, C, fh, fw = coarse.shape
    H, W = label.shape[1:]
    if name == "align_corners_false":
        return _torch_chain(coarse, label, torch.float64, align=False)
    x = coarse.double().requires_grad_()
    Wy, Wx = S.axis_matrix(fh, H), S.axis_matrix(fw, W)
    if name == "i1_dropped_at_the_end":
        Wy, Wx = _drop_last_i1(Wy), _drop_last_i1(Wx)
    z = torch.einsum("yi,ncij,xj->ncyx", Wy, x, Wx)
    if name == "bf16_logits":
        z = z + (z.detach().bfloat16().double() - z.detach())      # rounded before the softmax, the gradient passed straight through
    lab = label.long()
    valid = lab < C
    lse = torch.logsumexp(z, 1)
    nll = lse - z.gather(1, lab.clamp(max=C - 1)[:, None])[:, 0]
    vsum = lambda v: torch.where(valid, v, torch.zeros_like(v)).sum()
    if name == "mean_over_all_pixels":
        loss = vsum(nll) / valid.numel()
    elif name == "count_per_image":
        per = torch.where(valid, nll, torch.zeros_like(nll)).sum((1, 2)) / valid.sum((1, 2))
        loss = per.mean()
    else:
        loss = vsum(nll) / valid.sum()
    (nll.sum() / valid.sum() if name == "ignored_pixels_get_gradient" else loss).backward()
    return dict(loss=loss.detach(), lse=lse.detach(), grad=x.grad)


def _applies(name, shape):
    (fh, fw), (H, W), N = shape
    if name == "align_corners_false":
        return (fh > 1 and H > 1) or (fw > 1 and W > 1)            # a size of 1 on both axes' input or output side: the two modes coincide
    if name == "i1_dropped_at_the_end":                             # some output position reads the last input position as a fractional i1 tap
        return any(not torch.equal(_drop_last_i1(m), m) for m in (S.axis_matrix(fh, H), S.axis_matrix(fw, W)))
    if name == "count_per_image":
        return N > 1
    return True


def test_a_loss_that_stops_after_256_partials_fails_the_bar():
    """the finish kernel adds partial t, then t + 256: a loss whose sums end with the first 256 partials — the first 65536 label pixels — is what
    a dropped second trip gives.  Evaluated in float64: nothing but the defect separates it from the restatement."""
    shape = S.PAST_256_PARTIALS
    assert S.forward_workgroups(shape) > 256
    coarse, label = S.make_case(shape, 21, torch.float32, 14)
    ref = S.restate(coarse, label)
    z = torch.einsum("yi,ncij,xj->ncyx", ref["Wy"], coarse.double(), ref["Wx"])
    lab = label.long()
    nll = (torch.logsumexp(z, 1) - z.gather(1, lab.clamp(max=20)[:, None])[:, 0]).reshape(-1)
    valid = ref["valid"].reshape(-1)
    whole = torch.where(valid, nll, torch.zeros_like(nll))
    assert S.within(whole.sum() / valid.sum(), ref["loss"], S.loss_bar(ref, coarse))                       # nothing planted: the restatement
    assert bool(valid[65536:].any())
    cut = whole[:65536].sum()
    for name, loss in (("sum and count cut", cut / valid[:65536].sum()), ("sum cut", cut / valid.sum())):
        err = abs(float(loss - ref["loss"]))
        print(f"{name}: |loss - ref| {err:.3e}, bar {S.loss_bar(ref, coarse):.3e}")
        assert not S.within(loss, ref["loss"], S.loss_bar(ref, coarse)), name
    assert not S.within(cut, ref["nll_sum"], S.nll_sum_bar(ref, coarse))
    assert float(valid[:65536].sum()) != float(ref["count"])                                              # (the counts are asserted as equalities)


VARIANTS = ["align_corners_false", "mean_over_all_pixels", "ignored_pixels_get_gradient", "i1_dropped_at_the_end", "bf16_logits", "count_per_image"]


@pytest.mark.parametrize("name", VARIANTS)
def test_wrong_variants_fail_the_bars(name):
    judged = 0
    for shape in HOST_SHAPES:
        if not _applies(name, shape):
            continue
        coarse, label = S.make_case(shape, 21, torch.float32, 14)
        ref = S.restate(coarse, label)
        honest = S.judge(_variant("none", coarse, label), ref, coarse)
        assert all(ok for ok, _r in honest.values()), (shape, honest)     # the variant machinery itself is the restatement when nothing is planted
        verdict = S.judge(_variant(name, coarse, label), ref, coarse)
        print(name, S.shape_id(shape), {k: f"{r:.3g}" for k, (_ok, r) in verdict.items()})
        assert not all(ok for ok, _r in verdict.values()), (name, shape, verdict)
        judged += 1
    assert judged >= 1


# ---------------------------------------------------------------------------------------------- what needs no device
def test_device_entry_points_refuse_the_cpu():
    from wseg_amd.seg_loss import seg_ce_rows, seg_cross_entropy
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg_cross_entropy(torch.zeros(1, 21, 5, 7), torch.zeros(1, 33, 47, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg_ce_rows(torch.zeros(35, 24), 24, torch.zeros(1, 33, 47, dtype=torch.uint8), 1, 5, 7, 33, 47)


GOOD = dict(ld=24, dtype=L.F32, N=2, fh=5, fw=7, H=33, W=47, n_cls=21, ld_d=24, d_dtype=L.F32)
REJECTS = [
    (dict(ld=16, ld_d=16), "must be a multiple of 8 and >= 24"),
    (dict(ld=28, ld_d=28), "must be a multiple of 8 and >= 24"),
    (dict(n_cls=33), "n_cls=33 outside [2, 32]"),
    (dict(n_cls=1), "n_cls=1 outside [2, 32]"),
    (dict(dtype=L.F32X3), "dtype 2 (f32 or bf16)"),
    (dict(H=0), "bad dims"),
    (dict(fw=0), "bad dims"),
    (dict(N=64, H=8192, W=8192), "below 2^31"),
]


def _forward(kw, rows=L._ANY):
    ptr = C.c_void_p(L._ANY)                                   # stand-in addresses nobody dereferences: every call below is refused first
    return L.lib.wseg_seg_ce_forward(C.c_void_p(rows), kw["ld"], kw["dtype"], ptr, ptr, ptr, ptr, kw["N"], kw["fh"], kw["fw"], kw["H"], kw["W"],
                                     kw["n_cls"], None)


def _backward(kw, rows=L._ANY, d_rows=L._ANY):
    ptr = C.c_void_p(L._ANY)
    return L.lib.wseg_seg_ce_backward(C.c_void_p(rows), kw["ld"], kw["dtype"], ptr, ptr, ptr, None, C.c_void_p(d_rows), kw["ld_d"], kw["d_dtype"],
                                      kw["N"], kw["fh"], kw["fw"], kw["H"], kw["W"], kw["n_cls"], None)


def test_entry_points_exist_and_reject_bad_arguments():
    for fn in ("wseg_seg_ce_workspace_bytes", "wseg_seg_ce_forward", "wseg_seg_ce_backward"):
        assert hasattr(L.lib, fn), fn
    assert L.seg_ce_workspace_bytes(1, 57, 301) == -(-57 * 301 // 256) * 12      # [blocks][3] f32, one block of 256 label pixels
    assert L.seg_ce_workspace_bytes(10, 448, 448) == 10 * 448 * 448 // 256 * 12
    assert L.seg_ce_workspace_bytes(64, 8192, 8192) == -1 and L.seg_ce_workspace_bytes(0, 8, 8) == -1
    err = lambda: L.lib.wseg_last_error().decode()
    for change, text in REJECTS:
        kw = {**GOOD, **change}
        for call in (_forward, _backward):
            assert call(kw) == -1, (change, call.__name__)
            assert text in err(), (change, err())
    assert _forward(GOOD, rows=L._ANY + 8) == -1 and "not 16-byte aligned" in err()
    assert _backward(GOOD, d_rows=L._ANY + 8) == -1 and "d_rows null or not 16-byte aligned" in err()
    assert _backward({**GOOD, "ld_d": 28}) == -1 and "ld_d=28" in err()
    assert _backward({**GOOD, "d_dtype": L.F32X3}) == -1 and "d_dtype 2" in err()
    null = C.c_void_p(None)
    assert L.lib.wseg_seg_ce_forward(C.c_void_p(L._ANY), 24, L.F32, null, null, null, null, 1, 5, 7, 33, 47, 21, None) == -1
    assert "null pointer" in err()


def test_training_mode_is_still_refused_and_says_what_exists():
    from wseg_amd.deeplabv1_resnet38 import Net
    net = Net(precision="fp32")
    net.train()
    with pytest.raises(RuntimeError, match="the training loss exists .*the training forward does not yet"):
        net(torch.zeros(1, 3, 40, 56))
