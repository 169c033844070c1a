"""The DeepLab training loss on the GPU (csrc/seg_loss.hip, wseg_amd/seg_loss.py) against the float64 restatement and the bars derived in
tests/seg_loss_f64.py (from the arithmetic, safety factor 2, never fitted to a run; judged on the CPU by tests/test_seg_loss_host.py).

The kernels run on the engine layout — pixel rows of ld 24 with 1e30 in the pad columns, which must never reach a result — for f32 and bf16
rows (bf16 rows are read exactly: the float64 side gets the same values), 21 and 2 classes, over every shape of seg_loss_f64.SHAPES (the
shape whose forward launch has more than 256 workgroups — the finish kernel's second trip — at 21 classes only), and for 9, 16, 25 and 32
classes (two and four 8-class chunks, the kernels' other instantiations) on rows of ld = the chunks and 8 columns wider.  The
two counts of out4 are EQUAL to the float64 counts; the loss, the per-pixel log-sum-exp and every element of the gradient lie within their
bars (a coarse cell no valid pixel touches has the bar 0: exact zeros); no pixel is excluded.  The named cases pin what no bar expresses:
torch's answer on an all-ignored batch, out-of-range labels, exact power-of-two gscale, the loss-only call, run-to-run bits, the batch
layout, the autograd wrapper's dtype / memory-format contract, and the refusals."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import seg_loss_f64 as S

pytestmark = pytest.mark.gpu

LD = 24
SENTINEL = 7.0
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def _rows(coarse, dtype, ld=LD):
    """[N, C, fh, fw] float -> pixel rows [N * fh * fw, ld] of `dtype` on the device (columns >= C hold a poison the kernels must not use)"""
    N, C, fh, fw = coarse.shape
    rows = torch.full((N * fh * fw, ld), 1e30)
    rows[:, :C] = coarse.permute(0, 2, 3, 1).reshape(-1, C)
    return rows.to(dtype).cuda()


def _grad_of(d, coarse):
    N, C, fh, fw = coarse.shape
    return d[:, :C].float().view(N, fh, fw, C).permute(0, 3, 1, 2)


def _run(coarse, label, dtype, d_dtype=torch.float32, ld_d=None, gscale=None, ld=LD):
    """(out4, lse, d_rows) on the host: forward and backward of the engine-layout entry points on rows of `ld`; d_rows starts as SENTINEL everywhere"""
    from wseg_amd.seg_loss import seg_ce_rows, seg_ce_rows_backward
    N, C, fh, fw = coarse.shape
    H, W = label.shape[1:]
    out4, ctx = seg_ce_rows(_rows(coarse, dtype, ld), ld, label.cuda(), N, fh, fw, H, W, C)
    ld_d = ld_d or (C + 7) // 8 * 8
    d = torch.full((N * fh * fw, ld_d), SENTINEL, dtype=d_dtype, device="cuda")
    seg_ce_rows_backward(ctx, None if gscale is None else torch.tensor([gscale], device="cuda"), out=d, ld_d=ld_d)
    torch.cuda.synchronize()
    return out4.cpu(), ctx["lse"].cpu(), d.cpu()


@functools.lru_cache(maxsize=None)
def _case(shape, n_cls, dt):
    """(coarse, label, the float64 restatement) of one sweep case: computed once, shared, never modified"""
    coarse, label = S.make_case(shape, n_cls, DTYPES[dt], 21)
    return coarse, label, S.restate(coarse, label)


def _check(got, ref, coarse, what, **kw):
    verdict = S.judge(got, ref, coarse, **kw)
    print(what, {k: f"err/bar {r:.3f}" for k, (_ok, r) in verdict.items()})
    assert all(ok for ok, _r in verdict.values()), (what, verdict)


def _sweep_case(shape, n_cls, dt, ld=LD):
    """one case of the sweep on rows of `ld`; returns what the f32 d_rows run gave"""
    coarse, label, ref = _case(shape, n_cls, dt)
    nc8 = (n_cls + 7) // 8 * 8
    out4, lse, d = _run(coarse, label, DTYPES[dt], ld=ld)
    assert float(out4[1]) == float(ref["count"]) and float(out4[3]) == float(ref["oor"]) == 0.0         # integer counts: equal, not close
    assert S.within(out4[2], ref["nll_sum"], S.nll_sum_bar(ref, coarse))
    _check(dict(loss=out4[0], lse=lse, grad=_grad_of(d, coarse)), ref, coarse, f"{S.shape_id(shape)} n_cls {n_cls} {dt} rows of ld {ld}, f32 d_rows")
    assert d.shape[1] == nc8 and bool((d[:, n_cls:nc8] == 0).all())                                    # the pad columns of the 8-chunk: zeros
    assert (d[:, n_cls:nc8].numel() == 0) == (n_cls % 8 == 0)                                          # (a whole chunk of classes has no pad column)
    # bf16 d_rows: the same f32 sums rounded once; ld_d = 32 (40 for four chunks): the columns past the chunks keep what they held
    ld_w = max(32, nc8 + 8)
    out4_b, _lse, d_b = _run(coarse, label, DTYPES[dt], d_dtype=torch.bfloat16, ld_d=ld_w, ld=ld)
    assert torch.equal(out4_b, out4)
    assert torch.equal(d_b[:, :nc8], d.bfloat16())                                                     # ONE rounding of the f32 result
    _check(dict(loss=out4_b[0], grad=_grad_of(d_b, coarse)), ref, coarse, "   bf16 d_rows", grad_store_bf16=True)
    assert bool((d_b[:, n_cls:nc8] == 0).all()) and bool((d_b[:, nc8:] == SENTINEL).all()) and d_b.shape[1] == ld_w > nc8
    _o, _l, d_w = _run(coarse, label, DTYPES[dt], ld_d=ld_w, ld=ld)
    assert torch.equal(d_w[:, :nc8], d) and bool((d_w[:, nc8:] == SENTINEL).all())
    return out4, lse, d


SWEEP = [pytest.param(s, n, id=f"{S.shape_id(s)}-{n}") for s, n in S.CLASS_CASES]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("shape,n_cls", SWEEP)
def test_kernels_against_float64(shape, n_cls, dt):
    (_fh, _fw), (H, W), N = shape
    if shape == S.PAST_256_PARTIALS:                               # what the case is there for: the finish kernel's second trip, an image
        assert S.forward_workgroups(shape) > 256 and (H * W) % 256 != 0 and N == 2 and n_cls == 21     # boundary inside a workgroup
    else:
        assert S.forward_workgroups(shape) <= 256
    _sweep_case(shape, n_cls, dt)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("n_cls", S.NC8_COUNTS)
@pytest.mark.parametrize("shape", S.NC8_SHAPES, ids=S.shape_id)
def test_every_class_chunk_count(shape, n_cls, dt):
    """the kernels are instantiated per number of 8-class chunks (1 .. 4): 9 / 16 classes run two, 25 / 32 four (21 runs three, 2 and 8 one).
    Rows of ld = the chunks themselves (16 and 32 classes: not one pad column anywhere), and rows 8 columns wider with the poison behind
    the chunks: the same bits."""
    nc8 = (n_cls + 7) // 8 * 8
    assert nc8 // 8 == {9: 2, 16: 2, 25: 4, 32: 4}[n_cls] and n_cls <= 32
    tight = _sweep_case(shape, n_cls, dt, ld=nc8)
    coarse, label, _ref = _case(shape, n_cls, dt)
    wide = _run(coarse, label, DTYPES[dt], ld=nc8 + 8)
    assert all(torch.equal(a, b) for a, b in zip(tight, wide))


def _torch_f64(coarse, label):
    x = coarse.double().requires_grad_()
    loss = F.cross_entropy(F.interpolate(x, label.shape[1:], mode="bilinear", align_corners=True), label.long(), ignore_index=255)
    loss.backward()
    return loss.detach(), x.grad


def test_all_ignored_batch_is_torchs_answer():
    coarse, label, _ref = _case(((5, 7), (33, 47), 1), 21, "f32")
    label = torch.full_like(label, 255)
    t_loss, t_grad = _torch_f64(coarse, label)                    # torch's float64 answer, taken at run time
    out4, _lse, d = _run(coarse, label, torch.float32)
    assert S.within(out4[0], t_loss, 0.0) and S.within(_grad_of(d, coarse), t_grad, 0.0)               # NaN where torch has NaN, equal elsewhere
    assert float(out4[1]) == 0.0 and float(out4[3]) == 0.0
    _o, _l, d_b = _run(coarse, label, torch.bfloat16, d_dtype=torch.bfloat16)
    assert S.within(_grad_of(d_b, coarse), t_grad, 0.0)


def test_out_of_range_labels_are_counted_and_ignored():
    coarse, label, _ref = _case(((5, 7), (33, 47), 1), 21, "f32")
    bad = label.clone()
    g = torch.Generator().manual_seed(5)
    where = torch.rand(label.shape, generator=g) < 0.1
    bad[where] = torch.randint(21, 255, (int(where.sum()),), generator=g, dtype=torch.int64).to(torch.uint8)
    bad[0, 0, 0], bad[0, -1, -1] = 21, 254                         # both ends of the range
    clean = torch.where(bad >= 21, torch.full_like(bad, 255), bad)
    n_bad = int(((bad >= 21) & (bad != 255)).sum())
    out4, lse, d = _run(coarse, bad, torch.float32)                # (_run synchronises: the run ends clean)
    out4_c, lse_c, d_c = _run(coarse, clean, torch.float32)
    assert float(out4[3]) == n_bad > 0 and float(out4_c[3]) == 0.0
    assert torch.equal(out4[:3], out4_c[:3]) and torch.equal(lse, lse_c) and torch.equal(d, d_c)        # they contribute nothing
    assert float(out4[1]) == float((clean < 21).sum())


def test_out_of_range_labels_at_nine_classes():
    """the same with 9 classes on rows of ld 16: the values 9 .. 15 are columns of the second chunk (zeros in the engine's rows, the poison here)
    and must be ignored like 254, never read as a class"""
    coarse, label, ref = _case(((5, 7), (33, 47), 1), 9, "f32")
    bad = label.clone()
    g = torch.Generator().manual_seed(6)
    where = torch.rand(label.shape, generator=g) < 0.1
    bad[where] = torch.randint(9, 255, (int(where.sum()),), generator=g, dtype=torch.int64).to(torch.uint8)
    bad[0, 0, 0], bad[0, 0, 1], bad[0, -1, -2], bad[0, -1, -1] = 9, 15, 16, 254      # both ends of the range, both sides of the chunk's end
    clean = torch.where(bad >= 9, torch.full_like(bad, 255), bad)
    n_bad = int(((bad >= 9) & (bad != 255)).sum())
    out4, lse, d = _run(coarse, bad, torch.float32, ld=16)
    out4_c, lse_c, d_c = _run(coarse, clean, torch.float32, ld=16)
    assert float(out4[3]) == n_bad > 0 and float(out4_c[3]) == 0.0
    assert torch.equal(out4[:3], out4_c[:3]) and torch.equal(lse, lse_c) and torch.equal(d, d_c)        # they contribute nothing
    assert float(out4[1]) == float((clean < 9).sum()) < float(ref["count"])
    ref_c = S.restate(coarse, clean)                                                                   # and what is left is the loss of the clean map
    _check(dict(loss=out4[0], lse=lse, grad=_grad_of(d, coarse)), ref_c, coarse, "9 classes, out-of-range labels")
    assert bool((d[:, 9:] == 0).all())


def test_gscale_is_exact_for_powers_of_two():
    coarse, label, _ref = _case(((5, 7), (33, 47), 1), 21, "f32")
    _o, _l, d1 = _run(coarse, label, torch.float32)
    for g in (0.25, 4.0, -2.0):
        _o, _l, dg = _run(coarse, label, torch.float32, gscale=g)
        assert torch.equal(dg, d1 * g), g


def test_loss_only_call_gives_the_same_bits():
    from wseg_amd.seg_loss import seg_ce_rows, seg_ce_rows_backward
    coarse, label, _ref = _case(((13, 16), (57, 301), 1), 21, "f32")
    rows = _rows(coarse, torch.float32)
    with_lse, _ctx = seg_ce_rows(rows, LD, label.cuda(), 1, 13, 16, 57, 301, 21)
    without, ctx0 = seg_ce_rows(rows, LD, label.cuda(), 1, 13, 16, 57, 301, 21, with_lse=False)
    assert torch.equal(with_lse.cpu(), without.cpu()) and ctx0["lse"] is None
    with pytest.raises(RuntimeError, match="with_lse=False"):
        seg_ce_rows_backward(ctx0)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_two_runs_are_bit_identical(dt):
    coarse, label, _ref = _case(((13, 16), (57, 301), 1), 21, dt)
    a = _run(coarse, label, DTYPES[dt], d_dtype=DTYPES[dt])
    b = _run(coarse, label, DTYPES[dt], d_dtype=DTYPES[dt])
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_image_one_of_a_batch_equals_the_image_alone():
    """two images with the SAME valid mask (so equal valid counts) and their own logits and classes: the batch's count is twice each image's, a
    power of two apart, so image 1's gradient rows are exactly half of what the image gives alone; its lse plane is the same bits"""
    g = torch.Generator().manual_seed(31)
    coarse = 4.0 * torch.randn(2, 21, 5, 7, generator=g)
    label = S.make_label(1, 33, 47, 21, 32).repeat(2, 1, 1)
    label[1] = torch.where(label[1] == 255, label[1], (label[1] + 3) % 21)
    out4, lse, d = _run(coarse, label, torch.float32)
    out4_1, lse_1, d_1 = _run(coarse[1:], label[1:], torch.float32)
    out4_0, _lse_0, _d_0 = _run(coarse[:1], label[:1], torch.float32)
    assert float(out4[1]) == 2 * float(out4_1[1]) == 2 * float(out4_0[1])
    assert torch.equal(lse[1], lse_1[0])
    assert torch.equal(d[35:] * 2, d_1)
    ref = S.restate(coarse, label)
    assert S.within(out4[0], ref["loss"], S.loss_bar(ref, coarse))
    assert abs(float(out4[0]) - 0.5 * (float(out4_0[0]) + float(out4_1[0]))) <= 2 * S.loss_bar(ref, coarse)


@pytest.mark.parametrize("label_dtype", [torch.uint8, torch.int64])
@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("n_cls", [21, 8, 16, 32])                   # 8, 16, 32 (one, two, four whole chunks): channels_last rows are consumed
def test_autograd_wrapper(n_cls, dt, channels_last, label_dtype):    # in place; 21: packed into rows of ld 24
    from wseg_amd.seg_loss import seg_cross_entropy
    shape = ((5, 7), (33, 47), 3)
    coarse, label, ref = _case(shape, n_cls, dt)
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    x = coarse.to(DTYPES[dt]).cuda().contiguous(memory_format=fmt).requires_grad_()
    loss, stats = seg_cross_entropy(x, label.to(label_dtype).cuda())
    if channels_last and n_cls % 8 == 0:                             # no copy: the loss's rows ARE x's storage
        assert loss.grad_fn.saved["rows"].data_ptr() == x.data_ptr()
    (loss * 0.5).backward()
    assert x.grad.dtype == DTYPES[dt] and x.grad.shape == x.shape and x.grad.is_contiguous(memory_format=fmt)
    assert not stats.requires_grad and float(stats[0]) == float(loss.detach()) and float(stats[1]) == float(ref["count"]) and float(stats[3]) == 0.0
    half = dict(ref, grad=0.5 * ref["grad"])
    got = dict(loss=loss.detach().cpu(), grad=x.grad.float().cpu())
    _check(got, half, coarse, f"wrapper n_cls {n_cls} {dt} channels_last={channels_last} {label_dtype}", gscale=0.5, grad_store_bf16=dt == "bf16")
    # the plain-torch chain on the device (f32, on the same values): both sides lie within one bar of float64, so within two of each other
    y = coarse.cuda().requires_grad_()
    lab = label.long().cuda()
    p_loss = F.cross_entropy(F.interpolate(y, (33, 47), mode="bilinear", align_corners=True), lab, ignore_index=255)
    (p_loss * 0.5).backward()
    gb = S.grad_bar(ref, coarse, 0.5)
    gb = S.bf16_store_bar(half["grad"], gb) if dt == "bf16" else gb
    assert abs(float(loss.detach()) - float(p_loss.detach())) <= 2 * S.loss_bar(ref, coarse)
    assert bool(((x.grad.float().cpu().double() - y.grad.cpu().double()).abs() <= 2 * gb).all())


def test_bad_arguments_are_refused():
    from wseg_amd import _lib as L
    from wseg_amd.seg_loss import seg_ce_rows, seg_cross_entropy
    coarse, label, _ref = _case(((5, 7), (33, 47), 1), 21, "f32")
    rows, lab = _rows(coarse, torch.float32), label.cuda()
    with pytest.raises(RuntimeError):
        seg_ce_rows(rows[:, :16].contiguous(), 16, lab, 1, 5, 7, 33, 47)                                 # ld < 24
    big = torch.zeros(35 * LD + 8, device="cuda")
    with pytest.raises(ValueError, match="16-byte aligned"):
        seg_ce_rows(big[2:], LD, lab, 1, 5, 7, 33, 47)                                                   # rows 8 bytes off
    out4, ws = torch.empty(4, device="cuda"), torch.empty(L.seg_ce_workspace_bytes(1, 33, 47), device="cuda", dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="not 16-byte aligned"):
        L.seg_ce_forward(big[2:], LD, lab, None, ws, out4, 1, 5, 7, 33, 47, 21)                          # ... refused by the library as well
    with pytest.raises(RuntimeError, match="n_cls=33"):
        seg_ce_rows(torch.zeros(35, 40, device="cuda"), 40, lab, 1, 5, 7, 33, 47, n_cls=33)
    with pytest.raises(ValueError, match="label map"):
        seg_ce_rows(rows, LD, lab[:, :32], 1, 5, 7, 33, 47)                                              # a label shape mismatch
    with pytest.raises(TypeError):
        seg_ce_rows(rows, LD, lab.float(), 1, 5, 7, 33, 47)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg_ce_rows(rows.cpu(), LD, lab, 1, 5, 7, 33, 47)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg_cross_entropy(coarse, label)
    torch.cuda.synchronize()
