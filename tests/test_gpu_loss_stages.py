"""The loss phase of the contrast step (wseg_amd/loss_hip.py `step`, between Engine.run_forward and Engine.run_backward) stage by stage against
float64 in every precision mode.  Each stored tensor — the plane statistics of cam_low and rvd, bias, q / argc, the min-pool selection, c and
r, F, the 16 x 16 rvd, ncam / y, the prototype candidates and the prototypes; Gc, dlt, the 2N-row ECR selection, Gr; d_cam_low and d_rvd; the
records, the hard-pixel weights, dF; d_head; the seven slots of acc and out8 — is compared AT EVERY ELEMENT with the float64 statement of its
stage (tests/loss_f64.py, pinned to oracle/loss.py by tests/test_loss_host.py), computed from the tensors the device stored for that stage's
inputs, under the device's own stored decisions, inside the bars the kernel tests derive.  No bar is fitted.

The Recorder wraps the wseg_amd._lib entry points `step` calls, Engine.run_forward and Engine.run_backward (a monkeypatch, undone at the end of
the test) and keeps the arguments of every call.  ONLY ROLES are read from it: which device tensor is st_cam, q, dlt, res, acc, rec, d_head ...,
that a per-view launch was handed the tensors of ITS view (data pointers and storage offsets), and the scalar arguments as passed (asserted
against their definitions; the float64 references compute the coefficients themselves).  d_rvd and d_head are asserted to be the very tensors
handed to run_backward.  The phase runs on four streams and everything is read after ONE torch.cuda.synchronize(): a result read before its
event shows as a stage outside its bar.

Cases (nets of test_gpu_trunk_stages._net: procedural weights, injected dropout tables; world = 1):
  A  view 1 104 x 104 (a 13 x 13 map, not a multiple of 4, up-sampled to 16 x 16), view 2 128 x 128 (the 16 x 16 shortcut), N = 2; one image
     with a single class, one with three: seventeen classes absent from the batch.
  B  view 1 160 x 160 (20 x 20, down-sampled to 16 x 16), view 2 128 x 128, N = 3; one image carries all twenty classes.
  C  fp32 only, rng_parity=True with a seeded random.Random: the sort-based intra_weights path and _rand_flags; the weights also against the
     oracle's recorded selections on the stored similarities.
The conditions of the judgement (tests/test_loss_host.py check_conditions: undecided rank-band pixels <= 2 % per view, pseudo-label near-ties,
no exact tie of values at the ECR / min-pool thresholds) are asserted on the device's own tensors.

Cost.  Measured per case on an MI355X host (16 cores), pytest's call time: 2.4 s for the first case of the run and 0.9 - 1.0 s for the first
case of each other mode (they build that mode's net and packs); every other case 0.17 - 0.18 s, of which the step with its read-back takes
0.02 - 0.03 s and the float64 references 0.09 - 0.14 s.  The per-stage table of that run: profiles/r27_loss_stages_f64.txt."""
import random
import time

import numpy as np
import pytest
import torch

from oracle import loss as oloss
from tests import loss_f64 as LF
from tests.test_gpu_trunk_stages import DEV, MODES, _net
from tests.test_loss_host import BG, CASES, check_conditions, label_rows, weights_from_selections
from wseg_amd import synth

pytestmark = pytest.mark.gpu
IMG_SEED, MASK_SEED = 17, 60
ENTRIES = ("up_plane_stats", "cls_loss", "up_rvmin_values", "select_kth", "select_finish", "up_norm_resize_forward", "rows_resize_forward",
           "resize_planar_fwd", "pseudo_label", "proto_candidates", "proto_merge", "er_ecr_prep", "ecr_backward", "up_maps_backward", "nce_records",
           "intra_weights", "intra_weights_global", "nce_fused", "head_grad_fused", "loss_finish")


def _same(a, b):
    """the same device elements: one object, or two views of the same storage range"""
    return a is b or (torch.is_tensor(a) and torch.is_tensor(b) and a.data_ptr() == b.data_ptr() and a.numel() == b.numel() and a.dtype == b.dtype)


def _at(t, base, elems):
    """t starts `elems` elements into base"""
    return t.untyped_storage().data_ptr() == base.untyped_storage().data_ptr() and t.storage_offset() == base.storage_offset() + elems


def _eq(a, b):
    return abs(a - b) <= 1e-12 * abs(b)


class Recorder:
    def __init__(self, monkeypatch):
        from wseg_amd import _lib as L, engine as E
        self.calls = {k: [] for k in ENTRIES}
        self.kw = {k: [] for k in ENTRIES}
        self.fwd = self.bwd = None
        rec, rf0, rb0 = self, E.Engine.run_forward, E.Engine.run_backward

        def run_forward(self_, xs, **kw):
            out = rf0(self_, xs, **kw)
            rec.fwd = (xs, out[0], out[1])
            return out

        def run_backward(self_, S, grads, d_head_rows=None):
            rec.bwd = (S, grads, d_head_rows)
            return rb0(self_, S, grads, d_head_rows=d_head_rows)

        def entry(name, fn0):
            def f(*a, **kw):
                rec.calls[name].append(a)
                rec.kw[name].append(kw)
                return fn0(*a, **kw)
            return f

        monkeypatch.setattr(E.Engine, "run_forward", run_forward)
        monkeypatch.setattr(E.Engine, "run_backward", run_backward)
        for name in ENTRIES:
            monkeypatch.setattr(L, name, entry(name, getattr(L, name)))

    def record(self, N, label20, mode, parity):
        """the loss phase's tensors by role, from the launches' arguments, with the wiring asserted; -> (device record, out8)"""
        from wseg_amd.loss_hip import _CAND_L
        k = self.calls
        xs, outs, S = self.fwd
        Sb, grads, d_head = self.bwd
        assert Sb is S and len(xs) == 2
        npix, P, K_ecr = LF.NPIX, N * 256, LF.k_ecr()
        (fin,) = k["loss_finish"]
        acc, out8 = fin[0], fin[2]
        assert _eq(fin[1], 1.0 / (N * 20 * npix)) and acc.shape == (8,)
        lab_dev = k["cls_loss"][0][1]
        assert torch.equal(lab_dev.cpu().double(), label20)
        assert len(k["up_plane_stats"]) == 4 and len(k["up_norm_resize_forward"]) == 4 and len(k["up_maps_backward"]) == 4
        (prep,) = k["er_ecr_prep"]
        (eb,) = k["ecr_backward"]
        (rc,) = k["nce_records"]
        (nf,) = k["nce_fused"]
        dlt, res_ecr, Gr = eb[0], eb[1], eb[2]
        rec_t = rc[0][0]["rec"]
        assert self.kw["nce_records"][0].get("split_bf16", False) == (mode != "fp32") and rc[1] == P
        assert _same(prep[6], dlt[:N]) and _same(prep[7], dlt[N:]) and _at(prep[8], acc, 2) and prep[9:11] == (N, npix) and _eq(prep[11], 1.0 / (N * 20 * npix))
        sk, sf = k["select_kth"], k["select_finish"]
        assert len(sk) == 3 and len(sf) == 3
        assert _same(sk[2][0], dlt) and sk[2][1:7] == (2 * N, 21 * npix, K_ecr, True, True, False) and _same(sk[2][7], res_ecr)
        assert _same(sf[2][0], res_ecr) and sf[2][1:4] == (2 * N, K_ecr, False) and _eq(sf[2][4], 1.0 / (N * K_ecr)) and _at(sf[2][5], acc, 3)
        assert eb[3:6] == (2 * N, 21 * npix, K_ecr) and _eq(eb[6], 1.0 / (N * K_ecr))
        assert nf[1] == P and _eq(nf[2], 0.1 / (2 * P)) and _eq(nf[3], 0.05) and _at(nf[4], acc, 4)
        assert d_head is not None and d_head.shape == S["head"].shape and d_head.dtype == S["head"].dtype
        cand0 = k["proto_candidates"][0][3]
        views, dv = [], []
        for i, (x, o, vw) in enumerate(zip(xs, outs, S["views"])):
            Sz, h, w, off = x.shape[2], vw["h"], vw["w"], vw["off"]
            cam_low, rvd, head = o[0], o[1], o[3]
            assert _at(head, S["head"], off * LF.HEAD_LD) and cam_low.shape == rvd.shape == (N, 21, h, w) and x.shape[2] == x.shape[3]
            ua, ub = k["up_plane_stats"][2 * i], k["up_plane_stats"][2 * i + 1]
            assert _same(ua[0], cam_low) and len(ua) == 6 and ua[2:] == (N * 21, h, w, Sz)
            assert _same(ub[0], rvd) and ub[2:6] == (N * 21, h, w, Sz) and _same(ub[6], lab_dev)
            st_cam, st_rv = ua[1], ub[1]
            cl = k["cls_loss"][i]
            assert _same(cl[0], st_cam) and _at(cl[2], acc, 0) and cl[4:] == (N, Sz * Sz, 0.5)
            bias = cl[3]
            rm = k["up_rvmin_values"][i]
            assert _same(rm[0], rvd) and rm[4:] == (N, h, w, Sz)
            q, argc = rm[2], rm[3]
            kmin = Sz * Sz // 4
            assert _same(sk[i][0], q) and sk[i][1:7] == (N, Sz * Sz, kmin, False, False, True)
            res_min = sk[i][7]
            assert _same(sf[i][0], res_min) and sf[i][1:4] == (N, kmin, True) and _eq(sf[i][4], 0.5 / (kmin * N)) and _at(sf[i][5], acc, 1)
            na, nb = k["up_norm_resize_forward"][2 * i], k["up_norm_resize_forward"][2 * i + 1]
            assert _same(na[0], cam_low) and _same(na[1], st_cam) and _same(nb[0], rvd) and _same(nb[1], st_rv) and na[4:] == nb[4:] == (N, h, w, Sz, 128)
            c, r_ = na[3], nb[3]
            assert _same(prep[i], c) and _same(prep[2 + i], r_)
            Gc = prep[4 + i]
            rr = k["rows_resize_forward"][i]
            assert _same(rr[0], head) and rr[1] == LF.HEAD_LD and rr[3:] == (N, h, w, 16, 16)
            Fm = rr[2]
            pl = k["pseudo_label"][i]
            if (h, w) == (16, 16):
                assert _same(pl[0], rvd)                                   # the shortcut: rvd itself
                R = rvd
            else:
                (rz,) = [a for a in k["resize_planar_fwd"] if _same(a[0], rvd)]
                assert rz[2:] == (N * 21, h, w, 16, 16, True) and _same(pl[0], rz[1])
                R = rz[1]
            assert _eq(pl[2], BG) and pl[5:] == (N, 256)
            y, ncam = pl[3], pl[4]
            pc = k["proto_candidates"][i]
            assert _same(pc[0], ncam) and _same(pc[1], Fm) and pc[6:] == (N, 256, LF.CAND_K) and _at(pc[3], cand0, i * _CAND_L)
            cv, cf, cc, tie = pc[3], pc[4], pc[5], pc[2]
            pm = k["proto_merge"][i]
            assert pm[0].data_ptr() == cv.data_ptr() and pm[1].data_ptr() == cf.data_ptr() and pm[2].data_ptr() == cc.data_ptr() and pm[4:6] == (1, LF.CAND_K)
            protos = pm[3]
            (mc,) = [a for a in k["up_maps_backward"] if _same(a[0], Gc)]
            assert _same(mc[1], cam_low) and _same(mc[2], st_cam) and _same(mc[4], bias) and mc[7:12] == (None, None, None, 0, 0.0) and mc[13:] == (N, h, w, Sz, 128)
            assert mc[5].shape == (h,) and mc[6].shape == (w,)
            (mr,) = [a for a in k["up_maps_backward"] if a[7] is not None and _same(a[7], q)]
            assert _same(mr[0], Gr[i * N:(i + 1) * N]) and _same(mr[1], rvd) and _same(mr[2], st_rv) and mr[4:7] == (None, None, None)
            assert _same(mr[8], argc) and _same(mr[9], res_min) and mr[10] == kmin and _eq(mr[11], 0.5 / (kmin * N)) and mr[13:] == (N, h, w, Sz, 128)
            d_cam_low, d_rvd = mc[12], mr[12]
            assert grads[i][0] is None and grads[i][2] is None and grads[i][3] is None and _same(grads[i][1], d_rvd)      # the very tensor handed on
            rv_ = rc[0][i]
            assert _same(rv_["F"], Fm) and _same(rv_["p_own"], protos) and _same(rv_["y_own"], y) and _at(rv_["rec"], rec_t, i * 3 * P)
            rkey = flags = None
            if parity:
                iw = k["intra_weights"][i]
                assert _same(iw[0], y) and _at(iw[1], rec_t, i * 3 * P + P) and iw[2] is None and iw[5] == P and self.kw["intra_weights"][i] == dict(ld_s=1)
                assert rv_.get("rkey") is None and not k["intra_weights_global"]
                flags, w_intra = iw[3], iw[4]
            else:
                ig = k["intra_weights_global"][i]
                assert _at(ig[0], rec_t, i * 3 * P) and ig[2:] == (P, 1, 0, 1.0, 6 * P) and not k["intra_weights"]
                rkey, w_intra = rv_["rkey"], ig[1]
            fv, fo = nf[0][i], nf[0][1 - i]
            assert _same(fv["F"], Fm) and _same(fv["p_own"], protos) and _same(fv["y_own"], y) and _same(fv["w_intra"], w_intra)
            assert _same(fv["p_oth"], fo["p_own"]) and _same(fv["y_oth"], fo["y_own"]) and not _same(fv["p_oth"], protos)
            dF = fv["dF"]
            hg = k["head_grad_fused"][i]
            assert _same(hg[0], dF) and _same(hg[1], d_cam_low) and _same(hg[2], head) and _at(hg[3], d_head, off * LF.HEAD_LD) and hg[4:] == (LF.HEAD_LD, N, h, w, 16, 16)
            dv.append(dict(cam_low=cam_low, rvd=rvd, head=head.reshape(-1, LF.HEAD_LD), st_cam=st_cam, st_rv=st_rv, bias=bias, q=q.view(N, -1), argc=argc.view(N, -1), res_min=res_min,
                           c=c, r=r_, F=Fm, R=R.reshape(N, 21, 16, 16), y=y, ncam=ncam.view(N, 21, 256), cv=cv.view(21, LF.CAND_K), cf=cf.view(21, LF.CAND_K, 128),
                           cc=cc.view(-1)[:21], protos=protos, Gc=Gc.view(N, 21, 128, 128), d_cam_low=d_cam_low, d_rvd=d_rvd, rkey=rkey, flags=flags,
                           w_intra=w_intra, dF=dF, tie=tie, rec=rv_["rec"]))
            views.append(dict(S=Sz, h=h, w=w, off=off))
        dg = dict(dlt=dlt, res_ecr=res_ecr, Gr=Gr.view(2 * N, 21, 128, 128), acc=acc, out8=out8, d_head=d_head)
        return views, dv, dg


def _cpu(t):
    if t is None:
        return None
    return t.detach().cpu().long() if not t.is_floating_point() else t.detach().float().cpu().double()


def _to_record(N, label20, views, dv, dg):
    """the device record as tests/loss_f64.py reads it: float64 / int64 CPU tensors, the statistics split into their columns"""
    from tests.f64_bars import _bits
    P = N * 256
    lab = LF._label_full(label20).view(-1) > 0
    r = dict(N=N, label20=label20, bg=BG, tie=_cpu(dv[0]["tie"]), M=dg["d_head"].shape[0], views=[])
    for i, (v, d) in enumerate(zip(views, dv)):
        v = dict(v)
        for which in ("cam", "rv"):
            st = d["st_" + which].detach().cpu()
            live = lab if which == "rv" else torch.ones_like(lab)
            mn = st[:, 1].double()
            # planes the label mask skips keep the initial keys: max 0, min all-ones bits (a NaN), sum 0, both indices -1
            assert bool(torch.isnan(mn[~live]).all()) and bool((st[:, 0][~live] == 0).all())
            v[which + "_max"], v[which + "_min"], v[which + "_sum"] = st[:, 0].double(), torch.where(live, mn, torch.zeros((), dtype=torch.float64)), st[:, 2].double()
            v[which + "_imx"], v[which + "_imn"] = _bits(st[:, 3]), _bits(st[:, 4])
        for key in ("cam_low", "rvd", "head", "bias", "q", "argc", "res_min", "c", "r", "F", "R", "y", "ncam", "cv", "cf", "cc", "protos", "Gc", "d_cam_low",
                    "d_rvd", "rkey", "flags", "w_intra", "dF"):
            v[key] = _cpu(d[key])
        rec = d["rec"].detach().cpu().view(3, P)
        r[f"rec_y.v{i}"], r[f"sim.v{i}"] = rec[0].view(torch.int32).long(), rec[1].double()
        if v["rkey"] is not None:
            r[f"rec_key.v{i}"] = rec[2].double()
        r["views"].append(v)
    for key in ("dlt", "res_ecr", "Gr", "acc", "out8", "d_head"):
        r[key] = _cpu(dg[key])
    return r


def _run(monkeypatch, case, mode, parity=False):
    from wseg_amd import loss_hip
    from wseg_amd.train import second_view
    c = CASES[case]
    N = c["N"]
    net = _net("contrast", mode)
    net.train()
    eng = net._engine
    label20 = label_rows(c["labels"])
    img1 = synth.synthetic_images(N, c["S"][0], IMG_SEED + N).to(DEV)
    img2 = second_view(img1)
    assert tuple(img2.shape[2:]) == (c["S"][1],) * 2
    net.set_dropout_masks([synth.synthetic_dropout_masks(N, MASK_SEED), synth.synthetic_dropout_masks(N, MASK_SEED + 1)])
    torch.manual_seed(23)                                     # the random keys of the hard-pixel sampling
    rec = Recorder(monkeypatch)
    got = loss_hip.step(net, img1, img2, label20.float().to(DEV), BG, random.Random(5) if parity else None, parity, zero_grads=True)
    torch.cuda.synchronize()
    views, dv, dg = rec.record(N, label20, mode, parity)
    assert all(v.data_ptr() == dg["out8"].data_ptr() + 4 * j for j, v in enumerate(got.values()))     # what the step returns is what is judged
    return _to_record(N, label20, views, dv, dg)


def _report(tag, r, mode, t0):
    t1 = time.perf_counter()
    table = LF.judge(r, mode)
    print(f"\n== {tag}")
    for name, n, ratio, ok, differs, left in table:
        print(f"{name:28s} elements {n:8d}  max err/bar {ratio:8.4f}  decisions differing {differs:5d}  left out {100 * left:6.3f} %{'' if ok else '   OUTSIDE'}")
    cond = LF.conditions(r)
    print(f"[{tag}] conditions {cond}")
    print(f"[{tag}] {len(table)} stored tensors judged; step + read-back {t1 - t0:.2f} s, float64 references {time.perf_counter() - t1:.2f} s")
    bad = [row for row in table if not row[3]]
    assert not bad, bad
    assert {LF.row_of(row[0]) for row in table} == set(LF.ROW_ORDER) - {"acc"} and sum(1 for row in table if ":acc." in row[0]) == 7
    check_conditions(cond)
    return table


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ["A", "B"])
def test_loss_phase_stage_by_stage(monkeypatch, case, mode):
    t0 = time.perf_counter()
    r = _run(monkeypatch, case, mode)
    dims = [(v["h"], v["w"]) for v in r["views"]]
    assert dims == ([(13, 13), (16, 16)] if case == "A" else [(20, 20), (16, 16)]) and r["views"][1]["off"] == r["N"] * dims[0][0] * dims[0][1]
    _report(f"case {case} [{mode}]", r, mode, t0)


def test_loss_phase_rng_parity_path(monkeypatch):
    """case C: the geometry of case A in fp32 with rng_parity=True — intra_weights (the sort in LDS) with the host flags of _rand_flags.  The
    stage judge holds the weights to the rule on the stored flags; here the flags and the rank band are also held to the ORACLE's selections,
    intra_view_nce run with the same random stream on the stored labels and similarities (pixels whose similarity is an exact duplicate
    within their class may be ordered either way)."""
    t0 = time.perf_counter()
    r = _run(monkeypatch, "A", "fp32", parity=True)
    _report("case C [fp32, rng_parity]", r, "fp32", t0)
    rng = random.Random(5)
    for i, v in enumerate(r["views"]):
        y, sim, P = v["y"], r[f"sim.v{i}"], v["y"].shape[0]
        fo = torch.zeros(P, 128, dtype=torch.float64)
        fo[torch.arange(P), y] = sim                          # features whose similarity to prototype e_y is the stored record
        sel = []
        oloss.intra_view_nce(fo, y, torch.eye(21, 128, dtype=torch.float64), rng, sel)
        want = weights_from_selections(y, sel)
        differ = np.nonzero(((v["w_intra"] - want).abs() > 1e-6 * float(want.max())).numpy())[0]
        for p in differ:
            assert int(((y == y[p]) & (sim == sim[p])).sum()) > 1, (i, int(p))
        print(f"[case C] view {i}: {len(differ)} of {P} weights differ from the oracle's selections (exact duplicates of a similarity)")
        assert float(want.sum()) > 0 and len(differ) <= 0.02 * P
