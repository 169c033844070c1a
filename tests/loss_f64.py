"""The loss phase (wseg_amd/loss_hip.py `step`, between Engine.run_forward and Engine.run_backward) stated in float64, one function per
stage, each with the per-element bar of its stage.  TEST INFRASTRUCTURE, no tests here.

Part 1: the float64 references and bar helpers of the kernel-by-kernel tests (moved from tests/test_gpu_loss_kernels.py, which imports them;
bodies unchanged except that _nce_reference takes the arithmetic's dtype and knows bit-identical prototype rows, see there).

Part 2: the stages in the order `step` runs them.  A stage is a function st_*(A, r[, v]) -> {key: (value, bar)} over the record r (dict; per
view r["views"][i]): it reads the STORED inputs of its stage from the record and states what the stage stores.  The same functions serve
  * run_chain: A.own, arithmetic A.dt (float64: the pin of tests/test_loss_host.py; float32: the honest emulation), decisions taken by the
    stage itself, results rounded as stored and written into the record, optionally with ONE planted wiring defect;
  * judge: float64 under the record's own stored decisions; every stored element is compared with (value, bar), and every decision that
    differs from float64's must be a near-tie of the float64 values within the stage's value bar.
Coefficients are computed here from their definitions (0.5 / (k_min N), 1 / (N 20 npix), 1 / (N K_ecr), 0.1 / (2 P), 0.05), never read
from the record: a launch handed another coefficient leaves the bar of its stage.

Bars (u = U32 = 2^-24, SAFETY = 2) are the kernel tests' derivations, restated per stage beside the code; none is fitted.  Where a stage adds
something to a kernel test's situation the derivation is written there (the ER sum's |a - b| rounding, 1 - max in dlt, the undecided rank
band's share of the intra sum).

Decisions: plane arg-max / arg-min, arg channel of the min-pool, top-k thresholds (exact on the stored f32 values), max_onehot (exact on the
stored values), the zeroing and arg-max of the pseudo-labels, top-32 membership (exact, lowest index first), hard-pixel selections (integer
rule on the stored records), and the rank band 3..12 of nce_fused, which is not stored: pixels whose float64 gap at rank 2/3 or 12/13 is
below 2 S_BAR are left out of the dF comparison (share capped by NCE_MAX_EXCLUDED per view); a boundary between two prototypes with
bit-identical rows is no decision (value and gradient are the same either way) and does not count.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from .f64_bars import SAFETY, U32, _coord_bar, _interp_bar

F64 = torch.float64
HEAD_LD = 192


# ================================================================================================ part 1: moved from test_gpu_loss_kernels.py
def _up64(low, S):
    """bilinear align_corners=True upsample of [planes, h, w] -> [planes, S, S] in float64."""
    return F.interpolate(low.double()[None], size=(S, S), mode="bilinear", align_corners=True)[0]


def _resize64(x, oh, ow, align):
    return F.interpolate(x.double()[None], size=(oh, ow), mode="bilinear", align_corners=align)[0]


def _resize_bwd64(g, ih, iw, align):
    x = torch.zeros(g.shape[0], ih, iw, dtype=torch.float64, requires_grad=True)
    (_resize64(x, g.shape[1], g.shape[2], align) * g.double()).sum().backward()
    return x.grad


def _select_ref(v64, k, largest, use_abs, relu):
    f = v64.abs() if use_abs else v64
    thr = torch.sort(f, dim=1, descending=largest).values[:, k - 1]
    beyond = f > thr[:, None] if largest else f < thr[:, None]
    term = f.clamp_min(0) if relu else f
    zero = torch.zeros((), dtype=torch.float64)
    return (thr, torch.where(beyond, term, zero).sum(1), beyond.sum(1).double(), (f == thr[:, None]).sum(1).double(),
            torch.where(beyond, term.abs(), zero).sum(1))


def _stats_chain(S, chunks):
    # up_stats_partial: S*S / (256 chunks) serial adds per thread, an 8-level LDS tree, then `chunks` same-address atomics
    return math.ceil(S * S / (256 * chunks)) + 8 + chunks


def _exact_grid(h, w, S):
    return (h - 1) * 16 % (S - 1) == 0 and (w - 1) * 16 % (S - 1) == 0


def _max_norm_inj(U, imx, imn, e=1e-5):
    """max_norm of [planes, S*S] with max / min taken at the given positions (the kernel's decisions)."""
    R = U.clamp_min(0)
    rows = torch.arange(U.shape[0])
    mx, mn = R[rows, imx][:, None], R[rows, imn][:, None]
    return (R - mn - e).clamp_min(0) / (mx - mn + e)


def _label_full(label20):
    return torch.cat([torch.ones(label20.shape[0], 1), label20], 1).double()


def _protos64(vals, feats):
    """float64 weighted mean + F.normalize over a given candidate set: vals [21, K], feats [21, K, 128]."""
    v, f = vals.double(), feats.double()
    return F.normalize((v[:, :, None] * f).sum(1) / v.sum(1, keepdim=True), dim=-1)


def _proto_bar(vals, feats, K):
    # acc: K products + K adds (2K roundings of sum|v f|), wsum: K adds of sum|v|, the division 1; then the norm (a 2-wave
    # block sum: 7 levels, sqrt, max, division: 10 roundings) relative to the prototype
    v, f = vals.double(), feats.double()
    ws = v.sum(1, keepdim=True)
    pr = (v[:, :, None] * f).sum(1) / ws
    dpr = (2 * K * U32 * (v[:, :, None] * f).abs().sum(1) + pr.abs() * K * U32 * v.abs().sum(1, keepdim=True)) / ws.abs() + U32 * pr.abs()
    nrm = pr.norm(dim=1, keepdim=True)
    return SAFETY * (dpr / nrm + dpr.norm(dim=1, keepdim=True) / nrm * (pr.abs() / nrm) + 10 * U32 * pr.abs() / nrm)


# delta S, the error of one f32 similarity against normalize(F) . p in float64 (|S| <= 1): the row norm is a 32-term lane chain plus
# two shuffles (34), the contraction a chain of at most 128 MFMA partial sums with sum|terms| <= |F| |p| = |F| (Cauchy-Schwarz; the
# prototypes are unit vectors), scaled by 1 / |F|.  S_ERR is the raw figure, S_BAR the bar (the safety factor applied once).
S_ERR = (128 + 34) * U32
S_BAR = SAFETY * S_ERR                       # 1.9e-5
S_SPLIT = 3e-6                               # the split-bf16 record pass against the exact one (test_nce_records' bar)
ITAU = 10.0                                  # 1 / tau, tau = 0.1
NCE_CI = 0.05                                # coef_intra; coef_cross = 0.1 / (2 P) (the step's values at world 1)
NCE_MAX_EXCLUDED = 0.02                      # share of pixels per view whose rank band 3..12 may be undecided at S_BAR


def _nce_reference(V, cc, ci, with_grad, dt=torch.float64):
    """float64 restatement of contrast_train.py:245-334 for both views (tau = 0.1): per view the per-pixel cross-prototype,
    cross-pseudo-label and intra-view terms, the rank band, and (with_grad) dF through the F.normalize backward with the
    elementwise error bar of the kernel's chain.  V[i]: F, p, y, w (f32 / int CPU tensors); w is used as given.
    dt: the arithmetic (float32 for the host emulation of tests/test_loss_host.py).  A rank boundary (2/3 or 12/13) between two prototypes
    whose rows are bit-identical is no decision — either order gives the same value and the same gradient — and is not `undecided`."""
    out = []
    for v, o in ((V[0], V[1]), (V[1], V[0])):
        P = v["F"].shape[0]
        F64_ = v["F"].to(dt)
        nr = F64_.norm(dim=1, keepdim=True)
        fn = F64_ / nr.clamp_min(1e-12)
        Po, Pt = v["p"].to(dt), o["p"].to(dt)
        So, St = fn @ Po.T, fn @ Pt.T
        yo, yt = v["y"].long()[:, None], o["y"].long()[:, None]
        # semi-hard negatives: similarity ranks 3..12, descending, the lower class first on a tie (:293-294)
        srt, order = torch.sort(So, dim=1, descending=True, stable=True)
        neg = torch.zeros(P, 21, dtype=dt).scatter_(1, order[:, 3:13], 1.0)
        inf = torch.full((), float("inf"), dtype=dt)
        same_a = (Po[order[:, 2]] == Po[order[:, 3]]).all(1)
        same_b = (Po[order[:, 12]] == Po[order[:, 13]]).all(1)
        gap = torch.minimum(torch.where(same_a, inf, srt[:, 2] - srt[:, 3]), torch.where(same_b, inf, srt[:, 12] - srt[:, 13]))
        dead = nr[:, 0] == 0                                  # S == 0 exactly on both sides: the stated tie rule decides, exactly
        r = dict(So=So, yo=yo, undecided=(gap < 2 * S_BAR) & ~dead, dead=dead)
        Eo, Et = torch.exp(ITAU * So), torch.exp(ITAU * St)
        oh_yo = torch.zeros(P, 21, dtype=dt).scatter_(1, yo, 1.0)
        oh_yt = torch.zeros(P, 21, dtype=dt).scatter_(1, yt, 1.0)
        m = neg + oh_yo                                       # the positive, and the band (the positive again if it lies inside)
        a2 = (m * Eo).sum(1, keepdim=True)
        sig_o, sig_t, q = Eo / Eo.sum(1, keepdim=True), Et / Et.sum(1, keepdim=True), m * Eo / a2
        r["L"] = (-torch.log(sig_t.gather(1, yo))[:, 0], -torch.log(sig_o.gather(1, yt))[:, 0], -torch.log(Eo.gather(1, yo) / a2)[:, 0])
        if with_grad:
            w = v["w"].to(dt)[:, None]
            kc, ki = cc * ITAU, ci * ITAU * w
            dSo = kc * (sig_o - oh_yt) + ki * (q - oh_yo)
            dSt = kc * (sig_t - oh_yo)
            dfn = dSo @ Po + dSt @ Pt
            dot = (dfn * fn).sum(1, keepdim=True)
            inv = torch.where(dead[:, None], torch.zeros((), dtype=dt), 1.0 / nr.clamp_min(1e-300 if dt == torch.float64 else 1e-37))
            r["dF"] = (dfn - fn * dot) * inv
            # ---- the bar of dF, term by term (raw errors; SAFETY once at the end)
            # e = expf(10 S): the product rounds (10 u on the exponent), expf 2 u -> 12 u relative; a softmax entry s = e / sum: 12 u
            # + (12 + 21) u of the 21-term sum + 1 u of the division = 46 u relative; through delta S it moves by
            # sum_j |ds/dS_j| S_ERR = 10 s * 2 (1 - s) S_ERR <= 20 s S_ERR.  The same holds for q (entries sum to 1, <= 13 terms).
            # dS = kc (s - [c == y]) + ki (q - [c == y]): each difference 1 rounding, kc 1 and ki 2 roundings and their products 1
            # each (<= 4 u of the term), the final add 1 u of dS.
            rel = 20 * S_ERR + 46 * U32
            e_dSo = rel * (kc * sig_o + ki * q) + 4 * U32 * (kc * (sig_o - oh_yt).abs() + ki * (q - oh_yo).abs()) + U32 * dSo.abs()
            e_dSt = rel * kc * sig_t + 5 * U32 * dSt.abs()
            # d fn = dS . P: a chain of 44 MFMA terms on sum |dS| |P|
            e_dfn = e_dSo @ Po.abs() + e_dSt @ Pt.abs() + 44 * U32 * (dSo.abs() @ Po.abs() + dSt.abs() @ Pt.abs())
            # fn = F * (1 / |F|): the norm 17 u (half of the 34-chain of its square) + sqrt, reciprocal, product: 20 u, the product
            # 1 u more; dot = sum_128 dfn fn: 32 products per lane + 2 shuffles (34) and 1 u per product
            e_dot = (e_dfn * fn.abs()).sum(1, keepdim=True) + (21 + 35) * U32 * (dfn * fn).abs().sum(1, keepdim=True)
            # dF = (dfn - fn dot) * inv: fn dot carries fn's 21 u and 1 u, the difference 1 u, inv 20 u and the product 1 u
            bar = inv * (e_dfn + fn.abs() * e_dot + 22 * U32 * (fn * dot).abs()) + 22 * U32 * r["dF"].abs()
            r["dF_bar"] = SAFETY * bar
        out.append(r)
    return out


def _nce_sum_bar(L, weight, P):
    """|sum_f32 - sum_64| of one loss sum = sum_p weight_p L_p.  Per pixel L = -log(e_y / sum_c e_c) moves by 20 S_ERR through delta S
    (sum_c |dL/dS_c| = 10 * 2 (1 - s_y) <= 20), by (12 + 12 + 21 + 1) u through exp / sum / division into the log, and by 2 u |L| (logf, the
    coefficient).  The accumulation: `trips` serial adds per lane, a 6-level wave tree, 4 waves, one same-address atomic per workgroup."""
    groups = 2 * ((P + 63) // 64)
    blocks = min(2048, (groups + 3) // 4)
    chain = math.ceil(groups / (4 * blocks)) + 6 + 4 + blocks
    return SAFETY * float((weight * (20 * S_ERR + 46 * U32 + 2 * U32 * L.abs())).sum() + chain * U32 * (weight * L.abs()).sum())


def sampling_rule(yn, sim, rkn=None, flags=None):
    """contrast_train.py:302-331 restated on integers (numpy): per class with len >= 2 the random half (the len // 2 smallest keys, or the
    pixels a host draw flagged) and the similarity rank band [int(0.6 len) - len // 2, int(0.6 len)), ties ordered by pixel index;
    weight = selections / (2 (len // 2) C), C = classes present."""
    P = len(yn)
    ref = np.zeros(P)
    present = np.unique(yn)
    for c in present:
        idx = np.nonzero(yn == c)[0]                          # ascending pixel index: a stable sort keeps it among equal keys
        n = len(idx)
        if n < 2:
            continue
        half, kk = n // 2, int(n * 0.6)
        unit = 1.0 / (2 * half * len(present))
        if flags is None:
            ref[idx[np.argsort(rkn[idx], kind="stable")[:half]]] += unit
        else:
            ref[idx[flags[idx] != 0]] += unit
        ref[idx[np.argsort(sim[idx], kind="stable")[kk - half:kk]]] += unit
    return ref


def rand_flags_rule(yn, rng):
    """the reference's host draws of one view (contrast_train.py:291 / :316) as per-pixel flags: P unused draws of 10-of-21, then per present
    class (ascending) with n >= 2 members a sample of n // 2 member positions"""
    P = len(yn)
    for _ in range(P):
        rng.sample(range(21), 10)
    flags = np.zeros(P, dtype=np.uint8)
    for c in np.unique(yn).tolist():
        idx = np.nonzero(yn == c)[0]
        if len(idx) < 2:
            continue
        flags[idx[np.asarray(rng.sample(range(len(idx)), len(idx) // 2), dtype=np.int64)]] = 1
    return flags


# ================================================================================================ part 2: the stages
class Arith:
    """dt: the arithmetic; own: the stage takes its decisions itself and its results are stored (run_chain); defects: planted wiring defects;
    mode: fp32 | bf16x3 | bf16 (what the record pass and the store of d_head do)."""
    def __init__(self, dt=F64, own=False, defects=(), mode="fp32"):
        self.dt, self.own, self.defects, self.mode = dt, own, frozenset(defects), mode

    def has(self, d):
        return d in self.defects

    def coef(self, x):
        """a coefficient as a kernel holds it: an f32 argument (the float64 chain of the pin keeps it exact)"""
        return x if self.own and self.dt == F64 else float(torch.tensor(x, dtype=torch.float32))


NPIX = 128 * 128
CAND_K = 32


def k_ecr():
    return int(21 * NPIX * 0.2)


def _lab(r):
    return _label_full(r["label20"])                           # [N, 21] float64


def _up(low, S, dt):
    return F.interpolate(low.to(dt), size=(S, S), mode="bilinear", align_corners=True)


def _select_chain(n):
    gs = max(1, min(32, (n + 8191) // 8192))
    per_thread = (math.ceil(n / (4 * gs * 256)) * 4) if n % 4 == 0 else math.ceil(n / (gs * 256))
    return per_thread + 6 + 4 + gs                # serial per thread, wave tree, 4 waves, same-address atomics of the workgroups


def _finish(res, k, relu, scale):
    """select_finish of res rows {thr, sum, count beyond, count equal}: scale * sum_rows (s + (k - cs) t); -> (value, sum |terms|)"""
    t = res[:, 0].clamp_min(0) if relu else res[:, 0]
    return scale * (res[:, 1] + (k - res[:, 2]) * t).sum(), scale * (res[:, 1].abs() + (k - res[:, 2]).abs() * t.abs()).sum()


# ---- per view: plane statistics
def st_stats(A, r, v):
    """up_plane_stats of cam_low (every plane) and of rvd (labelled planes and bg only: the others keep the initial keys, sum 0 and index -1).
    max / min under the stored positions within ubar (one bilinear sample); a position other than float64's is a near-tie within 2 ubar; the
    sum within its accumulation chain plus every sample's ubar (test_up_plane_stats)."""
    N, S, h, w = r["N"], v["S"], v["h"], v["w"]
    planes, out, info = N * 21, {}, dict(differs=0, bad=0)
    for which, key in (("cam", "cam_low"), ("rv", "rvd")):
        low = v[key]
        U = _up(low, S, A.dt).reshape(planes, -1)
        R = U.clamp_min(0)
        live = torch.ones(planes, dtype=torch.bool) if which == "cam" or A.has("st_rv_unmasked") else _lab(r).view(-1) > 0
        if A.own:
            imx, imn = R.argmax(1), R.argmin(1)
        else:
            imx, imn = v[which + "_imx"], v[which + "_imn"]
            ok = (imx[live] >= 0) & (imx[live] < S * S) & (imn[live] >= 0) & (imn[live] < S * S)
            info["bad"] += int((~ok).sum()) + int(((imx[~live] != -1) | (imn[~live] != -1)).sum())
            imx, imn = imx.clamp(0, S * S - 1), imn.clamp(0, S * S - 1)
        rows = torch.arange(planes)
        zero = torch.zeros((), dtype=A.dt)
        vmx, vmn, sm = torch.where(live, R[rows, imx], zero), torch.where(live, R[rows, imn], zero), torch.where(live, U.sum(1), zero)
        ubar = _interp_bar(h, w, float(low.abs().max()))
        chunks = max(1, min(min(16, S // 16), max(1, 4096 // planes)))
        sbar = torch.where(live, SAFETY * (_stats_chain(S, chunks) + 1) * U32 * U.abs().sum(1).double() + S * S * ubar, zero.double())
        vbar = torch.where(live, torch.full((), ubar, dtype=F64), zero.double())
        if not A.own:
            dmx, dmn = (vmx < R.max(1).values) & live, (vmn > R.min(1).values) & live
            info["differs"] += int(dmx.sum() + dmn.sum())
            info["bad"] += int(((vmx < R.max(1).values - 2 * ubar) & live).sum() + ((vmn > R.min(1).values + 2 * ubar) & live).sum())
        neg = torch.full((planes,), -1, dtype=torch.long)
        out.update({which + "_max": (vmx, vbar), which + "_min": (vmn, vbar), which + "_sum": (sm, sbar),
                    which + "_imx": (torch.where(live, imx, neg), None), which + "_imn": (torch.where(live, imn, neg), None)})
    return out, info


# ---- per view: classification loss
def _cls(z, y, N, npix, coef):
    """multilabel soft margin over z [N, 20] and its gradient per hi-res pixel, with the bars of test_cls_loss"""
    terms = F.binary_cross_entropy_with_logits(z, y.to(z.dtype), reduction="none")
    loss = terms.sum() / (20 * N)
    sg = torch.sigmoid(z)
    bias = coef * (sg - y.to(z.dtype)) / (20 * N) / npix
    z64, t64, s64 = z.double(), terms.double(), sg.double()
    l1p = torch.log1p(torch.exp(-z64.abs()))
    term_err = (U32 * (z64.abs() + 8 * (t64 + l1p))).sum()
    lbar = SAFETY * (float(term_err) + 11 * U32 * float(t64.sum())) / (20 * N) + SAFETY * 2 * U32 * float(loss)
    bbar = SAFETY * coef / (20 * N * npix) * (U32 * (z64.abs() * s64 * (1 - s64) + 4 * s64) + 4 * U32 * (s64 - y.double()).abs() + 2.0 ** -126)
    return loss, lbar, bias, bbar


def st_cls(A, r, v):
    """cls_loss: z = plane sum / npix (the GAP of the upsampled CAM), loss into acc[0], bias[n, c] = 0.5 dloss/dz / npix (c = 0: exactly 0)"""
    N, npix = r["N"], v["S"] * v["S"]
    z = (v["cam_sum"].to(A.dt).view(N, 21) / npix)[:, 1:]
    loss, lbar, bias, bbar = _cls(z, r["label20"], N, npix, 0.5)
    zc = torch.zeros(N, 1, dtype=A.dt)
    return {"bias": (torch.cat([zc, bias], 1).view(-1), torch.cat([zc.double(), bbar], 1).view(-1)), "cls_sum": (loss, lbar)}, {}


# ---- per view: min-pool values, selection, sum
def st_q(A, r, v):
    """up_rvmin_values: q = max over the labelled fg classes of the upsampled rvd, argc the first arg channel (test_up_rvmin_values...)"""
    N, S = r["N"], v["S"]
    U = _up(v["rvd"], S, A.dt).view(N, 21, S * S)
    lab = _lab(r).to(A.dt)
    # (only labelled planes are evaluated: an absent class never takes the arg channel; every image of the cases has a class, and rvd >= 0)
    prod = torch.where(lab[:, 1:, None] > 0, U[:, 1:], torch.full((), float("-inf"), dtype=A.dt))
    info = {}
    if A.own:
        ak = prod.argmax(1) + 1
    else:
        ak = v["argc"]
        ubar = _interp_bar(v["h"], v["w"], float(v["rvd"].abs().max()))
        bad = (ak < 1) | (ak > 20)
        ak = ak.clamp(1, 20)
        at = torch.gather(prod, 1, (ak - 1)[:, None]).squeeze(1)
        info = dict(differs=int((at < prod.max(1).values).sum()), bad=int(bad.sum()) + int((at < prod.max(1).values - 2 * ubar).sum()))
    q = torch.gather(prod, 1, (ak - 1)[:, None]).squeeze(1)
    return {"q": (q, torch.full_like(q, _interp_bar(v["h"], v["w"], float(v["rvd"].abs().max())), dtype=F64)), "argc": (ak, None)}, info


def st_minpool(A, r, v):
    """select_kth(q, k_min, smallest, relu) + select_finish(relu, 0.5 / (k_min N)): threshold and counts exact on the stored q, the sum within
    its chain (test_select_kth_and_finish); the view's share of acc[1]"""
    N, n = r["N"], v["S"] * v["S"]
    k = n // 4
    thr, s, cs, ce, sabs = _select_ref(v["q"].to(A.dt).double(), k, False, False, True)
    res = torch.stack([thr, s.to(A.dt).double() if A.own else s, cs, ce], 1)
    chain = _select_chain(n)
    zero = torch.zeros(N, dtype=F64)
    rbar = torch.stack([zero, SAFETY * chain * U32 * sabs, zero, zero], 1)
    coef = 0.5 / k if A.has("minpool_coef_without_N") else 0.5 / (k * N)
    stored = res if A.own else v["res_min"]
    val, mag = _finish(stored, k, not A.has("minpool_finish_without_relu"), coef)
    fbar = SAFETY * (N + 5) * U32 * float(mag)     # the finish loop on the STORED rows: 3 roundings per row, a chain of N adds, the scale and the atomic
    return {"res_min": (res, rbar), "minpool_sum": (val, fbar)}, {}


# ---- per view: max-norm + 128 x 128 resize
def st_norm(A, r, v):
    """up_norm_resize_forward of cam_low -> c and of rvd -> r under the stored arg-max / arg-min positions: max_norm moves by 3 ubar / D plus
    3 roundings, the second resize adds its own sample error; unlabelled planes exactly 0 (test_up_norm_resize_forward)"""
    N, S, h, w = r["N"], v["S"], v["h"], v["w"]
    lab = _lab(r).view(-1)
    out = {}
    for which, key, tag in (("cam", "cam_low", "c"), ("rv", "rvd", "r")):
        low = v[key]
        U = _up(low, S, A.dt).reshape(N * 21, -1)
        imx, imn = v[which + "_imx"].clamp(0, S * S - 1), v[which + "_imn"].clamp(0, S * S - 1)
        An = _max_norm_inj(U, imx, imn).view(1, N * 21, S, S)
        ref = (F.interpolate(An, size=(128, 128), mode="bilinear", align_corners=True)[0] * lab.to(A.dt)[:, None, None]).view(N, 21, 128, 128)
        R = U.double().clamp_min(0)
        D = R.max(1).values - R.min(1).values + 1e-5
        ubar = _interp_bar(h, w, float(low.abs().max()))
        bar = ((SAFETY * (3 * ubar / D + 3 * U32) + _interp_bar(S, S, 1.0)) * lab).view(N, 21, 1, 1).expand(N, 21, 128, 128)
        out[tag] = (ref, bar)
    return out, {}


# ---- per view: features, 16 x 16 rvd, pseudo-labels, prototypes
def st_F(A, r, v):
    """rows_resize_forward: head rows [:, :128] of the view -> F [N 256, 128] (test_rows_resize_forward_and_head_grad_fused)"""
    N, h, w = r["N"], v["h"], v["w"]
    x = v["head"][:, :128].to(A.dt).view(N, h, w, 128).permute(0, 3, 1, 2)
    ref = F.interpolate(x, size=(16, 16), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).reshape(-1, 128)
    return {"F": (ref, torch.full(ref.shape, _interp_bar(h, w, float(v["head"][:, :128].abs().max())), dtype=F64))}, {}


def st_R(A, r, v):
    """the 16 x 16 rvd: rvd itself when the map is 16 x 16 already (bit-equal), else resize_planar_fwd (test_resize_planar_fwd_and_bwd)"""
    N, h, w = r["N"], v["h"], v["w"]
    if A.has("pseudo_from_unresized_rvd"):
        return {"R": (v["rvd"].reshape(-1)[:N * 21 * 256].view(N, 21, 16, 16).clone(), None)}, {}
    if (h, w) == (16, 16):
        return {"R": (v["rvd"].clone(), torch.zeros(N, 21, 16, 16, dtype=F64))}, {}
    M = float(v["rvd"].abs().max())
    ref = F.interpolate(v["rvd"].to(A.dt), size=(16, 16), mode="bilinear", align_corners=True)
    return {"R": (ref, torch.full(ref.shape, SAFETY * (2.0 * _coord_bar(max(h, w)) * 2.0 * M + 6.0 * U32 * M), dtype=F64))}, {}


def _ncam(R, bg, dt, f32_rule):
    """pseudo_label's normalised CAM of R [N, 21, 256]; the zeroing decision v < mn + 1e-5 as the kernel takes it in f32 (one IEEE add and a
    compare on stored f32 values) when f32_rule, else in dt; -> ncam, zero decisions, bar (test_pseudo_label)"""
    v32 = R.float().clamp_min(0)
    mn32 = v32.min(2, keepdim=True).values
    vv = R.to(dt).clamp_min(0)
    mx, mn = vv.max(2, keepdim=True).values, vv.min(2, keepdim=True).values
    zero = (v32 < (mn32 + torch.tensor(1e-5, dtype=torch.float32))) if f32_rule else (vv < mn + 1e-5)
    D = mx - mn + 1e-5
    ref = (torch.where(zero, torch.zeros((), dtype=dt), vv) - mn - 1e-5) / D
    ref[:, 0] = bg
    v64, mx64, mn64, D64 = vv.double(), mx.double(), mn.double(), D.double()
    bar = SAFETY * (2 * U32 * (v64 + mn64 + 1e-5) / D64 + ref.double().abs() * (2 * U32 * (mx64 + mn64 + 1e-5) / D64 + 2 * U32))
    return ref, zero, bar


def st_pseudo(A, r, v):
    """pseudo_label: ncam (the zeroing decision reproduced in f32; one that differs from float64's is a near-tie of the threshold) and y, the
    first arg-max of the STORED scores ncam * label exactly; a label other than float64's is a near-tie within 2 max bar"""
    N = r["N"]
    R = v["R"].view(N, 21, 256)
    exact = A.own and A.dt == F64
    ref, zero, bar = _ncam(R, r["bg"], A.dt, not exact)
    lab = _lab(r)
    info = {}
    if A.own:
        y = (ref.to(A.dt).double() if not exact else ref) * lab[:, :, None]
        y = torch.from_numpy(np.argmax(y.numpy(), axis=1)).long().view(-1)
    else:
        y = torch.from_numpy(np.argmax((v["ncam"] * lab[:, :, None]).numpy(), axis=1)).long().view(-1)
        ref64, zero64, _b = _ncam(R, r["bg"], F64, False)
        diff = zero != zero64
        v64 = R.clamp_min(0)
        mn = v64.min(2, keepdim=True).values
        nz_bad = int(((v64 - mn - 1e-5).abs()[diff] > SAFETY * 2 * U32 * (mn + 1e-5).expand_as(v64)[diff]).sum())
        s64 = ref64 * lab[:, :, None]
        at = torch.gather(s64, 1, v["y"].view(N, 1, 256).clamp(0, 20)).squeeze(1)
        ydiff = v["y"].view(N, 256) != torch.from_numpy(np.argmax(s64.numpy(), axis=1))
        y_bad = int(((at < s64.max(1).values - 2 * float(bar.max())) & ~diff.any(1)).sum())
        info = dict(differs=int(diff.sum()) + int(ydiff.sum()), bad=nz_bad + y_bad, near=int(ydiff.sum()), of=N * 256)
    return {"ncam": (ref, bar), "y": (y, None)}, info


def st_protos(A, r, v):
    """proto_candidates (exact: the top-32 of the stored ncam row, lowest index first; constant rows take the tie table) and proto_merge at
    world 1 (weighted mean + normalise of the stored candidates, _proto_bar)"""
    N, K = r["N"], CAND_K
    rows = v["ncam"].view(N, 21, 256).transpose(0, 1).reshape(21, -1)
    const = rows.max(1).values == rows.min(1).values
    idx = torch.argsort(rows, dim=1, descending=True, stable=True)[:, :K]
    idx[const] = r["tie"].long()
    cv, cf = torch.gather(rows, 1, idx), v["F"][idx]
    scv, scf = (cv, cf) if A.own else (v["cv"], v["cf"])
    if A.dt == F64:
        pr = _protos64(scv, scf)
    else:
        a, f = scv.to(A.dt), scf.to(A.dt)
        pr = F.normalize((a[:, :, None] * f).sum(1) / a.sum(1, keepdim=True), dim=-1)
    srt = torch.sort(rows, dim=1, descending=True).values
    nbar = float(_ncam(v["R"].view(N, 21, 256), r["bg"], F64, False)[2].max())
    info = dict(near=int((((srt[:, K - 1] - srt[:, K]) <= 2 * nbar) & ~const).sum()), of=21)
    z = lambda t: torch.zeros(t.shape, dtype=F64)
    return {"cv": (cv, z(cv)), "cf": (cf, z(cf)), "cc": (const.long(), None), "protos": (pr, _proto_bar(scv, scf, K))}, info


# ---- across views: ER / ECR
def _onehot(c):
    """cam with channel 0 = 1 - max fg, then max_onehot over the fg channels (every tied maximum kept) — on the stored values, exact"""
    x = c.clone()
    mx = x[:, 1:].max(1, keepdim=True).values
    x[:, 0] = 1.0 - mx[:, 0]
    x[:, 1:] = torch.where(x[:, 1:] == mx, x[:, 1:], torch.zeros((), dtype=x.dtype))
    return x


def st_prep(A, r):
    """er_ecr_prep: Gc = +- sign(c1 - c2) f32(er_coef) (bit-equal; channel 0 exactly 0), dlt1 = r1 - onehot(c2), dlt2 = r2 - onehot(c1) — one
    rounding of 1 - max (u) and one of the subtraction (u |dlt|) — and the ER sum: per term one rounding of a - b, then 20 adds per pixel, the
    block tree (6 + 4) and one same-address atomic per block (test_er_ecr_prep_select_and_backward)"""
    N = r["N"]
    v1, v2 = r["views"]
    dt = A.dt
    c1, c2, r1, r2 = (t.to(dt).view(N, 21, NPIX) for t in (v1["c"], v2["c"], v1["r"], v2["r"]))
    er_coef = 1.0 / (N * NPIX) if A.has("er_coef_without_20") else 1.0 / (N * 20 * NPIX)
    terms = (c1 - c2)[:, 1:].abs()
    er = terms.sum()
    ebar = SAFETY * (20 + 10 + N * NPIX // 256 + 1) * U32 * float(terms.double().sum())
    g = torch.sign(c1 - c2).double() * A.coef(er_coef)
    g[:, 0] = 0.0
    oh1, oh2 = _onehot(c1), _onehot(c2)
    if A.has("dlt_directions_swapped"):
        oh1, oh2 = oh2, oh1
    d1, d2 = r1 - oh2, r2 - oh1
    dlt = torch.cat([d1.reshape(N, -1), d2.reshape(N, -1)])
    dbar = SAFETY * U32 * (1.0 + dlt.double().abs())
    z = torch.zeros(g.shape, dtype=F64)
    return {"Gc1": (g.view(N, 21, 128, 128), z.view(N, 21, 128, 128)), "Gc2": ((-g + 0.0).view(N, 21, 128, 128), z.view(N, 21, 128, 128)),
            "dlt": (dlt, dbar), "er_sum": (er, ebar)}, {}


def st_ecr(A, r):
    """the 2N-row ECR selection: select_kth(dlt, K_ecr = int(21 npix 0.2), largest |.|) exact threshold and counts on the stored dlt, the sum
    within its chain, and select_finish with 1 / (N K_ecr) into acc[3]"""
    N, n = r["N"], 21 * NPIX
    K = round(21 * NPIX * 0.2) if A.has("k_ecr_rounded") else k_ecr()
    thr, s, cs, ce, sabs = _select_ref(r["dlt"].to(A.dt).double(), K, True, True, False)
    res = torch.stack([thr, s.to(A.dt).double() if A.own else s, cs, ce], 1)
    zero = torch.zeros(2 * N, dtype=F64)
    rbar = torch.stack([zero, SAFETY * _select_chain(n) * U32 * sabs, zero, zero], 1)
    coef = 1.0 / (N * K)
    val, mag = _finish(res if A.own else r["res_ecr"], K, False, coef)
    return {"res_ecr": (res, rbar), "ecr_sum": (val, SAFETY * (2 * N + 5) * U32 * float(mag))}, {}


def st_Gr(A, r):
    """ecr_backward: +- f32(coef) on the strict members (bit-equal), the remainder (K - cs) / ce shared by the ties at the threshold (2
    roundings), exactly 0 elsewhere"""
    N, K = r["N"], k_ecr()
    dlt, res = r["dlt"], r["res_ecr"]
    c32 = A.coef(1.0 / (N * K))
    a, thr = dlt.abs(), res[:, 0:1]
    share = (K - res[:, 2:3]) / res[:, 3:4].clamp_min(1)
    g = torch.sign(dlt) * torch.where(a > thr, torch.ones((), dtype=F64), torch.where(a == thr, share, torch.zeros((), dtype=F64))) * c32
    return {"Gr": (g.to(A.dt).view(2 * N, 21, 128, 128), (SAFETY * 2 * U32 * g.abs() * (a == thr)).view(2 * N, 21, 128, 128))}, {}


# ---- back, per view
def _maps_backward(A, G, low, imx, imn, lab, bias, sel, h, w, S):
    """up_maps_backward in A.dt autograd under the stored max / min / top-k decisions, with the per-cell bar of test_up_maps_backward:
    every hi-res term reaches a cell through one LDS atomic; a cell takes <= (2S/h + 3)(2S/w + 3) hi-res pixels, each from <= (2 OS/S + 3)^2
    outputs, plus 2 * chunks route / flush atomics and the 8-level A / B trees.  Weights carry the coordinate error (_coord_bar per axis, both
    resizes), and max / min / every gated sample the ubar of the U they were read from (relative ubar / D on invD and on av).
    sel: None or (q, argc, res_min, k, coef)."""
    dt, OS = A.dt, 128
    N = lab.shape[0]
    L21 = lab.view(-1)
    x = low.to(dt).reshape(N * 21, h, w).clone().requires_grad_(True)
    U = F.interpolate(x[None], size=(S, S), mode="bilinear", align_corners=True)[0].reshape(N * 21, S * S)
    total = torch.zeros((), dtype=dt)
    abs_hi = torch.zeros(N * 21, S * S, dtype=F64)
    ubar = _interp_bar(h, w, float(low.abs().max()))
    norm_hi = None
    if G is not None:
        ls = torch.nonzero(L21 != 0).view(-1)
        An = _max_norm_inj(U[ls], imx[ls], imn[ls]).view(1, -1, S, S)
        out = F.interpolate(An, size=(OS, OS), mode="bilinear", align_corners=True)[0]
        Gl = G.to(dt).reshape(N * 21, OS, OS)[ls]
        total = total + (out * Gl).sum()
        Rl = U[ls].detach().double().clamp_min(0)
        rows = torch.arange(len(ls))
        D = Rl[rows, imx[ls]] - Rl[rows, imn[ls]] + 1e-5
        # (a plane that is <= 0 at its arg-max is relu'd to 0 everywhere: the gate passes nothing and the norm term reaches it with exactly 0)
        alive = (Rl[rows, imx[ls]] > 0).double()[:, None]
        gabs = _resize_bwd64(Gl.double().abs(), S, S, True).view(len(ls), -1) * alive
        norm_hi = torch.zeros(N * 21, S * S, dtype=F64)
        norm_hi[ls] = gabs / D[:, None]
        # the max / min routes: |At| + |At - Bt| <= 2 sum |t|, scattered from the arg-max / arg-min pixels
        route = 2 * gabs.sum(1) / D
        norm_hi[ls, imx[ls]] += route
        norm_hi[ls, imn[ls]] += route
        abs_hi += norm_hi
        relD = torch.zeros(N * 21, dtype=F64)
        relD[ls] = 3 * ubar / D                               # per plane (the kernel test takes the smallest D of all planes: its maps are positive)
        # the gate of max_norm, relu(U) - mn - e > 0, is a decision per hi-res pixel that is not stored, and the gradient jumps by G / D across
        # it (the kernel test draws positive maps, where no pixel is near the gate; a CAM that changes sign has a contour of them).  With the
        # sample and the minimum's sample each within ubar of float64's, a pixel is undecided when the gate's sign differs between the two
        # ends of that interval (U <= -ubar is relu'd to exactly 0 on both sides: decided).  Either decision is accepted: the pixel's whole
        # term |G| / D, and its share 2 |G| / D of the max / min routes, go into the bar of the cells they reach.
        Ul = U[ls].detach().double()
        Umin = Ul[rows, imn[ls]][:, None]
        lower = (Ul - ubar).clamp_min(0) - (Umin + ubar).clamp_min(0) - 1e-5
        upper = (Ul + ubar).clamp_min(0) - (Umin - ubar).clamp_min(0) - 1e-5
        flip = ((lower <= 0) & (upper > 0)).double() * gabs / D[:, None]
        flip_hi = torch.zeros(N * 21, S * S, dtype=F64)
        flip_hi[ls] = flip
        flip_hi[ls, imx[ls]] += 2 * flip.sum(1)
        flip_hi[ls, imn[ls]] += 2 * flip.sum(1)
    if bias is not None:
        total = total + (U * bias.to(dt)[:, None]).sum()
        abs_hi += bias.double().abs()[:, None]
    if sel is not None:
        qk, ak, rk, k, coef = sel
        thr, cs, ce = rk[:, 0:1], rk[:, 2:3], rk[:, 3:4]
        wsel = torch.where(qk < thr, 1.0, torch.where(qk == thr, (k - cs) / ce.clamp_min(1), 0.0)) * (qk > 0)
        for c in range(1, 21):
            m = (ak == c).double() * wsel * coef * lab[:, c:c + 1]
            total = total + (m.to(dt) * U.view(N, 21, S * S)[:, c]).sum()
            abs_hi.view(N, 21, -1)[:, c] += m.abs()
    total.backward()
    chunks = max(1, min(64, S * S // 2048))
    chain = (2 * S / h + 3) * (2 * S / w + 3) * (2 * OS / S + 3) ** 2 + 2 * chunks + 16 + OS * OS / (256 * chunks)
    cell_abs = _resize_bwd64(abs_hi.view(N * 21, S, S), h, w, True)
    rel = chain * U32 + 2 * (_coord_bar(max(h, w)) + _coord_bar(S))
    bar = SAFETY * rel * cell_abs
    if norm_hi is not None:
        bar = bar + SAFETY * relD[:, None, None] * _resize_bwd64(norm_hi.view(N * 21, S, S), h, w, True) + _resize_bwd64(flip_hi.view(N * 21, S, S), h, w, True)
    return x.grad.view(N, 21, h, w), bar.view(N, 21, h, w)


def st_d_cam_low(A, r, v):
    """d_cam_low = up_maps_backward(Gc, cam_low, st_cam, bias, adjoint-ones vectors): the ER term through max_norm + resize on the labelled
    planes and the GAP bias of the classification loss on every plane"""
    S = v["S"]
    imx, imn = v["cam_imx"].clamp(0, S * S - 1), v["cam_imn"].clamp(0, S * S - 1)
    ref, bar = _maps_backward(A, v["Gc"], v["cam_low"], imx, imn, _lab(r), None if A.has("no_bias_in_d_cam_low") else v["bias"], None, v["h"], v["w"], S)
    return {"d_cam_low": (ref, bar)}, {}


def st_d_rvd(A, r, v, i):
    """d_rvd = up_maps_backward(Gr of THIS view — rows [iN, (i + 1)N) of the 2N-row Gr —, rvd, st_rv, q, argc, res_min, k_min,
    0.5 / (k_min N)): the ECR term and the min-pool selection"""
    N, S = r["N"], v["S"]
    j = 1 - i if A.has("Gr_halves_swapped") else i
    G = r["Gr"][j * N:(j + 1) * N]
    k = S * S // 4
    imx, imn = v["rv_imx"].clamp(0, S * S - 1), v["rv_imn"].clamp(0, S * S - 1)
    ref, bar = _maps_backward(A, G, v["rvd"], imx, imn, _lab(r), None, (v["q"], v["argc"], v["res_min"], k, 0.5 / (k * N)), v["h"], v["w"], S)
    return {"d_rvd": (ref, bar)}, {}


# ---- NCE
def _fn(Fm, dt):
    x = Fm.to(dt)
    return x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)


def st_rec(A, r):
    """nce_records: per view {label bits, similarity of the pixel to the prototype of its own label, random key}: labels and keys exact, the
    similarity within S_BAR (+ S_SPLIT in the split-bf16 record pass of the bf16 / bf16x3 modes)"""
    out = {}
    split = A.own and A.mode != "fp32" and A.dt == torch.float32      # the emulation of the split record pass: operands x = hi + lo in bf16
    sp = (lambda t: t.bfloat16().float() + (t - t.bfloat16().float()).bfloat16().float()) if split else (lambda t: t)
    for i, v in enumerate(r["views"]):
        s = (sp(_fn(v["F"], A.dt)) * sp(v["protos"].to(A.dt))[v["y"]]).sum(1)
        bar = S_BAR + (S_SPLIT if A.mode != "fp32" else 0.0)
        out[f"sim.v{i}"] = (s, torch.full(s.shape, bar, dtype=F64))
        out[f"rec_y.v{i}"] = (v["y"].clone(), None)
        if v.get("rkey") is not None:
            out[f"rec_key.v{i}"] = (v["rkey"].clone(), torch.zeros(s.shape, dtype=F64))
    return out, {}


def st_weights(A, r, v, i):
    """hard-pixel weights from the STORED records: the global-key rule (intra_weights_global at world 1, scale 1) or the RNG-parity rule
    (intra_weights with host flags); an integer rule, exact up to the kernel's one f32 division (rtol 1e-6, test_intra_weights...)"""
    yn, sim = v["y"].numpy(), r[f"sim.v{i}"].numpy()
    if v.get("flags") is not None:
        ref = sampling_rule(yn, sim, flags=v["flags"].numpy())
    else:
        ref = sampling_rule(yn, sim, rkn=v["rkey"].numpy())
    ref = torch.from_numpy(ref)
    return {"w_intra": (ref, 1e-6 * ref)}, {}


def st_nce(A, r):
    """nce_fused: dF of both views and the three sums (_nce_reference, _nce_sum_bar).  Undecided pixels (rank band) are left out of dF; in the
    intra sum each of them may sit on the other side of one boundary pair per boundary: a2 then changes by e(S_a) - e(S_b) with
    |S_a - S_b| < 2 S_BAR, i.e. L by at most 10 * 2 S_BAR per boundary, 40 S_BAR for both — added to that sum's bar with the pixel's weight."""
    v1, v2 = r["views"]
    P = v1["F"].shape[0]
    cc, ci = 0.1 / (2 * P), NCE_CI
    if A.has("coef_intra_cross_exchanged"):
        cc, ci = ci, cc
    V = [dict(F=v["F"], p=v["protos"], y=v["y"], w=v["w_intra"]) for v in (v1, v2)]
    if A.has("own_other_protos_swapped"):
        V[0]["p"], V[1]["p"] = V[1]["p"], V[0]["p"]
    if A.has("w_intra_of_view1_for_view2"):
        V[1]["w"] = V[0]["w"]
    ref = _nce_reference(V, cc, ci, True, A.dt)
    out, info = {}, dict(left_out=[float(x["undecided"].double().mean()) for x in ref])
    for i, x in enumerate(ref):
        keep = (~x["undecided"])[:, None].expand(P, 128)
        out[f"dF.v{i}"] = (x["dF"], torch.where(keep, x["dF_bar"].double(), torch.full((), float("inf"), dtype=F64)) if not A.own else None)
    for k, tag in enumerate(("cross_sum", "cross2_sum", "intra_sum")):
        wts = [torch.full((P,), cc, dtype=F64) if k < 2 else ci * v["w"].double() for v in V]
        val = sum((w_.to(A.dt) * x["L"][k]).sum() for w_, x in zip(wts, ref))
        Lk = torch.cat([x["L"][k].double() for x in ref])
        bar = _nce_sum_bar(Lk, torch.cat(wts), P)
        if k == 2:
            bar += float(sum((w_ * x["undecided"].double()).sum() for w_, x in zip(wts, ref))) * 40 * S_BAR
        out[tag] = (val, bar)
    return out, info


# ---- last
def _ulp_bf16(x):
    """one bf16 ulp of a float64 value (a result stored in bf16)"""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)


def st_d_head(A, r):
    """head_grad_fused per view at the view's row offset: columns [0, 128) the adjoint of the rows resize of dF gated by head > 0, columns
    [128, 149) d_cam_low of the pixel (a copy, rounded to the store format), the rest 0 (test_rows_resize_forward_and_head_grad_fused); stored
    in bf16 in bf16 mode: one bf16 ulp more"""
    N = r["N"]
    ref = torch.zeros(r["M"], HEAD_LD, dtype=A.dt)
    bar = torch.zeros(r["M"], HEAD_LD, dtype=F64)
    bf = A.mode == "bf16"
    for i, v in enumerate(r["views"]):
        h, w = v["h"], v["w"]
        n, off = N * h * w, (0 if A.has("d_head_view2_at_offset_0") else v["off"])
        dF = v["dF"]
        dF4 = dF.to(A.dt).view(N, 16, 16, 128).permute(0, 3, 1, 2)
        xg = torch.zeros(N, 128, h, w, dtype=A.dt, requires_grad=True)
        (F.interpolate(xg, size=(16, 16), mode="bilinear", align_corners=True) * dF4).sum().backward()
        xa = torch.zeros(N, 128, h, w, dtype=F64, requires_grad=True)
        (F.interpolate(xa, size=(16, 16), mode="bilinear", align_corners=True) * dF4.double().abs()).sum().backward()
        T2 = xa.grad.permute(0, 2, 3, 1).reshape(-1, 128)
        mask = v["head"][:, :128] > 0
        g = torch.where(mask, xg.grad.permute(0, 2, 3, 1).reshape(-1, 128), torch.zeros((), dtype=A.dt))
        nx, ny = math.ceil(2 * 16 / w) + 3, math.ceil(2 * 16 / h) + 3
        b = SAFETY * ((2 * _coord_bar(max(h, w)) + 4 * U32) * nx * ny * float(dF.abs().max()) + (nx * ny + 2) * U32 * T2)
        if bf:
            b = b + _ulp_bf16(g.double())
        dc = (v["d_rvd"] if A.has("d_rvd_into_head_grad") else v["d_cam_low"]).permute(0, 2, 3, 1).reshape(-1, 21)
        dc = dc.float().bfloat16().double() if bf else dc
        ref[off:off + n, :128], ref[off:off + n, 128:149] = g, dc.to(A.dt)
        bar[off:off + n, :128] = torch.where(mask, b, torch.zeros((), dtype=F64))
    return {"d_head": (ref, bar)}, {}


ACC_SLOTS = ("cls_sum", "minpool_sum", "er_sum", "ecr_sum", "cross_sum", "cross2_sum", "intra_sum")


def st_out8(A, r):
    """loss_finish on the stored acc: cls = 0.5 acc0 + acc1, er = acc2 er_coef, ecr = acc3, nce = acc4 + acc5 + acc6; a handful of roundings"""
    a = r["acc"].to(A.dt)
    er_coef = 1.0 / (r["N"] * 20 * NPIX)
    cls, er, ecr, nce = a[0] * 0.5 + a[1], a[2] * er_coef, a[3], a[4] + a[5] + a[6]
    out = torch.stack([cls + er + ecr + nce, cls, er, ecr, nce, a[6], a[4], a[5]])
    mag = float(a[:7].double().abs().sum())
    bar = torch.tensor([6, 2, 2, 0, 2, 0, 0, 0], dtype=F64) * SAFETY * U32 * mag
    return {"out8": (out, bar)}, {}


# ------------------------------------------------------------------------------------------------ chain and judge
ROW_ORDER = ["stats", "cls", "q", "minpool", "norm", "F", "R", "pseudo", "protos", "prep", "ecr", "Gr", "d_cam_low", "d_rvd", "rec", "weights",
             "nce", "d_head", "acc", "out8"]
VIEW_ROWS = {"stats": st_stats, "cls": st_cls, "q": st_q, "minpool": st_minpool, "norm": st_norm, "F": st_F, "R": st_R, "pseudo": st_pseudo,
             "protos": st_protos, "d_cam_low": st_d_cam_low}
GLOBAL_ROWS = {"prep": st_prep, "ecr": st_ecr, "Gr": st_Gr, "rec": st_rec, "nce": st_nce, "d_head": st_d_head, "out8": st_out8}
SCALAR_OF = {"cls_sum": 0, "minpool_sum": 1, "er_sum": 2, "ecr_sum": 3, "cross_sum": 4, "cross2_sum": 5, "intra_sum": 6}
GLOBAL_TO_VIEW = {"Gc1": (0, "Gc"), "Gc2": (1, "Gc"), "dF.v0": (0, "dF"), "dF.v1": (1, "dF")}


def _stage(A, r, row):
    """[(view index or None, {key: (value, bar)}, info)] of one row"""
    if row in VIEW_ROWS:
        return [(i, *VIEW_ROWS[row](A, r, v)) for i, v in enumerate(r["views"])]
    if row == "d_rvd":
        return [(i, *st_d_rvd(A, r, v, i)) for i, v in enumerate(r["views"])]
    if row == "weights":
        return [(i, *st_weights(A, r, v, i)) for i, v in enumerate(r["views"])]
    return [(None, *GLOBAL_ROWS[row](A, r))]


def _get(r, i, key):
    if i is not None:
        return r["views"][i].get(key)
    if key in GLOBAL_TO_VIEW:
        j, k = GLOBAL_TO_VIEW[key]
        return r["views"][j].get(k)
    return r.get(key)


def _put(r, i, key, val):
    if i is not None:
        r["views"][i][key] = val
    elif key in GLOBAL_TO_VIEW:
        j, k = GLOBAL_TO_VIEW[key]
        r["views"][j][k] = val
    else:
        r[key] = val


def copy_record(r):
    """a record whose stages can be run again without touching r (the tensors are shared: no stage writes in place)"""
    out = dict(r)
    out["views"] = [dict(v) for v in r["views"]]
    out["acc_parts"] = dict(r.get("acc_parts", {}))
    return out


def run_chain(r, dt=F64, mode="fp32", defects=(), rng=None, start=None):
    """runs every stage on the record's inputs (N, label20, bg, tie, M, views[i]: S, h, w, off, cam_low, rvd, head, and rkey or — with rng — the
    RNG-parity flags; views[i]["w_inject"] replaces the weights the stage computes), stores what each stage stores, rounded to dt (d_head to
    bf16 in bf16 mode), and accumulates acc like the kernels do.  start: the first row to run, on a record that holds the rows before it."""
    A = Arith(dt, True, defects, mode)
    rnd = lambda t: t.to(dt).double() if t.is_floating_point() else t
    parts = r.setdefault("acc_parts", {})
    for row in ROW_ORDER[ROW_ORDER.index(start) if start else 0:]:
        if row == "acc":
            acc = torch.zeros(8, dtype=F64)
            for (key, _i), val in parts.items():
                acc[SCALAR_OF[key]] += val
            r["acc"] = acc.to(dt).double()
            continue
        if row == "weights" and rng is not None:
            for v in r["views"]:                              # view 1 fully before view 2 (the RNG order of the reference)
                v["flags"] = torch.from_numpy(rand_flags_rule(v["y"].numpy(), rng))
        for i, vals, _info in _stage(A, r, row):
            for key, (val, _bar) in vals.items():
                if key in SCALAR_OF:
                    parts[(key, i)] = float(val)
                    continue
                val = val.detach()
                if key == "d_head" and mode == "bf16":
                    val = val.float().bfloat16().double()
                if key == "w_intra" and "w_inject" in r["views"][i]:
                    val = r["views"][i]["w_inject"]
                _put(r, i, key, rnd(val))
    return r


def judge(r, mode="fp32", only=None, table=None):
    """[(tag, elements, worst err / bar, ok, decisions differing, share left out)] — every stored element of every stage against float64 computed
    from the stored inputs of that stage"""
    A = Arith(F64, False, (), mode)
    table = [] if table is None else table
    for row in ROW_ORDER:
        if only is not None and row not in only:
            continue
        if row == "acc":
            continue                                           # (the slots are judged in the rows of the stages that add to them)
        sums = {}
        for i, vals, info in _stage(A, r, row):
            sfx = "" if i is None else f".v{i}"
            first = True
            for key, (ref, bar) in vals.items():
                if key in SCALAR_OF:
                    s = sums.setdefault(key, [0.0, 0.0])
                    s[0] += float(ref); s[1] += float(bar)
                    continue
                got = _get(r, i, key)
                left = 0.0
                if bar is None:                               # a decision or an exact copy
                    ok = got is not None and got.shape == ref.shape and bool((got == ref).all())
                    ratio = 0.0 if ok else float("inf")
                else:
                    err = (got.double() - ref.double()).abs()
                    fin = torch.isfinite(bar)
                    left = 1.0 - float(fin.double().mean())
                    err, bar_ = err[fin], bar[fin]
                    ok = bool((err <= bar_).all()) and bool(torch.isfinite(got.double()).all())
                    ratio = float((err / bar_.clamp_min(1e-300)).max()) if err.numel() else 0.0
                    ratio = ratio if bool((err[bar_ == 0] == 0).all()) else float("inf")
                differs, bad = (info.get("differs", 0), info.get("bad", 0)) if first else (0, 0)
                ok = ok and left <= NCE_MAX_EXCLUDED + 1e-12     # no stage is judged on under 98 % of its elements
                table.append((f"{row}:{key}{sfx}", int(ref.numel()), ratio, ok and bad == 0, differs, left))
                first = False
        for key, (ref, bar) in sums.items():                  # an acc slot: the sum of what the views / launches add, plus the atomics' roundings
            got = float(r["acc"][SCALAR_OF[key]])
            bar = bar + SAFETY * 2 * U32 * abs(ref)
            ratio = abs(got - ref) / max(bar, 1e-300)
            table.append((f"{row}:acc.{key}", 1, ratio, ratio <= 1.0 and math.isfinite(got), 0, 0.0))
    return table


def row_of(tag):
    return tag.split(":")[0]


def worst(table):
    out = {}
    for tag, _n, ratio, _ok, _d, _l in table:
        k = tag.split(".v")[0]
        if k not in out or ratio > out[k][0]:
            out[k] = (ratio, tag)
    return out


def conditions(r):
    """what the inputs of a case must satisfy for the judgement to cover at least 98 % of every stage: shares of undecided rank-band pixels per
    view, pseudo-label and top-32 near-ties, and whether the ECR / min-pool thresholds are exact ties (count at the threshold > 1).  An ECR
    threshold of exactly 0 is no tie of values: with few classes labelled, fewer than 20 % of a sample's entries are non-zero at all (unlabelled
    planes are exactly 0 in both maps), the threshold falls among those zeros and their gradient is sign(0) = 0 whatever their share."""
    out = dict(undecided=[], label_near=[], top32_near=[], minpool_ties=[], ecr_zero_thr=int((r["res_ecr"][:, 0] == 0).sum()),
               ecr_ties=int(((r["res_ecr"][:, 3] > 1) & (r["res_ecr"][:, 0] != 0)).sum()))
    V = [dict(F=v["F"], p=v["protos"], y=v["y"], w=v["w_intra"]) for v in r["views"]]
    ref = _nce_reference(V, 0.1 / (2 * V[0]["F"].shape[0]), NCE_CI, False)
    A = Arith()
    for v, x in zip(r["views"], ref):
        out["undecided"].append(float(x["undecided"].double().mean()))
        s64 = _ncam(v["R"].view(r["N"], 21, 256), r["bg"], F64, False)
        sc = s64[0] * _lab(r)[:, :, None]
        top2 = torch.topk(sc, 2, dim=1).values
        out["label_near"].append(float(((top2[:, 0] - top2[:, 1]) <= 2 * float(s64[2].max())).double().mean()))
        out["top32_near"].append(st_protos(A, r, v)[1]["near"] / 21)
        out["minpool_ties"].append(int((v["res_min"][:, 3] > 1).sum()))
    return out
