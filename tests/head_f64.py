"""Float64 statement of the contrast net's head passes (the part of Engine.run_forward behind the trunk and of Engine.run_backward in front of
it: network/resnet38_contrast.py:31-75), ONE STAGE AT A TIME, with the derived error bar of every stored tensor.  TEST INFRASTRUCTURE, no
tests here: tests/test_head_host.py pins it to oracle/net.py and shows on the CPU what the bars catch, tests/test_gpu_head_stages.py judges
the engine with it.  It also holds the float64 references and bar helpers of the PCM kernels that tests/test_gpu_pcm_head_kernels.py uses.

Written from oracle/net.py::net_forward, pcm and cam_normalize, not from the engine.  On pixel rows [rows(view 1) ++ rows(view 2)], with
fea = relu(bn7(conv6)) . dropout7 and conv4 / conv5 the inputs of b5 / b6 (detached):
  head      [relu(fea W_proj^T) | fea W_fc8^T | 0]                                     192 columns, the last 43 exact zeros
  feat      [relu(conv4 W_f8_3^T) | relu(conv5 W_f8_4^T) | x_s | 0]                    256 columns; x_s: the view's image, bilinear align_corners=True
  cam_low   head's columns 128..148 as planes, cmax = max_hw relu(cam_low)             per view, exact copies
  G         cam_normalize's gate: v = relu(relu(cam) - 1e-5) / (cmax + 1e-5); column 0 = 1 - max_c v, a foreground class below the
            pixel's maximum zeroed, column 21 = 1, columns 22.. = 0
  Fm        feat W_f9^T with W_f9's columns taken in feat's order [f8_3 | f8_4 | x_s] (the parameter's are [x_s | f8_3 | f8_4])
  Fh, nrm   Fm / (|Fm| + 1e-5), |Fm|;     Fb, Gb, Gl (bf16 mode): bf16(Fh), bf16(G), bf16(G - Gb)
  rvd, den  per image out = relu(Fh Fh^T)^T G, den = out[:, 21], rvd = out[:, :21] / (den + 1e-5)
  cam, cam_rv   cam_low / rvd, bilinear align_corners=True to (H, W)                   (not in the stride-8 `lowres` form)
  backward: d_cam_low, dr = the exact adjoints of the two resizes, d_rvd = dr + g_rvd;  DN, dFh = the PCM backward (DN the gradient at
  `out`); dF = the l2norm backward; dW_f9 = dF^T feat with its columns rotated back into the parameter's order; d_feat = (dF W_f9) . (feat > 0);
  dW_f8_3 = d_feat[:, 0:64]^T conv4, dW_f8_4 = d_feat[:, 64:192]^T conv5; d_head_rows = [g_fproj . (head > 0) | d_cam_low | 0];
  dW_fc_proj, dW_fc8 = d_head_rows[:, :128]^T fea, d_head_rows[:, 128:149]^T fea;  D = (d_head_rows W_head) . s7 . dropout7 . (fea > 0), the
  gradient at conv6 before bn7.

One statement, three arithmetics (tests/trunk_f64.py: Ref, Emu, Exact).  A stage is computed from the tensors STORED for its inputs (the
record `r`), so errors do not compound; under Ref it returns (reference, bar) per tensor, under Emu / Exact the tensor.

Bars.  No bar is fitted; each is one the project has derived, with SAFETY as there:
  the convs and weight gradients     tests/conv_f64.py through trunk_f64's arithmetics: K = 4096 (head), 512, 1024, 195 (f9), 192 (the two
                                     data gradients: the launch's K, padding included); weight gradients n = pixels + the plan's splits
  x_s, cam, cam_rv                   f64_bars._interp_bar (+ one bf16 ulp where the value is stored in bf16: test_pcm_xs)
  the resize adjoints                the backward bar of test_resize_planar_fwd_and_bwd; dr + g_rvd: one more rounding
  G                                  test_cam_gate's arithmetic bar under the stored tensor's own kept entries; a kept entry that is no
                                     (near-)maximum, or a zeroed one that is no near-tie below another class, is judged outside
  Fh, nrm, dF                        the l2norm bars of test_l2norm_forward_and_backward
  Fb, Gb, Gl                         the plain roundings, bit for bit; Gb + Gl = G to 2^-17 (test_to_bf16_and_split_bf16)
  rvd, den                           _pcm_fwd_bars (bf16: relu_rel = BF16_RND)
  DN, dFh                            _pcm_bwd_reference's bars with its flip term; the share of pairs inside the gate band is returned
                                     (BAND_CAP).  The engine hands the kernel the rvd / den its forward STORED, so the reference of dFh is the
                                     same formula from those stored values (sum_i (W_ij + W_ji) Fh_i, W = (S > 0) . G DN^T: autograd's
                                     gradient when rvd / den are exact, which the pin shows), not autograd's from a recomputed forward.
  d_head_rows                        exact (test_head_grad_rows): the f32 values, rounded to bf16 where stored so
`defect`: the planted wiring defects of tests/test_head_host.py, meaningful under Emu only."""
import math

import torch
import torch.nn.functional as F

from tests import conv_f64 as X
from tests import trunk_f64 as T
from tests.f64_bars import SAFETY, U32, _coord_bar, _interp_bar

KF = 192                    # PCM feature channels
BAND_CAP = 1e-3             # largest share of (i, j) pairs whose gate may be undecided at sbar
BF16_RND = 2.0 ** -9        # per value the bf16 kernels round (see the docstring of test_gpu_pcm_head_kernels.py)
SPLIT_T = 3.0 * 2.0 ** -17  # the split-precision gate product
HEAD_LD, FEAT_LD, NCLS, NPROJ = 192, 256, 21, 128
HEAD_CONVS = ("fc_proj", "fc8", "f8_3", "f8_4", "f9")


# ------------------------------------------------------------------------------------------------ moved from test_gpu_pcm_head_kernels.py
def _ulp_bf16(x):
    """one bf16 ulp of a float64 value (a result stored in bf16)"""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)


def _pcm_fwd64(Fh, G):
    """one image, float64: Fh [hw,192], G [hw,32] -> rv [21,hw], den [hw], S [hw,hw] (S[i,j])"""
    S = Fh @ Fh.T
    out = torch.relu(S).T @ G                                 # out[j][c] = sum_i relu(S_ij) G_ic (relu: autograd closes the gate at S == 0)
    den = out[:, 21]
    return (out[:, :21] / (den + 1e-5)[:, None]).T, den, S


def _pcm_fwd_bars(Fh, G, hw, relu_rel=0.0):
    """raw error of one image's S, and the bars of rv [21,hw] and den [hw].
    S: a chain of 192 on sum_k |Fh_ik Fh_jk|.  out[j][c] = sum_i relu(S_ij) G_ic (all terms >= 0): relu is 1-Lipschitz, so every
    term moves by <= (eS_ij + relu_rel relu(S_ij)) G_ic, and the i-loop is a chain of hw on out itself.  rv = out / (den + 1e-5):
    the add and the f32 constant 1 u of D each, the division 1 u of rv."""
    rv, den, S = _pcm_fwd64(Fh, G)
    eS = KF * U32 * (Fh.abs() @ Fh.abs().T)
    out = S.clamp_min(0).T @ G
    e_out = (eS + relu_rel * S.clamp_min(0)).T @ G + hw * U32 * out
    D = den + 1e-5
    bar_rv = SAFETY * ((e_out[:, :21] + rv.T.abs() * (e_out[:, 21] + 2 * U32 * D)[:, None]) / D[:, None] + U32 * rv.T.abs()).T
    return rv, den, S, eS, bar_rv, SAFETY * e_out[:, 21]


def _pcm_bwd_reference(Fh, G, g, rv_in, den_in, hw, base, t_chain, t_rel=0.0, w_rel=0.0, with_band=True):
    """One image in float64.  Fh [hw,192], G [hw,32], g = d_cam_rv [21,hw], rv_in / den_in the f32 values handed to the kernel,
    base [hw,192] the dFh the kernel accumulates onto.  Returns the autograd gradient of sum(g * rv) with respect to Fh (G
    constant), its elementwise bar, DN by its formula with its bar, and the number of pairs inside the gate band.

    DN[j][c] = g_jc * (1 / (den_j + 1e-5)): the add, the constant, the division and the product = 4 u;  DN[j][21] = -(sum_c g rv) * inv:
    a chain of 21 and 1 u per product on sum|g rv|, then the same 4 u.
    t_ij = sum_c P_ic Q_jc over the 32 gate channels: a chain of t_chain, + t_rel of sum|P||Q| (the split product), + DN's own error
    and the roundings of the rv / den inputs (u each) through |G|.  W = gate * t (+ w_rel |t| where W is rounded to bf16).
    dFh[j][k] += sum_i W_ij Fh_ik, twice (t_ij and t_ji): each a chain of hw on sum_i |W_ij Fh_ik|, each `+=` 1 u of its result.
    Gate flips: a row i with |S_ij| <= sbar_ij (sbar = SAFETY * 192 u sum_k |Fh_ik Fh_jk|) may be gated either way by the kernel:
    |t_ij| |Fh_ik| from each launch, in float64."""
    x = Fh.clone().requires_grad_(True)
    rv, _, _ = _pcm_fwd64(x, G)
    (rv * g).sum().backward()
    ref = x.grad
    S = Fh @ Fh.T
    gate = S > 0
    gT, rvT = g.T, rv_in.T                                    # [hw,21]
    Dn = (den_in + 1e-5)[:, None]
    grv = (gT * rvT).abs().sum(1, keepdim=True)
    DN = torch.zeros(hw, 32, dtype=torch.float64)
    DN[:, :21] = gT / Dn
    DN[:, 21:22] = -(gT * rvT).sum(1, keepdim=True) / Dn
    eDN = 4 * U32 * DN.abs()
    eDN[:, 21:22] += 22 * U32 * grv / Dn
    e_in = 2 * U32 * DN.abs()                                 # rv_in, den_in = f32(float64 reference): 1 u each
    e_in[:, 21:22] += 2 * U32 * grv / Dn
    t = G @ DN.T                                              # t[i,j] = sum_c G_ic DN_jc
    ta = G.abs() @ DN.abs().T
    e_t = (t_chain * U32 + t_rel) * ta + G.abs() @ (eDN + e_in).T + w_rel * t.abs()
    Fa = Fh.abs()
    if with_band:
        band = S.abs() <= SAFETY * KF * U32 * (Fa @ Fa.T)
    else:                                                     # S exact in f32: no undecided gate
        band = torch.zeros_like(gate)
    sym = lambda M: (M + M.T).T @ Fa                          # [j,k] = sum_i (M_ij + M_ji) |Fh_ik|
    live = (gate | band).double()
    mag = sym(gate.double() * t.abs())
    arith = hw * U32 * mag + sym(live * e_t) + 2 * U32 * (base.abs() + mag)
    flip = sym(band.double() * t.abs())
    return ref, SAFETY * arith + flip, DN, SAFETY * eDN, int(band.sum())


# ------------------------------------------------------------------------------------------------ helpers
def kind(A):
    return "exact" if isinstance(A, T.Exact) else "emu" if isinstance(A, T.Emu) else "ref"


def _pick(A, ref, bar, emu):
    """a stage outside the convs: (ref(), bar(ref)) under Ref, emu() under Emu, ref() under Exact"""
    k = kind(A)
    if k == "emu":
        return emu()
    v = ref()
    return (v, bar(v)) if k == "ref" else v


def _cat(A, parts):
    """column blocks (each what A.out / _pick returned) side by side"""
    if kind(A) == "ref":
        return torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1)
    return torch.cat(parts, 1)


def _zeros(A, rows, cols):
    z = torch.zeros(rows, cols, dtype=torch.float64)
    return (z, z.clone()) if kind(A) == "ref" else z


def _mm(a, b):          # rows [M, K] times the forward weight [OC, K]
    return a[0] @ b[0].T


def _mm_dgrad(a, b):    # dY [M, OC] times the forward weight [OC, IC]
    return a[0] @ b[0]


def _mm_wgrad(a, b):    # x [M, IC], dY [M, OC] -> dW [OC, IC]
    return b[0].T @ a[0]


def view_rows(N, dims):
    """[(row offset, rows, h, w)] per view"""
    out, off = [], 0
    for (h, w) in dims:
        out.append((off, N * h * w, h, w))
        off += N * h * w
    return out


def planes(rows_, N, h, w):
    """pixel rows [N*h*w, C] -> [N, C, h, w]"""
    return rows_.reshape(N, h, w, rows_.shape[1]).permute(0, 3, 1, 2)


def _interp(x, size, align=True):
    return F.interpolate(x, size=size, mode="bilinear", align_corners=align)


def _interp_adj(g, h, w):
    """the exact adjoint of the align_corners=True resize (h, w) -> g's size, in g's dtype"""
    x = torch.zeros(g.shape[0], g.shape[1], h, w, dtype=g.dtype, requires_grad=True)
    (_interp(x, g.shape[2:]) * g).sum().backward()
    return x.grad


def _store_bar(A, ref, bar):
    """a result outside the convs that is stored in the mode's activation format: one bf16 ulp more in bf16 mode"""
    return bar + _ulp_bf16(ref) if A.store == "bf16" else bar


def weights64(params, mode):
    """{name: [OC, IC] float64} of the five head convs as `mode` stores them: bf16 values in bf16 mode, f32 values otherwise.
    params: name -> weight [OC, IC, 1, 1] (the module's parameters, or a state dict's entries)"""
    out = {}
    for name in HEAD_CONVS:
        w = params[name].detach().float().cpu()
        w = w.reshape(w.shape[0], w.shape[1])
        out[name] = (w.bfloat16() if mode == "bf16" else w).double()
    return out


def f9_in_feat_order(w9):
    """W_f9's columns in feat's order [f8_3 | f8_4 | x_s]: column ic of the result is the parameter's column (ic + 3) % 195"""
    return torch.roll(w9, -3, dims=1)


# ------------------------------------------------------------------------------------------------ forward stages
def st_head(A, r, W, defect=None):
    y, e = A.linear(_mm, [r["fea"]], [torch.cat([W["fc_proj"], W["fc8"]])], 4096)
    y = torch.cat([F.relu(y[:, :NPROJ]), y[:, NPROJ:]], 1)
    return {"head": _cat(A, [A.out(y, e), _zeros(A, y.shape[0], HEAD_LD - NPROJ - NCLS)])}


def _x_s(A, r, align=True):
    """the x_s columns of all views: [M, 3]"""
    parts = []
    for x, (h, w) in zip(r["xs"], r["dims"]):
        H, Wd = x.shape[2:]
        ref = lambda: X.rows(_interp(x.double(), (h, w), align))
        bar = lambda v: _store_bar(A, v, torch.full_like(v, _interp_bar(H, Wd, float(x.abs().max()))))
        emu = lambda: X.store(X.rows(_interp(x.float(), (h, w), align)), A.store)
        parts.append(_pick(A, ref, bar, emu))
    if kind(A) == "ref":
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    return torch.cat(parts)


def st_feat(A, r, W, defect=None):
    y3, e3 = A.linear(_mm, [r["conv4"]], [W["f8_3"]], 512)
    y4, e4 = A.linear(_mm, [r["conv5"]], [W["f8_4"]], 1024)
    f3, f4 = A.out(F.relu(y3), e3), A.out(F.relu(y4), e4)
    xs = _x_s(A, r, align=defect != "xs_align_false")
    M = y3.shape[0]
    if defect == "f8_4_at_col0":                              # f8_4 lands on columns 0..127, columns 128..191 stay as allocated
        return {"feat": _cat(A, [f4, _zeros(A, M, 64), xs, _zeros(A, M, FEAT_LD - 195)])}
    return {"feat": _cat(A, [f3, f4, xs, _zeros(A, M, FEAT_LD - 195)])}


def st_cam_low(A, r, W, defect=None):
    N, head, cams, cmaxs = r["N"], r["head"], [], []
    for off, n, h, w in view_rows(N, r["dims"]):
        cam = planes(head[off:off + n, NPROJ:NPROJ + NCLS], N, h, w).contiguous().double()
        cmax = cam.clamp_min(0).flatten(2).amax(2)
        z = torch.zeros(())
        cams.append((cam, z * cam) if kind(A) == "ref" else cam)
        cmaxs.append((cmax, z * cmax) if kind(A) == "ref" else cmax)
    return {"cam_low": cams, "cmax": cmaxs}


def gate_ref(cam, cmax):
    """cam_normalize's arithmetic in float64 from [N,21,hw] and [N,21]: v and test_cam_gate's bar of it.
    v: the subtraction 1 u and its f32 constant u * 1e-5 -> u (d + 2e-5) / m; the denominator's add and constant 2 u, the division 1 u"""
    d = cam.clamp_min(0)
    m = (cmax + 1e-5)[:, :, None]
    v = (d - 1e-5).clamp_min(0) / m
    return v, SAFETY * U32 * ((d + 2e-5) / m + 3 * v)


def _gate_rows(v):
    """[N,21,hw] values -> G rows [N*hw, 32] under the definition's own decisions (a foreground class below the pixel's maximum zeroed)"""
    fg = v[:, 1:]
    fgmax = fg.max(1, keepdim=True).values
    G = torch.zeros(v.shape[0], 32, v.shape[2], dtype=v.dtype)
    G[:, 1:NCLS] = torch.where(fg < fgmax, torch.zeros((), dtype=v.dtype), fg)
    G[:, 0:1] = 1 - fgmax
    G[:, NCLS] = 1
    return G.permute(0, 2, 1).reshape(-1, 32)


def st_G(A, r, W, defect=None, info=None):
    """G of all views.  Under Ref the arithmetic is judged under the stored G's own kept entries (r["G"]); an entry whose decision is not the
    float64 one up to a near-tie gets the bar -1 (outside whatever its value).  info["gate_differs"] counts the kept / zeroed decisions that
    are not float64's."""
    N, parts = r["N"], []
    for (off, n, h, w), cam, cmax in zip(view_rows(N, r["dims"]), r["cam_low"], r["cmax"]):
        cam = cam.flatten(2)
        if kind(A) == "exact":
            parts.append(_gate_rows(gate_ref(cam.double(), cmax.double())[0]))
            continue
        if kind(A) == "emu":
            c32, eps = cam.float(), torch.tensor(1e-5, dtype=torch.float32)
            v = (c32.clamp_min(0) - eps).clamp_min(0) / (cmax.float() + eps)[:, :, None]
            parts.append(_gate_rows(v).double())
            continue
        v, bar = gate_ref(cam.double(), cmax.double())
        got = r["G"][off:off + n].reshape(N, h * w, 32).permute(0, 2, 1).double()
        fg, fbar = v[:, 1:], bar[:, 1:]
        pbar = fbar.max(1, keepdim=True).values               # the pixel's bar: what the f32 maximum may be off by
        fgmax = fg.max(1, keepdim=True).values
        kept = got[:, 1:NCLS] != 0
        top2 = torch.topk(fg, 2, dim=1).values
        others = torch.where(fg == fgmax, top2[:, 1:2].expand_as(fg), fgmax.expand_as(fg))      # the largest value of the other classes
        kept_ok = fg >= (fgmax - 2 * pbar)                    # nothing but a (near-)maximum is kept
        zeroed_ok = (fg <= fbar) | (fg < others) | (fg <= others + 2 * pbar)
        ref, b = torch.zeros_like(got), torch.zeros_like(got)
        ref[:, 1:NCLS] = torch.where(kept, fg, torch.zeros((), dtype=torch.float64))
        b[:, 1:NCLS] = torch.where(kept, fbar, torch.zeros((), dtype=torch.float64))
        b[:, 1:NCLS][torch.where(kept, ~kept_ok, ~zeroed_ok)] = -1.0
        ref[:, 0:1] = 1 - fgmax                               # bg = 1 - fgmax: the maximum off by <= pbar, the subtraction 1 u
        b[:, 0:1] = pbar + SAFETY * U32 * (1 - fgmax).abs()
        ref[:, NCLS] = 1
        if info is not None:
            info["gate_differs"] = info.get("gate_differs", 0) + int((kept != ((fg == fgmax) & (fg > 0))).sum())
            info["gate_entries"] = info.get("gate_entries", 0) + kept.numel()
        parts.append((ref.permute(0, 2, 1).reshape(-1, 32), b.permute(0, 2, 1).reshape(-1, 32)))
    if kind(A) == "ref":
        return {"G": (torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]))}
    return {"G": torch.cat(parts)}


def st_Fm(A, r, W, defect=None):
    w9 = W["f9"] if defect == "f9_no_rotation" else f9_in_feat_order(W["f9"])
    return {"Fm": A.out(*A.linear(_mm, [r["feat"][:, :195]], [w9], 195))}


def l2norm_ref(Fm):
    nr = Fm.norm(dim=1, keepdim=True)
    return Fm / (nr + 1e-5), nr[:, 0]


def st_Fh(A, r, W, defect=None):
    """|F|: a chain of 10 on a sum of squares, halved by the root, + the root: 6 u;  r = 1 / (|F| + 1e-5) 9 u, Fh = F r: 10 u (the test's)"""
    Fm = r["Fm"]
    if kind(A) == "emu":
        x = Fm.float()
        nr = (x * x).sum(1, keepdim=True).sqrt()
        return {"Fh": (x * (1.0 / (nr + torch.tensor(1e-5, dtype=torch.float32)))).double(), "nrm": nr[:, 0].double()}
    y, nr = l2norm_ref(Fm.double())
    if kind(A) == "exact":
        return {"Fh": y, "nrm": nr}
    return {"Fh": (y, SAFETY * 10 * U32 * y.abs()), "nrm": (nr, SAFETY * 6 * U32 * nr)}


def st_Fb(A, r, W, defect=None):
    """bf16 mode only: the plain roundings, bit for bit; the split of G: hi + lo to 2^-17 relative"""
    Fh, G = r["Fh"], r["G"]
    Fb, Gb = Fh.float().bfloat16().double(), G.float().bfloat16().double()
    Gl = (G.float() - Gb.float()).bfloat16().double()
    if kind(A) != "ref":
        return {"Fb": Fb, "Gb": Gb, "Gl": Gl}
    Gb_got = r.get("Gb", Gb).double()
    return {"Fb": (Fb, 0 * Fb), "Gb": (Gb, 0 * Gb), "Gl": (G.double() - Gb_got, 2.0 ** -17 * G.double().abs())}


def _pcm_fwd_emu(Fh, G, bf16):
    S = (Fh @ Fh.T).clamp_min(0)
    if bf16:
        S = S.bfloat16().float()
    out = S.T @ G
    den = out[:, 21]
    return (out[:, :21] / (den + torch.tensor(1e-5, dtype=Fh.dtype))[:, None]).T, den


def st_rvd(A, r, W, defect=None):
    """per view rvd [N,21,h,w], den [N,hw] from the stored Fh / G (bf16 mode: Fb / Gb)"""
    N, bf16 = r["N"], A.store == "bf16"
    Fh, G = (r["Fb"], r["Gb"]) if bf16 else (r["Fh"], r["G"])
    rvds, dens = [], []
    for vi, (off, n, h, w) in enumerate(view_rows(N, r["dims"])):
        hw, rv, dn = h * w, [], []
        goff = 0 if defect == "G_other_view" and vi == 1 else off            # view 2's gate rows read at view 1's offset
        for i in range(N):
            f, g = Fh[off + i * hw: off + (i + 1) * hw], G[goff + i * hw: goff + (i + 1) * hw]
            if kind(A) == "emu":
                a, b = _pcm_fwd_emu(f.float(), g.float(), bf16)
                rv.append(a.double()); dn.append(b.double())
            elif kind(A) == "exact":
                a, b, _S = _pcm_fwd64(f.double(), g.double())
                rv.append(a); dn.append(b)
            else:
                a, b, _S, _eS, ba, bb = _pcm_fwd_bars(f.double(), g.double(), hw, BF16_RND if bf16 else 0.0)
                rv.append((a, ba)); dn.append((b, bb))
        if kind(A) == "ref":
            rvds.append(tuple(torch.stack([x[k] for x in rv]).reshape(N, NCLS, h, w) for k in (0, 1)))
            dens.append(tuple(torch.stack([x[k] for x in dn]) for k in (0, 1)))
        else:
            rvds.append(torch.stack(rv).reshape(N, NCLS, h, w)); dens.append(torch.stack(dn))
    return {"rvd": rvds, "den": dens}


def st_cam(A, r, W, defect=None):
    """cam, cam_rv per view: the stored cam_low / rvd resized to the image's size"""
    out = {"cam": [], "cam_rv": []}
    for x, cam_low, rvd in zip(r["xs"], r["cam_low"], r["rvd"]):
        size = tuple(x.shape[2:])
        for key, low in (("cam", cam_low), ("cam_rv", rvd)):
            ref = lambda: _interp(low.double(), size)
            bar = lambda v: torch.full_like(v, _interp_bar(low.shape[2], low.shape[3], float(low.abs().max())))
            emu = lambda: _interp(low.float(), size).double()
            out[key].append(_pick(A, ref, bar, emu))
    return out


# ------------------------------------------------------------------------------------------------ backward stages
def resize_bwd_bar(g, h, w):
    """the backward bar of test_resize_planar_fwd_and_bwd for d_out = g [.., oh, ow] gathered onto (h, w): at most nx * ny outputs touch an
    input pixel; each term's weights carry |delta f| <= _coord_bar per axis plus 4 roundings, the row / column sums are chains of nx + ny + 2"""
    oh, ow = g.shape[2:]
    nx, ny = math.ceil(2 * ow / w) + 3, math.ceil(2 * oh / h) + 3
    T2 = _interp_adj(g.double().abs(), h, w)
    return SAFETY * ((2.0 * _coord_bar(max(h, w)) + 4.0 * U32) * nx * ny * float(g.abs().max()) + (nx + ny + 4) * U32 * T2)


def st_d_cam_low(A, r, W, defect=None):
    """not `lowres`: d_cam_low, dr = the adjoints of the two resizes at g_cam / g_cam_rv, d_rvd = dr + g_rvd (one f32 add of the stored dr)"""
    out = {"d_cam_low": [], "dr": [], "d_rvd": []}
    for (g_cam, g_cam_rv, _g_fp, g_rvd), (h, w) in zip(r["g"], r["dims"]):
        for key, g in (("d_cam_low", g_cam), ("dr", g_cam_rv)):
            out[key].append(_pick(A, lambda: _interp_adj(g.double(), h, w), lambda v: resize_bwd_bar(g, h, w),
                                  lambda: _interp_adj(g.float(), h, w).double()))
    for i, (_a, _b, _c, g_rvd) in enumerate(r["g"]):
        dr = r["dr"][i] if "dr" in r else (out["dr"][i][0] if kind(A) == "ref" else out["dr"][i])
        out["d_rvd"].append(_pick(A, lambda: dr.double() + g_rvd.double(), lambda v: X.stored_bar(v, SAFETY * U32 * v.abs(), "f32"),
                                  lambda: (dr.float() + g_rvd.float()).double()))
    return out


def pcm_bwd_formula(Fh, G, DN):
    """dFh [hw,192] = sum_i (W_ij + W_ji) Fh_i with W = (S > 0) . t, t_ij = sum_c G_ic DN_jc: the gradient of sum(g rv) at Fh, G constant"""
    Wm = (Fh @ Fh.T > 0).to(Fh.dtype) * (G @ DN.T)
    return (Wm + Wm.T) @ Fh


def _pcm_bwd_emu(Fh, G, Gl, g, rv, den, bf16, no_lo=False):
    """the honest kernel in float32: DN by its formula; bf16 mode: the split gate product t = Gl.DNb + Gb.DNl + Gb.DNb, W rounded to bf16"""
    gT, rvT = g.T, rv.T
    inv = 1.0 / (den + torch.tensor(1e-5, dtype=torch.float32))[:, None]
    DN = torch.zeros(Fh.shape[0], 32)
    DN[:, :NCLS] = gT * inv
    DN[:, NCLS:NCLS + 1] = -(gT * rvT).sum(1, keepdim=True) * inv
    gate = (Fh @ Fh.T > 0).float()
    if not bf16:
        Wm = gate * (G @ DN.T)
        return DN, None, None, (Wm + Wm.T) @ Fh
    DNb, DNl = X.split_bf16(DN)
    t = G @ DNl.T + G @ DNb.T
    if not no_lo:
        t = t + Gl @ DNb.T
    Wm = (gate * t).bfloat16().float()
    return DN, DNb, DNl, (Wm + Wm.T) @ Fh


def st_DN(A, r, W, defect=None, info=None):
    """DN [M,32] and dFh [M,192] (bf16 mode: DNb, DNl too) from the stored Fh, G (bf16: Fb, Gb + Gl), d_rvd, rvd, den; dFh starts from zero.
    info["band"] / info["pairs"]: the pairs inside the gate band / all pairs (BAND_CAP)."""
    N, bf16 = r["N"], A.store == "bf16"
    Fh = r["Fb"] if bf16 else r["Fh"]
    keys = ("DN", "dFh") + (("DNb", "DNl") if bf16 else ())
    acc = {k: [] for k in keys}
    for (off, n, h, w), d_rvd, rvd, den in zip(view_rows(N, r["dims"]), r["d_rvd"], r["rvd"], r["den"]):
        hw = h * w
        for i in range(N):
            sl = slice(off + i * hw, off + (i + 1) * hw)
            g, rv, dn = d_rvd[i].reshape(NCLS, hw), rvd[i].reshape(NCLS, hw), den[i]
            if kind(A) == "emu":
                res = _pcm_bwd_emu(Fh[sl].float(), (r["Gb"] if bf16 else r["G"])[sl].float(), r["Gl"][sl].float() if bf16 else None,
                                   g.float(), rv.float(), dn.float(), bf16, no_lo=defect == "gate_without_lo")
                for k, v in zip(("DN", "DNb", "DNl", "dFh"), res):
                    if k in acc:
                        acc[k].append(v.double())
                continue
            f = Fh[sl].double()
            Gs = (r["Gb"][sl].double() + r["Gl"][sl].double()) if bf16 else r["G"][sl].double()
            if kind(A) == "exact":
                DN = torch.zeros(hw, 32, dtype=torch.float64)
                Dn = (dn.double() + 1e-5)[:, None]
                DN[:, :NCLS] = g.double().T / Dn
                DN[:, NCLS:NCLS + 1] = -(g.double().T * rv.double().T).sum(1, keepdim=True) / Dn
                acc["DN"].append(DN); acc["dFh"].append(pcm_bwd_formula(f, Gs, DN))
                continue
            _auto, bar, DN, bar_dn, nb = _pcm_bwd_reference(f, Gs, g.double(), rv.double(), dn.double(), hw, torch.zeros(hw, KF, dtype=torch.float64),
                                                            **(dict(t_chain=96, t_rel=SPLIT_T, w_rel=BF16_RND) if bf16 else dict(t_chain=32)))
            if info is not None:
                info["band"], info["pairs"] = info.get("band", 0) + nb, info.get("pairs", 0) + hw * hw
            acc["DN"].append((DN, bar_dn)); acc["dFh"].append((pcm_bwd_formula(f, Gs, DN), bar))
            if bf16:                                          # the split of the stored DN: hi the plain rounding, hi + lo to 2^-17
                DNg = r.get("DN", DN)[sl].double()
                hi = DNg.float().bfloat16().double()
                hi_got = r["DNb"][sl].double() if "DNb" in r else hi
                acc["DNb"].append((hi, 0 * hi)); acc["DNl"].append((DNg - hi_got, 2.0 ** -17 * DNg.abs()))
    if kind(A) == "ref":
        return {k: (torch.cat([x[0] for x in v]), torch.cat([x[1] for x in v])) for k, v in acc.items()}
    return {k: torch.cat(v) for k, v in acc.items()}


def st_dF(A, r, W, defect=None):
    """the l2norm backward from the stored Fm, nrm, dFh.  dF = d r - F k, k = dot r r / |F|: 12 u |d| r + 40 u |F| A r^2 / |F|, A = sum |F d|
    (test_l2norm_forward_and_backward), one bf16 ulp more where dF is stored in bf16"""
    Fm, d = r["Fm"], r["dFh"]
    if kind(A) == "emu":
        x, dd, nr = Fm.float(), d.float(), r["nrm"].float()[:, None]
        rr = 1.0 / (nr + torch.tensor(1e-5, dtype=torch.float32))
        k = torch.where(nr > 0, (x * dd).sum(1, keepdim=True) * rr * rr / nr, torch.zeros(()))
        return {"dF": X.store(dd * rr - x * k, A.store)}
    x = Fm.double().clone().requires_grad_(True)
    nr = x.norm(dim=1, keepdim=True)
    ((x / (nr + 1e-5)) * d.double()).sum().backward()
    ref, nr, v, dd = x.grad, nr.detach(), x.detach(), d.double()
    if kind(A) == "exact":
        return {"dF": ref}
    rr = 1.0 / (nr + 1e-5)
    Aa = (v * dd).abs().sum(1, keepdim=True)
    bar = SAFETY * U32 * (12 * dd.abs() * rr + 40 * v.abs() * Aa * rr * rr / nr.clamp_min(1e-300))
    return {"dF": (ref, _store_bar(A, ref, bar))}


def _wg(A, x, dy, splits):
    y, e = A.linear(_mm_wgrad, [x], [dy], x.shape[0], extra=splits)
    return A.out(y, e, "f32")


def _roll_cols(A, o, k):
    return tuple(torch.roll(t, k, dims=1) for t in o) if kind(A) == "ref" else torch.roll(o, k, dims=1)


def st_dW_f9(A, r, W, defect=None):
    """[192, 195] in the parameter's column order [x_s | f8_3 | f8_4]: feat's column ic lands in column (ic + 3) % 195"""
    o = _wg(A, r["feat"][:, :195], r["dF"], r.get("splits", {}).get("f9", 1))
    return {"dW_f9": o if defect == "no_dw_rot" else _roll_cols(A, o, 3)}


def st_d_feat(A, r, W, defect=None):
    """(dF W_f9 in feat's column order) . (feat > 0) on all 256 columns; the columns from 195 on have no weight: exact zeros"""
    y, e = A.linear(_mm_dgrad, [r["dF"]], [f9_in_feat_order(W["f9"])], 192)
    if defect != "d_feat_ungated":
        keep = (r["feat"][:, :195] > 0).to(y.dtype)
        y, e = y * keep, e * keep
    return {"d_feat": _cat(A, [A.out(y, e), _zeros(A, y.shape[0], FEAT_LD - 195)])}


def st_dW_f8_3(A, r, W, defect=None):
    return {"dW_f8_3": _wg(A, r["conv4"], r["d_feat"][:, 0:64], r.get("splits", {}).get("f8_3", 1))}


def st_dW_f8_4(A, r, W, defect=None):
    c0 = 0 if defect == "f8_4_dy_at_col0" else 64
    return {"dW_f8_4": _wg(A, r["conv5"], r["d_feat"][:, c0:c0 + 128], r.get("splits", {}).get("f8_4", 1))}


def st_d_head_rows(A, r, W, defect=None):
    """head_grad_rows: [g_fproj . (head > 0) | d_cam_low | 0], exact; stored in bf16 in bf16 mode (the plain rounding)"""
    N, parts = r["N"], []
    for (off, n, h, w), g, dc in zip(view_rows(N, r["dims"]), r["g"], r["d_cam_low"]):
        gf = X.rows(g[2].double())
        if defect != "head_relu_dropped":
            gf = gf * (r["head"][off:off + n, :NPROJ] > 0)
        parts.append(torch.cat([gf, X.rows(dc.double()), torch.zeros(n, HEAD_LD - NPROJ - NCLS, dtype=torch.float64)], 1))
    v = torch.cat(parts)
    if A.store == "bf16":
        v = v.float().bfloat16().double()
    return {"d_head_rows": (v, 0 * v) if kind(A) == "ref" else v}


def st_dW_fc8(A, r, W, defect=None):
    """one launch over the 149 live columns of d_head_rows: rows 0..127 of the block are fc_proj's, 128..148 fc8's"""
    sp = r.get("splits", {}).get("fc_proj", 1)
    o = _wg(A, r["fea"], r["d_head_rows"][:, :NPROJ + NCLS], sp)
    if defect == "fc_rows_swapped":                           # fc8's 21 rows first
        o = torch.cat([o[NPROJ:], o[:NPROJ]])
    cut = lambda a, b: tuple(t[a:b] for t in o) if kind(A) == "ref" else o[a:b]
    return {"dW_fc_proj": cut(0, NPROJ), "dW_fc8": cut(NPROJ, NPROJ + NCLS)}


def st_D(A, r, W, defect=None):
    """the gradient at conv6 before bn7: (d_head_rows W_head) . s7 . dropout7[image] . (fea > 0); K = the launch's 192 columns"""
    N = r["N"]
    Wh = torch.cat([W["fc_proj"], W["fc8"]])
    y, e = A.linear(_mm_dgrad, [r["d_head_rows"][:, :NPROJ + NCLS]], [Wh], HEAD_LD)
    drop = None if defect == "D_without_dropout7" else r.get("drop7")
    s7 = torch.ones_like(r["s7"]) if defect == "D_without_s7" else r["s7"]
    return {"D": A.out(*T._gate(A, y, e, s7, r["fea"], drop, T.img_index(N, r["dims"]) if drop is not None else None))}


# ------------------------------------------------------------------------------------------------ rows, chain and judge
# (row of the stage table, its function, the tensors it stores; a list-valued tensor is per view)
FWD_ROWS = (("head", st_head, ("head",)), ("feat", st_feat, ("feat",)), ("cam_low", st_cam_low, ("cam_low", "cmax")), ("G", st_G, ("G",)),
            ("Fm", st_Fm, ("Fm",)), ("Fh", st_Fh, ("Fh", "nrm")), ("Fb", st_Fb, ("Fb", "Gb", "Gl")), ("rvd", st_rvd, ("rvd", "den")),
            ("cam", st_cam, ("cam", "cam_rv")))
BWD_ROWS = (("d_cam_low", st_d_cam_low, ("d_cam_low", "dr", "d_rvd")), ("DN", st_DN, ("DN", "DNb", "DNl", "dFh")), ("dF", st_dF, ("dF",)),
            ("dW_f9", st_dW_f9, ("dW_f9",)), ("d_feat", st_d_feat, ("d_feat",)), ("dW_f8_3", st_dW_f8_3, ("dW_f8_3",)),
            ("dW_f8_4", st_dW_f8_4, ("dW_f8_4",)), ("d_head_rows", st_d_head_rows, ("d_head_rows",)),
            ("dW_fc8", st_dW_fc8, ("dW_fc_proj", "dW_fc8")), ("D", st_D, ("D",)))
ROW_FN = {name: fn for name, fn, _t in FWD_ROWS + BWD_ROWS}
ROW_ORDER = [name for name, _fn, _t in FWD_ROWS + BWD_ROWS]


def _rows_of(r, mode, forward, backward):
    """the rows a record has: Fb in bf16 mode only, cam / d_cam_low outside the stride-8 form, d_head_rows where the caller gave gradients"""
    rows_ = []
    for name, fn, tensors in (FWD_ROWS if forward else ()) + (BWD_ROWS if backward else ()):
        if name == "Fb" and mode != "bf16":
            continue
        if name in ("cam", "d_cam_low") and r.get("lowres", True):
            continue
        if name == "d_head_rows" and "g" not in r:
            continue
        rows_.append((name, fn, tensors))
    return rows_


def run_chain(A, r, W, mode, backward=False, defects=None):
    """The head on its own outputs under arithmetic A (Emu or Exact): fills a copy of the record r, which holds the inputs N, dims, xs, fea,
    conv4, conv5, lowres; for the backward s7, drop7 and g [(g_cam, g_cam_rv, g_fproj, g_rvd)] per view (not lowres) or d_rvd [per view] and
    d_head_rows (the fused entry).  defects {row: defect}."""
    r = dict(r)
    for name, fn, _tensors in _rows_of(r, mode, True, backward):
        r.update(fn(A, r, W, defect=(defects or {}).get(name)))
    return r


def judge_tensor(tag, got, ref, bar, table):
    """every element of `got` against (ref, bar): appends (tag, max err, max err / bar, ok) to `table`, prints the line.  An exact stage has
    bar 0 (ratio 0 or inf); a decision outside its rule bar -1 (ratio inf)."""
    got = got.double()
    assert got.shape == ref.shape, (tag, tuple(got.shape), tuple(ref.shape))
    finite = bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    inside = err <= bar
    ratio = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(inside, torch.zeros(()), torch.full((), float("inf")))).double()
    ok = finite and bool(inside.all())
    table.append((tag, float(err.max()) if finite else float("inf"), float(ratio.max()) if finite else float("inf"), ok))
    print(f"{tag:28s} max err {table[-1][1]:.3e}  max err/bar {table[-1][2]:.4f}{'' if ok else '   <-- OUTSIDE'}")
    return ok


def judge(mode, r, W, forward=True, backward=True, table=None, info=None, only=None):
    """Every stored tensor of the record against its stage's float64 reference computed from the record's own stored inputs.  Tags are
    `<tensor>` or `<tensor>.v<view>`.  info: receives the band and gate counts.  only: the rows to judge.  Returns the table."""
    A, table = T.Ref(mode), [] if table is None else table
    for name, fn, tensors in _rows_of(r, mode, forward, backward):
        if only is not None and name not in only:
            continue
        ref = fn(A, r, W, info=info) if fn in (st_G, st_DN) else fn(A, r, W)
        for t in tensors:
            if t not in ref:
                continue
            assert t in r, (name, t)
            if isinstance(ref[t], list):
                for i, (rb, got) in enumerate(zip(ref[t], r[t])):
                    judge_tensor(f"{t}.v{i}", got, *rb, table)
            else:
                judge_tensor(t, r[t], *ref[t], table)
    return table


def row_of(tag):
    t = tag.split(".")[0]
    return next(name for name, _fn, tensors in FWD_ROWS + BWD_ROWS if t in tensors)


def worst(table):
    """{tensor: (worst err / bar, its tag)} of a judge table"""
    out = {}
    for tag, _err, ratio, _ok in table:
        k = tag.split(".")[0]
        if k not in out or ratio > out[k][0]:
            out[k] = (ratio, tag)
    return out
