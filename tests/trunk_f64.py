"""Float64 statement of the trunk (conv1a and the 17 blocks of network/resnet38d.py:160-189), ONE BLOCK AT A TIME and split into the stages the
network definition has, with the derived error bar of every stored tensor.  TEST INFRASTRUCTURE, no tests here: tests/test_trunk_host.py pins
it to oracle/net.py and shows on the CPU what the bars catch, tests/test_gpu_trunk_stages.py judges the engine's trunk with it.

Written from oracle/net.py::res_block / bot_block, not from the engine.  With t = relu(bn_branch2a(x)) the block's input and x the raw one:
  ResBlock     v     = relu(bn_branch2b1(conv_branch2a(t)))
               x_out = conv_branch2b1(v) + (x if the block has no conv_branch1 else conv_branch1(t))
               t_out = relu(bn_next(x_out))          bn_next: the next block's bn_branch2a; behind b7: bn7, times dropout7
  bottleneck   v1 = drop_2b1 . relu(bn_branch2b1(conv_branch2a(t))),  v2 = drop_2b2 . relu(bn_branch2b2(conv_branch2b1(v1))),
               x_out = conv_branch2b2(v2) + conv_branch1(t)
  stem         t_out = relu(bn(conv1a(image))) with b2's bn_branch2a
  backward of a ResBlock from D = dL/dx_out (s_* = the folded BatchNorm scale):
               du = dgrad_2b1(D) . s_2b1 . (v > 0);   dW_2b1 = v^T D,  dW_2a = t^T du,  dW_1 = t^T D
               D_in = [dgrad_2a(du) + dgrad_1(D) + tap] . s_2a . (t > 0)      tap: a gradient w.r.t. t from outside the trunk
               no conv_branch1:  D_in = dgrad_2a(du) . s_2a . (t > 0) + D;      the first trainable block: weight gradients only
  backward of a bottleneck: du2 = dgrad_2b2(D) . s_2b2 . drop_2b2 . (v2 > 0), du1 = dgrad_2b1(du2) . s_2b1 . drop_2b1 . (v1 > 0),
               dW_2b2 = v2^T D, dW_2b1 = v1^T du2, dW_2a = t^T du1, dW_1 = t^T D, D_in = [dgrad_2a(du1) + dgrad_1(D) + tap] . s_2a . (t > 0)
D_in is dL/dx of the block's raw input, the D of the block before it.

One statement, three arithmetics.  Every stage function takes an arithmetic A:
  Ref    float64 next to the error e of the held f32 value: returns (reference, bar) per stored tensor;
  Emu    the honest kernel on the CPU: torch's float32 convolutions (split-bf16: the three products), the epilogue in float32, the store
         rounded as conv_f64.store; returns the stored tensors (as float64 values);
  Exact  float64, nothing rounded: chained on its own outputs it is the network (the pin to oracle.net.backbone).
A stage is computed from the tensors STORED for its inputs (the record `r`: the device's, or in a chain the function's own), so errors do
not compound.  The ReLU / dropout decisions of the backward are the stored activations themselves (exact zeros: no near-tie).

Bars are those of tests/conv_f64.py, composed per launch (SAFETY on every error term, none on the storage rounding):
  held sum       e0 = SAFETY (acc_rel(n) + X3_MISSING) S, S the same product of magnitudes, n = K roundings (split-bf16 3 K), K the WHOLE
                 contraction of the launch that produces the stage: a K-concatenated launch (`fused`) has 9 mid + cin or cin + cout / 2
                 (backward: 9 mid + cout or cout + cout / 4); above N_CHAIN roundings the chain model, as there
  residual       + SAFETY U32 |sum|            (x_out's skip term or raw input, the tap, tmp, the same-shape block's D)
  BN affine      e |scale| + SAFETY U32 (|v scale| + |v scale + shift|);  a scale alone or a dropout factor: one rounding;  ReLU and masks exact
  t_out          from the UNROUNDED x_out: its e starts from the held sum, never from x_out's bar
  weight grads   conv_f64.wgrad_bar: n = pixels + splits (split-bf16 3 pixels + splits, + X3_MISSING), stored as f32; splits: the plan's
  stored         half an ulp of the stored format at |ref| + e (stored_bar)
Where a mode stores the skip conv's output first (the record holds `rpost` / `tmp`), that tensor is a stage of its own and the launch
behind it has K of its own conv alone.
BatchNorm folds: fold64 is the definition in float64, fold_bar the bar of the f32 fold the engine keeps (add, sqrt, divide; multiply,
subtract: at most 5 roundings on the scale, 6 U32 |mean scale| + U32 |shift| on the shift, with SAFETY); a judged fold is then an operand.
`defect`: the planted wiring defects of tests/test_trunk_host.py, meaningful under Emu only."""
import torch
import torch.nn.functional as F

from oracle.net import BN_EPS, _BLOCKS
from tests import conv_f64 as X
from tests.f64_bars import SAFETY, U32

MODES = {"fp32": ("f32", "f32"), "bf16x3": ("x3", "f32"), "bf16": ("bf16", "bf16")}      # mode -> (product arithmetic, storage format)
BLOCKS = {name: (kind, stride, fd, d) for name, kind, stride, fd, d in _BLOCKS}
ORDER = [b[0] for b in _BLOCKS]
FROZEN = ("b2", "b2_1", "b2_2")            # network/resnet38_contrast.py:29 not_training (+ conv1a)
DROP_P = {"b6.dropout_2b1": 0.3, "b6.dropout_2b2": 0.3, "b7.dropout_2b1": 0.5, "b7.dropout_2b2": 0.5, "dropout7": 0.5}   # resnet38d.py:64,68


# ------------------------------------------------------------------------------------------------------------------ arithmetics
class Ref:
    def __init__(self, mode):
        self.dt, self.store = MODES[mode]
        self.dtype, self.u = torch.float64, SAFETY * U32

    def c(self, x):
        return x.to(self.dtype)

    def linear(self, f, a, b, n, extra=0, dt=None):
        """(value, error of the held f32 value) of the bilinear f(a, b) accumulated over n products (+ extra roundings)"""
        x3 = (dt or self.dt) == "x3"
        y = f([self.c(t) for t in a], [self.c(t) for t in b])
        S = f([self.c(t).abs() for t in a], [self.c(t).abs() for t in b])
        return y, SAFETY * (X.acc_rel((3 if x3 else 1) * n + extra) + (X.X3_MISSING if x3 else 0.0)) * S

    def out(self, v, e, store=None):
        return v, X.stored_bar(v, e, store or self.store)


class Emu(Ref):
    def __init__(self, mode):
        super().__init__(mode)
        self.dtype, self.u = torch.float32, 0.0

    def linear(self, f, a, b, n, extra=0, dt=None):
        a, b = [self.c(t) for t in a], [self.c(t) for t in b]
        if (dt or self.dt) != "x3":
            return f(a, b), 0.0
        (ah, al), (bh, bl) = zip(*[X.split_bf16(t) for t in a]), zip(*[X.split_bf16(t) for t in b])
        return f(ah, bh) + f(ah, bl) + f(al, bh), 0.0

    def out(self, v, e, store=None):
        return X.store(v, store or self.store)


class Exact(Ref):
    def __init__(self):
        self.dt = self.store = "f64"
        self.dtype, self.u = torch.float64, 0.0

    def linear(self, f, a, b, n, extra=0, dt=None):
        return f([self.c(t) for t in a], [self.c(t) for t in b]), 0.0

    def out(self, v, e, store=None):
        return v


# ------------------------------------------------------------------------------------------------------------------ rows and maps
def to_maps(r, N, dims):
    """pixel rows [rows of view 1 ++ rows of view 2][C] -> [N, C, h, w] per view"""
    out, off = [], 0
    for (h, w) in dims:
        out.append(r[off:off + N * h * w].reshape(N, h, w, r.shape[1]).permute(0, 3, 1, 2))
        off += N * h * w
    assert off == r.shape[0], (off, tuple(r.shape), dims)
    return out


def to_rows(maps):
    return torch.cat([X.rows(m) for m in maps])


def img_index(N, dims):
    """the row of a [views * N, C] dropout table a pixel row belongs to"""
    return torch.cat([i * N + torch.arange(N).repeat_interleave(h * w) for i, (h, w) in enumerate(dims)])


def out_dims(dims, k, s, d):
    return [(X._osz(h, k, s, d, d * (k // 2)), X._osz(w, k, s, d, d * (k // 2))) for (h, w) in dims]


def block_dims(name, din):
    kind, s, fd, d = BLOCKS[name]
    return out_dims(din, 3, s, fd) if kind == "res" else out_dims(din, 1, s, 1)


def lin_conv(N, specs):
    """f(a, b) = sum_i conv(a[i], b[i]) on rows; specs[i] = (input dims, stride, dilation)"""
    def f(a, b):
        return sum(to_rows([F.conv2d(x, w, None, s, d * (w.shape[-1] // 2), d) for x in to_maps(xr, N, din)])
                   for xr, w, (din, s, d) in zip(a, b, specs))
    return f


def lin_dgrad(N, specs):
    """f(a, b) = sum_i the data gradient of conv b[i] (forward weight [OC, IC, k, k]) at dY = a[i]; specs[i] = (din, dout, stride, dilation)"""
    def f(a, b):
        tot = 0
        for dyr, w, (din, dout, s, d) in zip(a, b, specs):
            k, maps = w.shape[-1], []
            pad = d * (k // 2)
            for dy, (h, w_) in zip(to_maps(dyr, N, dout), din):
                op = [n - ((o - 1) * s - 2 * pad + d * (k - 1) + 1) for n, o in ((h, dy.shape[2]), (w_, dy.shape[3]))]
                maps.append(F.conv_transpose2d(dy, w, None, s, pad, op, 1, d))
            tot = tot + to_rows(maps)
        return tot
    return f


def lin_wgrad(N, din, dout, s, d, wshape):
    """f([x], [dy]) = dW [OC, IC, k, k] summed over the views"""
    def f(a, b):
        return sum(torch.nn.grad.conv2d_weight(x, wshape, dy, s, d * (wshape[-1] // 2), d)
                   for x, dy in zip(to_maps(a[0], N, din), to_maps(b[0], N, dout)))
    return f


# ------------------------------------------------------------------------------------------------------------------ epilogues
def _add(A, v, e, r):
    v = v + A.c(r)
    return v, e + A.u * v.abs()


def _affine(A, v, e, sc, sh, drop=None, img=None):
    """relu(v scale + shift) (. drop): the second output of a forward launch"""
    sc, sh = A.c(sc), A.c(sh)
    vs = v * sc
    x = vs + sh
    e = e * sc.abs() + A.u * (vs.abs() + x.abs())
    x = F.relu(x)
    if drop is not None:
        dr = A.c(drop)[img]
        x = x * dr
        e = e * dr + A.u * x.abs()
    return x, e


def _gate(A, v, e, sc, mask, drop=None, img=None):
    """v . scale (. drop) . (mask > 0): the BN-ReLU backward"""
    sc = A.c(sc)
    x = v * sc
    e = e * sc.abs() + A.u * x.abs()
    if drop is not None:
        dr = A.c(drop)[img]
        x = x * dr
        e = e * dr + A.u * x.abs()
    keep = (mask > 0).to(A.dtype)
    return x * keep, e * keep


# ------------------------------------------------------------------------------------------------------------------ operands
def weights64(params, mode):
    """{conv name: [OC, IC, k, k] float64} of the trunk's convs as `mode` stores them: bf16 values in bf16 mode, f32 values otherwise (the
    split of split-bf16 is arithmetic: X3_MISSING); conv1a is read as f32 in every mode.  params: name -> weight tensor (a state dict's
    `name + ".weight"` entries, or the module's parameters)."""
    out = {}
    for name, w in params.items():
        w = w.detach().float().cpu()
        out[name] = (w.bfloat16() if (mode == "bf16" and name != "conv1a") else w).double()
    return out


def trunk_params(sd):
    """{conv name: weight} of the trunk's convs in a state dict (conv_branch1: where it has one)"""
    return {k[:-len(".weight")]: v for k, v in sd.items() if v.dim() == 4 and (k.startswith("conv1a.") or k.split(".")[0] in BLOCKS)}


def bn_names():
    out = []
    for name in ORDER:
        out += [f"{name}.bn_branch2a", f"{name}.bn_branch2b1"] + ([f"{name}.bn_branch2b2"] if BLOCKS[name][0] == "bot" else [])
    return out + ["bn7"]


def fold64(sd, name):
    """(scale, shift) of BatchNorm `name` in eval mode, float64 from the state dict"""
    g, b, m, v = (sd[f"{name}.{k}"].detach().double().cpu() for k in ("weight", "bias", "running_mean", "running_var"))
    scale = g / torch.sqrt(v + BN_EPS)
    return scale, b - m * scale


def fold32(sd, name):
    """the f32 fold an implementation keeps (the honest emulation)"""
    g, b, m, v = (sd[f"{name}.{k}"].detach().float().cpu() for k in ("weight", "bias", "running_mean", "running_var"))
    scale = g / torch.sqrt(v + BN_EPS)
    return scale, b - m * scale


def fold_bar(sd, name):
    """bars of an f32 fold against fold64: scale = g / sqrt(v + eps): the add (half of it under the root), a root and a quotient of at most
    one ulp = 2 U32 each: 5 U32 |scale| (eps itself is read as f32(1e-5): 2^-25 1e-5 / v of the sum, far below); shift = b - m scale: the
    scale's error times |m|, the product, the difference: 6 U32 |m scale| + U32 |shift|."""
    scale, shift = fold64(sd, name)
    ms = (sd[f"{name}.running_mean"].detach().double().cpu() * scale).abs()
    return SAFETY * 5 * U32 * scale.abs(), SAFETY * U32 * (6 * ms + shift.abs())


def next_bn(name):
    i = ORDER.index(name)
    return ORDER[i + 1] + ".bn_branch2a" if i + 1 < len(ORDER) else "bn7"


def _drop(masks, key):
    return masks.get(key) if masks else None


# ------------------------------------------------------------------------------------------------------------------ forward stages
def stem_forward(A, xs, W, bn):
    """{"t_out"} from the images xs ([N, 3, H, W] per view): an f32 fma chain of 27 products from f32 operands in every mode"""
    N, dims = xs[0].shape[0], [tuple(x.shape[2:]) for x in xs]
    y, e = A.linear(lin_conv(N, [(dims, 1, 1)]), [to_rows(xs)], [W["conv1a"]], 27, dt="f32")
    return {"t_out": A.out(*_affine(A, y, e, *bn["b2.bn_branch2a"]))}


def block_forward(A, name, r, W, bn, masks, N, din, fused=False, defect=None):
    """The forward stages of block `name` from the record r: t, (x: the raw input, a block without conv_branch1), and — when judging — the
    stored inputs of the later launches v / v1, v2, rpost.  fused: the skip conv and the last conv are one K-concatenated launch (no rpost).
    Returns {stage: A.out(..)}: v | v1, v2; rpost (not fused, with a skip conv); x_out; t_out."""
    kind, s, fd, d = BLOCKS[name]
    dout, img, out = block_dims(name, din), None, {}
    w1 = W.get(name + ".conv_branch1")
    nsc, nsh = bn[next_bn(name)]
    ndrop = _drop(masks, "dropout7") if next_bn(name) == "bn7" else None
    if masks:
        img = img_index(N, dout)
    if defect == "short_skip":                      # the last eight input columns of the skip piece are missing
        w1 = w1.clone()
        w1[:, -8:] = 0
    t = r["t"]
    cin = t.shape[1]
    if kind == "res":
        w2a, w2b1 = W[name + ".conv_branch2a"], W[name + ".conv_branch2b1"]
        y, e = A.linear(lin_conv(N, [(din, s, fd)]), [t], [w2a], 9 * cin)
        out["v"] = A.out(*_affine(A, y, e, *bn[name + ".bn_branch2b1"]))
        last, wl, kl, dl = r.get("v", out["v"]), w2b1, 9 * w2b1.shape[1], d
    else:
        w2a, w2b1, wl = (W[f"{name}.conv_branch2{x}"] for x in ("a", "b1", "b2"))
        y, e = A.linear(lin_conv(N, [(din, s, 1)]), [t], [w2a], cin)
        out["v1"] = A.out(*_affine(A, y, e, *bn[name + ".bn_branch2b1"], _drop(masks, name + ".dropout_2b1"), img))
        y, e = A.linear(lin_conv(N, [(dout, 1, d)]), [r.get("v1", out["v1"])], [w2b1], 9 * w2b1.shape[1])
        out["v2"] = A.out(*_affine(A, y, e, *bn[name + ".bn_branch2b2"], _drop(masks, name + ".dropout_2b2"), img))
        last, kl, dl = r.get("v2", out["v2"]), wl.shape[1], 1
    if w1 is None:                                  # same shape: the raw input is the residual
        y, e = A.linear(lin_conv(N, [(dout, 1, dl)]), [last], [wl], kl)
        y, e = _add(A, y, e, r["x"])
    elif fused:
        y, e = A.linear(lin_conv(N, [(dout, 1, dl), (din, s, 1)]), [last, t], [wl, w1], kl + cin)
    else:
        ys, es = A.linear(lin_conv(N, [(din, s, 1)]), [t], [w1], cin)
        out["rpost"] = A.out(ys, es)
        y, e = A.linear(lin_conv(N, [(dout, 1, dl)]), [last], [wl], kl)
        y, e = _add(A, y, e, r.get("rpost", out["rpost"]))
    out["x_out"] = A.out(y, e)
    x, e = _affine(A, y, e, nsc, nsh, ndrop, img)
    if defect == "dropout7_twice":
        x = x * A.c(ndrop)[img]
    out["t_out"] = A.out(x, e)
    return out


# ------------------------------------------------------------------------------------------------------------------ backward stages
def block_backward(A, name, r, W, bn, masks, N, din, fused=False, splits=None, first=False, defect=None):
    """The backward stages of block `name` from the record r: t, v | v1, v2 (the stored activations), D, tap (or absent), and — when judging —
    du | du2, du1, tmp.  splits {stage: atomics per element of that weight gradient} (default 1).  first: the first trainable block, weight
    gradients only.  Returns {stage: A.out(..)}: du | du2, du1; dW_2b2, dW_2b1, dW_2a, dW_1 [OC, IC, k, k]; tmp (not fused, with a skip conv); D_in."""
    kind, s, fd, d = BLOCKS[name]
    dout, out, splits = block_dims(name, din), {}, splits or {}
    img = img_index(N, dout) if masks else None
    w1 = W.get(name + ".conv_branch1")
    t, D, tap = r["t"], r["D"], r.get("tap")
    cout = D.shape[1]
    sa = bn[name + ".bn_branch2a"][0]

    def wg(stage, x, dy, w, xin, st, dil):
        y, e = A.linear(lin_wgrad(N, xin, dout, st, dil, tuple(w.shape)), [x], [dy], dy.shape[0], extra=splits.get(stage, 1))
        out[stage] = A.out(y, e, "f32")

    if kind == "res":
        w2a, w2b1 = W[name + ".conv_branch2a"], W[name + ".conv_branch2b1"]
        s1 = bn[name + ".bn_branch2b1"][0]
        y, e = A.linear(lin_dgrad(N, [(dout, dout, 1, d)]), [D], [w2b1], 9 * cout)
        out["du"] = A.out(*_gate(A, y, e, s1, r["v"]))
        du = r.get("du", out["du"])
        wg("dW_2b1", r["v"], D, w2b1, dout, 1, d)
        dua, fda = du, fd
    else:
        w2a, w2b1, w2b2 = (W[f"{name}.conv_branch2{x}"] for x in ("a", "b1", "b2"))
        s1, s2 = bn[name + ".bn_branch2b1"][0], bn[name + ".bn_branch2b2"][0]
        d1, d2 = _drop(masks, name + ".dropout_2b1"), _drop(masks, name + ".dropout_2b2")
        if defect == "other_dropout":               # the factor of another site of the same width
            d1 = masks[{"b7.dropout_2b1": "b6.dropout_2b2"}[name + ".dropout_2b1"]]
        y, e = A.linear(lin_dgrad(N, [(dout, dout, 1, 1)]), [D], [w2b2], cout)
        out["du2"] = A.out(*_gate(A, y, e, s2, r["v2"], d2, img))
        du2 = r.get("du2", out["du2"])
        y, e = A.linear(lin_dgrad(N, [(dout, dout, 1, d)]), [du2], [w2b1], 9 * du2.shape[1])
        out["du1"] = A.out(*_gate(A, y, e, s1, r["v1"], d1, img))
        wg("dW_2b2", r["v2"], D, w2b2, dout, 1, 1)
        wg("dW_2b1", r["v1"], du2, w2b1, dout, 1, d)
        dua, fda = r.get("du1", out["du1"]), 1
    wg("dW_2a", t, dua, w2a, din, s, fda)
    if w1 is not None:
        wg("dW_1", t, D, w1, din, s, 1)
        if defect == "no_skip_wgrad":
            out["dW_1"] = out["dW_1"] * 0
    if first:
        return out
    ka = w2a.shape[2] * w2a.shape[3] * dua.shape[1]
    mask = r["v"] if defect == "mask_from_v" else t
    if defect == "swap_scale":
        sa = s1
    if w1 is None:
        y, e = A.linear(lin_dgrad(N, [(din, dout, s, fda)]), [dua], [w2a], ka)
        if defect == "residual_before_mask":
            out["D_in"] = A.out(*_gate(A, *_add(A, y, e, D), sa, mask))
        else:
            out["D_in"] = A.out(*_add(A, *_gate(A, y, e, sa, mask), D))
        return out
    late_tap = defect == "tap_after_mask"            # the tap behind mask . scale instead of in front of it
    if fused:
        y, e = A.linear(lin_dgrad(N, [(din, dout, s, fda), (din, dout, s, 1)]), [dua, D], [w2a, w1], ka + cout)
        pre = None if late_tap else tap
    else:
        ys, es = A.linear(lin_dgrad(N, [(din, dout, s, 1)]), [D], [w1], cout)
        if tap is not None and not late_tap:
            ys, es = _add(A, ys, es, tap)
        out["tmp"] = A.out(ys, es)
        y, e = A.linear(lin_dgrad(N, [(din, dout, s, fda)]), [dua], [w2a], ka)
        pre = out["tmp"] if late_tap else r.get("tmp", out["tmp"])
    if pre is not None:
        y, e = _add(A, y, e, pre)
    x, e = _gate(A, y, e, sa, mask)
    if late_tap:
        x, e = _add(A, x, e, tap)
    out["D_in"] = A.out(x, e)
    return out


# ------------------------------------------------------------------------------------------------------------------ chain and judge
def run_chain(A, xs, W, bn, masks, fused=(), D=None, taps=None, frozen=FROZEN):
    """The whole trunk on its own outputs under arithmetic A (Emu or Exact): the record {"stem": {..}, block: {every stored tensor}} a judge
    reads; with D (the gradient at b7's x_out, rows) the backward down to the first block behind `frozen` (a leading run of ORDER) too, taps
    {block: gradient w.r.t. that block's t}."""
    N, dims = xs[0].shape[0], [tuple(x.shape[2:]) for x in xs]
    rec = {"stem": dict(stem_forward(A, xs, W, bn), dims=dims, x=xs)}
    t, x = rec["stem"]["t_out"], None
    for name in ORDER:
        r = dict(t=t, dims=dims)
        if (name + ".conv_branch1") not in W:
            r["x"] = x
        r.update(block_forward(A, name, r, W, bn, masks, N, dims, fused=name in fused))
        rec[name] = r
        t, x, dims = r["t_out"], r["x_out"], block_dims(name, dims)
    if D is None:
        return rec
    for name in reversed(ORDER):
        if name in frozen:
            break
        r = rec[name]
        r["D"] = D
        if taps and name in taps:
            r["tap"] = taps[name]
        first = name == ORDER[len(frozen)]
        r.update(block_backward(A, name, r, W, bn, masks, N, r["dims"], fused=name in fused, first=first))
        D = r.get("D_in")
    return rec


FWD_STAGES = ("v", "v1", "v2", "rpost", "x_out", "t_out")
BWD_STAGES = ("du", "du2", "du1", "tmp", "D_in", "dW_2b2", "dW_2b1", "dW_2a", "dW_1")


def judge_stage(tag, got, ref, bar, table):
    """every element of `got` against (ref, bar): appends (tag, max err, max err / bar, ok) to `table`, prints the line"""
    got = got.double()
    assert got.shape == ref.shape, (tag, tuple(got.shape), tuple(ref.shape))
    finite = bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    ratio = float((err / bar).max()) if finite else float("inf")
    ok = finite and bool((err <= bar).all())
    table.append((tag, float(err.max()) if finite else float("inf"), ratio, ok))
    print(f"{tag:28s} max err {table[-1][1]:.3e}  max err/bar {ratio:.4f}{'' if ok else '   <-- OUTSIDE'}")
    return ok


def judge(mode, rec, W, bn, masks, N, splits=None, backward=True, forward=True, table=None, frozen=FROZEN):
    """Every stored tensor of the record against its stage's float64 reference computed from the record's own stored inputs.
    A block's structure is read off its record: `rpost` / `tmp` present = the skip conv's output was stored first; absent (and a skip conv
    exists) = one K-concatenated launch.  frozen: the net's frozen blocks, the block behind them gets weight gradients only.  Returns the table [(tag, max err, max err / bar, ok)]."""
    A, table = Ref(mode), [] if table is None else table
    if forward and "x" in rec.get("stem", {}):
        ref = stem_forward(A, rec["stem"]["x"], W, bn)
        judge_stage("stem.t_out", rec["stem"]["t_out"], *ref["t_out"], table)
    for name in ORDER:
        r = rec.get(name)
        if r is None:
            continue
        skip = (name + ".conv_branch1") in W
        if forward and "t_out" in r:
            ref = block_forward(A, name, r, W, bn, masks, N, r["dims"], fused=skip and "rpost" not in r)
            for st in FWD_STAGES:
                if st in ref:
                    if st in r:
                        judge_stage(f"{name}.{st}", r[st], *ref[st], table)
                    else:
                        assert st == "x_out", (name, st)           # the one output an implementation may keep to itself
        if backward and "D" in r:
            first = name == ORDER[len(frozen)]
            ref = block_backward(A, name, r, W, bn, masks, N, r["dims"], fused=skip and "tmp" not in r, splits=(splits or {}).get(name),
                                 first=first)
            for st in BWD_STAGES:
                if st in ref:
                    assert st in r, (name, st)
                    judge_stage(f"{name}.{st}", r[st], *ref[st], table)
    return table


def worst(table):
    """{stage kind: (worst err / bar, its tag)} of a judge table"""
    out = {}
    for tag, _err, ratio, _ok in table:
        kind = tag.split(".")[-1]
        if kind not in out or ratio > out[kind][0]:
            out[kind] = (ratio, tag)
    return out
