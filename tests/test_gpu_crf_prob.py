"""crf.crf_inference_from_probs (wseg_crf_update_prob) against the float64 filters of tests/crf_exact.py with a softmax unary — the DeepLab
stage's dense_crf (segmentation/lib/utils/DenseCRF.py): U = -ln(clip(p, 1e-5, 1)) rounded to float32 as pydensecrf's unary_from_softmax
returns it, Gaussian (sxy 3, compat 3), bilateral (sxy 32, srgb 13, compat 10).  The bars are the ones tests/test_gpu_crf.py derives for
the same filters (logit_bar); at t = 0 nothing is filtered and the logits are -U: logf's 1 ulp and the float32 rounding of U.
crf_inference (the label unary) shares the update kernel's body: its result on an existing case is pinned, bit for bit, to what the
library gave before the probability unary was added."""
import hashlib

import numpy as np
import pytest
import torch

from tests import crf_exact as X
from tests.test_gpu_crf import SAFETY, U32, _picture, logit_bar

pytestmark = pytest.mark.gpu

BILATERAL, GAUSSIAN = (32, 13, 10.0), (3, 3.0)
SEEDS = {(24, 40): 5, (40, 56): 1}
# sha256 of the float32 logits, Q and uint8 arg-max bytes of crf_inference on tests/test_gpu_crf.py's 40 x 56 case (bilateral (50, 5, 10), ten
# iterations), recorded on an MI355X from the library of the commit before this entry point existed
CRF_INFERENCE_SHA256 = "3a5ec5bc09998de6c0f816b9d3d1a8d6a42500533a4c56c0df782e98d49682e5"


def _prob(H, W, seed):
    """float32 [21, H, W]: a softmax with a few classes in front, one plane far below the clip (1e-5) and one pixel block of exact zeros"""
    g = torch.Generator().manual_seed(seed)
    lg = 3 * torch.randn(21, H, W, generator=g)
    lg[7] -= 40.0
    p = torch.softmax(lg, 0).float()
    p[3, :4, :4] = 0.0
    return p


def _reference(img, prob, t):
    """float64 mean field of crf_exact's filters from the unary of `prob`: dict(Q, logits, fb, fg) as [21, H, W]"""
    M, H, W = prob.shape
    N = H * W
    fg, fb = X.features(img, GAUSSIAN[0]), X.features(img, BILATERAL[0], BILATERAL[1])
    ng, nb = X.norm(fg), X.norm(fb)
    U = (-torch.log(prob.double().clamp(1e-5, 1.0))).float().double().reshape(M, N).t()      # unary_from_softmax returns float32
    lg = -U
    Q = torch.softmax(lg, 1)
    Fg = Fb = torch.zeros_like(Q)
    for _ in range(t):
        Fg, Fb = X.filt(fg, ng, Q), X.filt(fb, nb, Q)
        lg = -U + GAUSSIAN[1] * Fg + BILATERAL[2] * Fb
        Q = torch.softmax(lg, 1)
    shape = lambda z: z.t().reshape(1, M, H, W)
    return dict(Q=shape(Q), logits=shape(lg), fb=shape(Fb), fg=shape(Fg))


@pytest.mark.parametrize("t", [0, 1])
@pytest.mark.parametrize("size", [(24, 40), (40, 56)])
def test_prob_unary_against_float64(size, t):
    from wseg_amd import crf, synth
    H, W = size
    img = synth.synthetic_rgb_image(H, W, SEEDS[size])
    prob = _prob(H, W, 100 + H)
    ref = _reference(img.numpy(), prob, t)
    Q, logits, amax = crf.crf_inference_from_probs(img.cuda(), prob.cuda(), t=t, return_logits=True, return_argmax=True)
    assert tuple(Q.shape) == (21, H, W) and tuple(amax.shape) == (H, W)
    unary_bar = SAFETY * 3 * U32 * float(ref["logits"].abs().max()) if t == 0 else 0.0
    bar = unary_bar if t == 0 else logit_bar(img, BILATERAL[0], BILATERAL[1], ref, t=t)[0]
    err = float((logits.cpu().double() - ref["logits"][0]).abs().max())
    print(f"{H}x{W} t={t}: max |dlogit| {err:.3e}, bar {bar:.3e}, max |logit| {float(ref['logits'].abs().max()):.2f}")
    assert err <= bar
    if t == 0:
        assert abs(float(ref["logits"].min()) - np.log(1e-5)) < 1e-5              # the clip is reached: no logit below ln 1e-5
        assert abs(float(logits.min()) - np.log(1e-5)) < 1e-5
    assert float((Q.sum(0) - 1).abs().max()) <= 21 * 2 * U32 * SAFETY
    l64 = ref["logits"][0].reshape(21, H * W)
    top2 = torch.topk(l64, 2, 0)[0]
    sure = (top2[0] - top2[1]) >= 2 * max(bar, 1e-6)
    assert float(sure.double().mean()) >= 0.99
    assert bool((amax.cpu().reshape(-1).long()[sure] == l64.argmax(0)[sure]).all())
    if t == 1:
        assert float((l64.argmax(0) != prob.reshape(21, -1).argmax(0)).double().mean()) > 0.005      # the CRF does move labels


def test_defaults_are_the_reference_call():
    import inspect
    from wseg_amd import crf
    sig = inspect.signature(crf.crf_inference_from_probs).parameters
    assert sig["t"].default == 1 and sig["bilateral"].default == (32, 13, 10) and sig["gaussian"].default == (3, 3)
    with pytest.raises(ValueError):
        crf.crf_inference_from_probs(torch.zeros(8, 8, 3, dtype=torch.uint8, device="cuda"), torch.zeros(21, 8, 9, device="cuda"))
    with pytest.raises(ValueError):
        crf.crf_inference_from_probs(torch.zeros(8, 8, 3, dtype=torch.uint8, device="cuda"), torch.zeros(33, 8, 8, device="cuda"))


def crf_inference_digest():
    """sha256 over the bytes of (logits, Q, arg-max) of crf_inference on the 40 x 56 case of tests/test_gpu_crf.py"""
    from wseg_amd import crf
    img, cams = _picture(40, 56)
    lab = crf.labels_from_cams(cams, bg_score=0.26)
    Q, logits, amax = crf.crf_inference(img.cuda(), lab, t=10, bilateral=(50, 5, 10), gaussian=(3, 3), return_logits=True, return_argmax=True)
    h = hashlib.sha256()
    for x in (logits, Q, amax):
        h.update(x.cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def test_crf_inference_is_bit_identical_to_the_library_before():
    assert crf_inference_digest() == CRF_INFERENCE_SHA256
