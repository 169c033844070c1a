"""conv_fov's backward at dilation 12 at the kernel level: the data gradient and the weight gradient of the DeepLab head's 3x3 conv through the
C ABI against float64, with the cases, references and DERIVED bars of tests/conv_f64.py (imported, not edited) and the runners of
tests/test_gpu_conv_f64.py.  No launch of the project ran a backward at dilation 12 before the head's training path:
  * 3x3, dilation 12, IC 128 -> OC 256, N = 2 on the maps 5 x 7 (only the centre tap in range), 13 x 16 (one row / four columns of taps) and
    28 x 31 (both sides), on every tile family (data gradient) / tile hint (weight gradient) the planner can choose for the dtype; the
    256-tile data-gradient kernels run on a pack zero-padded to 256 rows (w_rows), as a launch with OC = 128 needs;
  * bf16 256 -> 256 on the two larger maps: the 256x256 weight-gradient kernel with its unit staging, which IC = 128 does not reach;
  * once per dtype at the real 4096 -> 512 on 5 x 7;
  * cls_conv's weight gradient 512 -> 21 from 24 columns of gradient rows 64 wide (OC_dw, ld_dy: what seg_head_backward launches).
Every element is compared; outputs start as NaN (data gradient) or lie in front of a sentinel guard (weight gradient)."""
import pytest

from tests import conv_f64 as X
from tests import test_gpu_conv_f64 as G

pytestmark = pytest.mark.gpu

DIL = 12
MAPS = [(5, 7), (13, 16), (28, 31)]
DGRAD_FAMS = {"bf16": (64, 128, 224, 256), "f32": (64, 128), "x3": (64, 128, 224, 256)}


def _dgrad_cases():
    out = []
    for dt in ("bf16", "f32", "x3"):
        for (h, w) in MAPS:
            c = X._case(f"fov_dgrad_{h}x{w}_{dt}", "dgrad", dt, 2, h, w, 128, 256, 3, 1, DIL, DGRAD_FAMS[dt])
            c.w_rows = 256 if dt != "f32" else 0                  # out_ch = 128: the 256-tile kernels read whole 256-row weight tiles
            out.append(c)
        out.append(X._case(f"fov_dgrad_real_{dt}", "dgrad", dt, 1, 5, 7, 4096, 512, 3, 1, DIL, (0,)))
    return out


def _wgrad_cases():
    out = []
    for dt in ("bf16", "f32", "x3"):
        for (h, w) in MAPS:
            out.append(X._wcase(f"fov_wgrad_{h}x{w}_{dt}", dt, 2, h, w, 128, 256, 3, 1, DIL, (128,), tiny_seg=0 if (h, w) == (5, 7) else None))
        out.append(X._wcase(f"fov_wgrad_real_{dt}", dt, 1, 5, 7, 4096, 512, 3, 1, DIL, (128, 256) if dt == "bf16" else (128,), unit=0, tiny_seg=0))
        for (h, w) in MAPS[:2]:
            out.append(X._wcase(f"cls_wgrad_{h}x{w}_{dt}", dt, 2, h, w, 512, 24, 1, 1, 1, (128,), OC_dw=21, ld_dy=64))
    for (h, w) in MAPS[1:]:
        out.append(X._wcase(f"fov_wgrad_pipe_{h}x{w}", "bf16", 2, h, w, 256, 256, 3, 1, DIL, (256,), unit=1))
    return out


DGRAD_RUNS = [(c, bm) for c in _dgrad_cases() for bm in c.fams]
WGRAD_RUNS = [(c, hint) for c in _wgrad_cases() for hint in c.hints]


@pytest.mark.parametrize("c,bm", DGRAD_RUNS, ids=[f"{c.name}-{bm}" for c, bm in DGRAD_RUNS])
def test_fov_data_gradient_f64(c, bm):
    G._run_conv(G._problem(c), bm)


@pytest.mark.parametrize("c,hint", WGRAD_RUNS, ids=[f"{c.name}-{h}" for c, h in WGRAD_RUNS])
def test_fov_and_cls_weight_gradient_f64(c, hint):
    G.test_wgrad_f64(c, hint)
