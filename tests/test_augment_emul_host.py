"""CPU: what tests/test_gpu_augment_kernels.py feeds the kernels of csrc/augment.hip, judged without a GPU.
  1. the numpy restatement of the kernel arithmetic (tests/augment_emul.py) equals Pillow on those very inputs — all 2^24 colours in both
     HSV directions, every blend factor, the contrast batch, the resize batch;
  2. each named wrong variant (fused blend, float hue, float fmod, truncating hsv2rgb, mean without + 0.5, luminance without + 0x8000)
     changes at least one output on them, so the GPU comparison against Pillow would notice it (the counts are printed: pytest -s);
  3. every input condition the GPU tests rely on holds, computed from Pillow alone."""
import numpy as np
import pytest

from tests import augment_emul as E


def _n_px(diff):
    return int(diff.any(axis=-1).sum())


@pytest.fixture(scope="module")
def tables():
    """Pillow's and the restatement's conversion of all 2^24 colours, both directions, as tables indexed by colour_index"""
    ac = E.all_colours()
    flat = ac.reshape(-1, 3)
    return dict(pil_hsv=E.pil_rgb2hsv(ac).reshape(-1, 3), pil_rgb=E.pil_hsv2rgb(ac).reshape(-1, 3),
                hsv={v: E.chunked(lambda a, v=v: E.emul_rgb2hsv(a, v), flat) for v in (None, "h_float", "fmod_float")},
                rgb={v: E.chunked(lambda a, v=v: E.emul_hsv2rgb(a, v), flat) for v in (None, "hsv_trunc")})


def _shifted(hsv, shift):
    out = hsv.copy()
    out[:, 0] = (out[:, 0].astype(np.int16) + shift) % 256
    return out


def test_hsv_restatement_equals_pillow_on_all_colours_and_the_domain_holds_every_branch(tables):
    hsv = tables["pil_hsv"]
    assert np.array_equal(tables["hsv"][None], hsv)
    assert np.array_equal(tables["rgb"][None], tables["pil_rgb"])
    i = np.floor(hsv[:, 0].astype(np.float64) * 6.0 / 255.0).astype(int)
    coloured = hsv[:, 1] > 0
    sectors = np.bincount(i[coloured], minlength=7)
    greys = np.unique(hsv[(hsv[:, 0] == 0) & (hsv[:, 1] == 0), 2])
    print("pixels per sector i = 0..6", sectors.tolist(), "h == 255", int((hsv[:, 0] == 255).sum()), "grey values", greys.size)
    assert (sectors[:6] > 0).all() and sectors.size == 7 and greys.size == 256
    assert sectors[6] == 0 and hsv[:, 0].max() == 254                # rgb2hsv never gives h = 255 (i == 6): only a shifted hue does


def test_hue_variants_change_outputs_at_every_shift(tables):
    for shift in E.HUE_SHIFTS:
        base = _shifted(tables["pil_hsv"], shift)
        ref = E.pil_hsv2rgb(base.reshape(4096, 4096, 3)).reshape(-1, 3)          # Pillow's hue op on all colours (data.ColorJitter)
        assert np.array_equal(tables["rgb"][None][E.colour_index(base)], ref)
        counts = {}
        for v in ("h_float", "fmod_float"):
            counts[v] = _n_px(tables["rgb"][None][E.colour_index(_shifted(tables["hsv"][v], shift))] != ref)
        counts["hsv_trunc"] = _n_px(tables["rgb"]["hsv_trunc"][E.colour_index(base)] != ref)
        wrapped = int((base[:, 0].astype(int) != tables["pil_hsv"][:, 0].astype(int) + shift).sum())
        print("hue shift", shift, "colours changed by variant", counts, "hues wrapped", wrapped)
        assert all(c > 0 for c in counts.values()), (shift, counts)
        top = int(((base[:, 0] == 255) & (base[:, 1] > 0)).sum())    # hsv2rgb's i == 6, the seventh value of floor(h * 6 / 255)
        print("          coloured pixels at h == 255 after the shift:", top)
        assert top > 0 or shift == 0
        assert wrapped > 0 or shift in (0, 1)                        # (the largest hue is 254: + 1 does not wrap yet)


def test_fuse_search_ranks_the_committed_factors_first():
    ranked = E.fuse_ranked()
    cand, _ = E.fuse_search()
    below, above = [r for r in ranked if r[0] < 1], [r for r in ranked if r[0] > 1]
    print("candidates", cand.size, "fuse-sensitive", sum(1 for _, c in ranked if c > 0))
    print("below 1:", below[:5], "above 1:", above[:5])
    assert tuple(f for f, _ in below[:len(E.FUSE_BELOW)]) == E.FUSE_BELOW
    assert tuple(f for f, _ in above[:len(E.FUSE_ABOVE)]) == E.FUSE_ABOVE
    assert all(np.float32(f) == f for f in E.FUSE_BELOW + E.FUSE_ABOVE) and below[len(E.FUSE_BELOW) - 1][1] > 1000
    plain = {f: int(E.fuse_changed(f).sum()) for f in (0.7, 1.3)}
    print("pairs a fused blend changes at the plain factors", plain)


def test_saturation_on_all_colours():
    ac = E.all_colours()
    flat = ac.reshape(-1, 3)
    lum = E.pil_lum(ac).reshape(-1)
    assert np.array_equal(E.emul_lum(flat), lum)
    n_lum = int((E.emul_lum(flat, "lum_no_round") != lum).sum())
    print("colours whose luminance changes without + 0x8000:", n_lum)
    assert len([f for f in E.SATURATION_FACTORS if f in E.FUSE_BELOW]) >= 2 and len([f for f in E.SATURATION_FACTORS if f in E.FUSE_ABOVE]) >= 2
    lums = {None: lum.astype(np.intp)[:, None], "lum_no_round": E.emul_lum(flat, "lum_no_round").astype(np.intp)[:, None]}
    deg, val = np.mgrid[0:256, 0:256]
    for f in E.SATURATION_FACTORS:
        ref = E.pil_op(ac, 2, f, 0).reshape(-1, 3)
        def run(variant):                                            # blend_u8 as a table over (degenerate, value), looked up per channel
            table = E.emul_blend(deg, val, f, variant if variant == "fused_blend" else None)
            return table[lums[variant if variant == "lum_no_round" else None], flat]
        assert np.array_equal(run(None), ref), f
        fused, nolum = _n_px(run("fused_blend") != ref), _n_px(run("lum_no_round") != ref)
        print("saturation", repr(f), "colours changed by a fused blend", fused, "by luminance without + 0x8000", nolum)
        if f in E.FUSE_BELOW + E.FUSE_ABOVE:
            assert fused > 0, f
        if f != 1.0:
            assert nolum > 0, f


def test_brightness_on_every_value():
    img = E.every_value_image()
    for c in range(3):
        assert np.array_equal(np.unique(img[..., c]), np.arange(256))
    for f in E.BRIGHTNESS_FACTORS:
        ref = E.pil_op(img, 0, f, 0)
        assert np.array_equal(E.emul_blend(0, img, f), ref), f
        over = int((np.float32(f) * img.astype(np.float32) > 255).sum())
        print("brightness", f, "unclipped values above 255:", over, "outputs at 255:", int((ref == 255).sum()))
        assert (over > 0) == (f > 1)
    assert any(f > 1 for f in E.BRIGHTNESS_FACTORS)


def _pil_means(case):
    """[(luminance sum, pixels)] of the current image at each contrast stage, from Pillow"""
    img, out = case["img"], []
    for op, f in zip(case["op"], case["factor"]):
        if op == 1:
            out.append((int(E.pil_lum(img).astype(np.int64).sum()), img.shape[0] * img.shape[1]))
        if op >= 0:
            img = E.pil_op(img, op, f, case["hue_shift"])
    return out


def test_contrast_batch():
    cases = E.contrast_cases()
    by = {c["name"]: c for c in cases}
    assert len(cases) >= 12 and len({c["img"].shape for c in cases}) >= 8
    changed = {v: {} for v in ("fused_blend", "mean_no_half", "lum_no_round")}
    for c in cases:
        ref = E.pil_chain(c["img"], c["op"], c["factor"], c["hue_shift"])
        got, means = E.emul_chain(c["img"], c["op"], c["factor"], c["hue_shift"])
        assert np.array_equal(got, ref), c["name"]
        (s, n), = _pil_means(c)
        assert means == [int(s / n + 0.5)]
        for v in changed:
            changed[v][c["name"]] = _n_px(E.emul_chain(c["img"], c["op"], c["factor"], c["hue_shift"], v)[0] != ref)
        print("contrast", c["name"], c["img"].shape[:2], "op", c["op"], "factor", c["factor"][c["op"].index(1)], "sum", s, "pixels", n, "mean", means[0],
              "pixels changed by variant", {v: changed[v][c["name"]] for v in changed})
        if c["name"] not in ("black", "white"):
            for ch in range(3):
                assert np.array_equal(np.unique(c["img"][..., ch]), np.arange(256)), (c["name"], ch)
    for k in (1, 127, 254):                                            # the means Pillow's Stat sees: exactly k + 0.5, exactly k, just below
        (s, n), = _pil_means(by[f"k{k}_half"]); assert 2 * s == (2 * k + 1) * n
        (s, n), = _pil_means(by[f"k{k}_exact"]); assert s == k * n
        (s, n), = _pil_means(by[f"k{k}_below"]); assert 2 * s == (2 * k + 1) * n - 2
        assert changed["mean_no_half"][f"k{k}_half"] > 0
    (s, n), = _pil_means(by["large_below"]); assert 2 * s == 255 * n - 2 and n > 1024 * 256
    (s, n), = _pil_means(by["large_half"]); assert 2 * s == 201 * n and n > 1024 * 256 and n % 64
    assert changed["mean_no_half"]["large_half"] > 0
    assert {c["op"].index(1) for c in cases} == {0, 1, 2, 3}                                   # contrast in each stage slot
    assert any((c["img"].shape[0] * c["img"].shape[1]) % 64 for c in cases)
    assert not by["black"]["img"].any() and (by["white"]["img"] == 255).all()
    for name, before in (("after_brightness", 0), ("after_hue", 3), ("after_two", 2)):       # the mean is that of the CURRENT image
        c = by[name]
        assert before in c["op"][:c["op"].index(1)]
        (s, n), = _pil_means(c)
        s0 = int(E.pil_lum(c["img"]).astype(np.int64).sum())
        print(name, "mean of the current image", int(s / n + 0.5), "of the uploaded image", int(s0 / n + 0.5))
        assert int(s / n + 0.5) != int(s0 / n + 0.5)
    fused = [c for c in cases if changed["fused_blend"][c["name"]] > 0]
    assert any(c["factor"][c["op"].index(1)] < 1 for c in fused) and any(c["factor"][c["op"].index(1)] > 1 for c in fused)
    assert sum(1 for v in changed["lum_no_round"].values() if v > 0) >= 1


def test_resize_batch():
    from wseg_amd import augment as A
    totals = np.zeros((2, 2), np.int64)
    assert len({c[1] for c in E.RESIZE_CASES}) >= 6 and any(c[1][0] != c[1][1] for c in E.RESIZE_CASES)
    assert any(c[1][1] == 1 for c in E.RESIZE_CASES) and {c[3] for c in E.RESIZE_CASES} >= {"checker", "step"}
    pairs = set()
    for case in E.RESIZE_CASES:
        name, (h, w), (rh, rw), _ = case
        img = E.resize_image(case)
        (xb, xk), (yb, yk) = A.pil_bicubic_coeffs(w, rw), A.pil_bicubic_coeffs(h, rh)
        pairs |= {(w, rw), (h, rh)}
        a1 = E.emul_resize_pass(img, xb, xk, 1)
        tmp = np.clip(a1, 0, 255).astype(np.uint8)
        assert np.array_equal(tmp, E.pil_resize(img, rw, h)), name
        a2 = E.emul_resize_pass(tmp, yb, yk, 0)
        assert np.array_equal(np.clip(a2, 0, 255).astype(np.uint8), E.pil_resize(img, rw, rh)), name
        hit = np.array([[(a1 < 0).sum(), (a1 > 255).sum()], [(a2 < 0).sum(), (a2 > 255).sum()]])
        totals += hit
        print("resize", name, (h, w), "->", (rh, rw), "taps", xk.shape[1], yk.shape[1], "horizontal below 0 / above 255", hit[0].tolist(),
              "vertical", hit[1].tolist())
        if name == "500to448":
            assert xk.shape[1] == 7
        if name == "97to41":
            assert yk.shape[1] == 11
        if name == "identity":                                       # Pillow copies; the coefficients must say the same
            assert np.array_equal(E.pil_resize(img, rw, rh), img)
            for b, k in ((xb, xk), (yb, yk)):
                assert ((k == 1 << 22).sum(axis=1) == 1).all() and ((k != 0).sum(axis=1) == 1).all()
    assert {(500, 448), (500, 768), (160, 768), (375, 576), (500, 500), (97, 41), (3, 7), (5, 3)} <= pairs
    assert (totals > 0).all(), totals                                # each pass clips on both sides


def test_finish_cases_and_the_slicing_reference():
    from wseg_amd import aff_data as D
    from wseg_amd import augment as A
    for crop in E.FINISH_CROPS:
        cases = E.finish_cases(crop)
        kinds = set()
        for c in cases:
            h, w = c["img"].shape[:2]
            kinds.add((h > crop, w > crop, c["img_top"] == max(h - crop, 0), c["img_left"] == max(w - crop, 0),
                       c["cont_top"] == max(crop - h, 0), c["cont_left"] == max(crop - w, 0), c["flip"]))
            assert 0 <= c["img_top"] <= h - c["ch"] and 0 <= c["img_left"] <= w - c["cw"]
            assert 0 <= c["cont_top"] <= crop - c["ch"] and 0 <= c["cont_left"] <= crop - c["cw"]
            for aff, lut in ((False, A.normalize_lut()), (True, D.normalize_lut_f32())):
                assert np.array_equal(E.ref_finish(c["img"], c, crop, lut, aff), E.host_finish(c["img"], c, crop, aff)), (crop, c["name"], aff)
        for flip in (0, 1):
            assert (True, True, False, False, True, True, flip) in kinds and (True, True, True, True, True, True, flip) in kinds     # larger: offsets 0 / max
            assert (False, False, True, True, False, False, flip) in kinds and (False, False, True, True, True, True, flip) in kinds  # smaller
            assert any(k[0] and not k[1] and k[6] == flip for k in kinds) and any(k[1] and not k[0] and k[6] == flip for k in kinds)
        print("finish crop", crop, "cases", [c["name"] for c in cases])
    lut = E.distinct_lut()
    assert np.unique(lut).size == 768 and np.array_equal(lut.astype(np.float64), 1000.0 * np.arange(3)[:, None] + np.arange(256))
    assert (40 * 40) % 256 and D.normalize_lut_f32()[0][0] != 0
