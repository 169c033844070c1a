"""AffinityNet training data, host side (wseg_amd/data.py aff_train_transform / VOC12AffDataset, wseg_amd/aff_data.py draws, sparse
packing and tables): CPU only."""
import os
import random

import numpy as np
import PIL.Image
import pytest

from tests import aff_data_ref as R

CROP = 64
# (H, W): smaller than the crop in both dimensions, larger in both, and the two mixed cases
SIZES = [(37, 50), (150, 203), (50, 100), (90, 41)]


def _stacks(h, w, seed):
    return R.quantised_stack(h, w, (0, 3, 7), seed), R.quantised_stack(h, w, (0, 3, 12), seed + 1)


def test_draw_aff_params_consumes_random_as_the_host_chain_does():
    """Same seed: the same generator state afterwards, and the host chain's image and label follow from the returned parameters (the jitter
    applied with wseg_amd.data.ColorJitter alone, then placement, float32 normalisation, container flip; the dense label rule)."""
    from wseg_amd import aff_data as D, data as wdata
    from wseg_amd.resnet38_contrast import Normalize
    flips = set()
    for si, (h, w) in enumerate(SIZES * 2):
        img, (la, ha), seed = R.image(h, w, si), _stacks(h, w, 10 * si), 300 + si
        ref_img, ref_label, state = R.host_chain(img, la, ha, seed, CROP)
        random.seed(seed)
        p = D.draw_aff_params(w, h, CROP)
        assert random.getstate() == state, (h, w)
        assert p["ch"] == min(CROP, h) and p["cw"] == min(CROP, w)
        flips.add(p["flip"])
        random.seed(seed)
        jit = np.asarray(wdata.ColorJitter(0.3, 0.3, 0.3, 0.1)(PIL.Image.fromarray(img)))
        cont = np.zeros((CROP, CROP, 3), np.float32)
        cont[p["cont_top"]:p["cont_top"] + p["ch"], p["cont_left"]:p["cont_left"] + p["cw"]] = \
            jit[p["img_top"]:p["img_top"] + p["ch"], p["img_left"]:p["img_left"] + p["cw"]]
        cont = Normalize()(cont)
        if p["flip"]:
            cont = np.fliplr(cont)
        assert ref_img.dtype == np.float32 and ref_img.shape == (3, CROP, CROP)
        assert np.array_equal(ref_img, np.transpose(cont, (2, 0, 1))), (h, w, p)
        assert np.array_equal(ref_label, R.dense_rule(la, ha, p, CROP, np.float32)[0]), (h, w, p)
    assert flips == {0, 1}


def test_pack_scores_is_lossless_drops_zero_planes_and_refuses_negatives():
    from wseg_amd import aff_data as D
    stack = R.quantised_stack(23, 31, (0, 4, 20), 5)
    ids, planes = D.pack_scores(stack)
    assert ids.dtype == np.int32 and ids.tolist() == [0, 4, 20]
    assert planes.dtype == np.float32 and planes.shape == (3, 23, 31) and planes.flags.c_contiguous
    back = np.zeros_like(stack)
    back[ids] = planes
    assert np.array_equal(back, stack)
    stack[0] = 0                                                # plane 0 all zero: not shipped
    assert D.pack_scores(stack)[0].tolist() == [4, 20]
    ids, planes = D.pack_scores(np.zeros((21, 3, 5), np.float32))
    assert ids.shape == (0,) and planes.shape == (0, 3, 5)
    stack[4, 2, 2] = -Q_SMALL
    with pytest.raises(ValueError, match="negative"):
        D.pack_scores(stack)
    with pytest.raises(ValueError):
        D.pack_scores(np.zeros((22, 3, 5), np.float32))


Q_SMALL = 2.0 ** -12


def test_host_label_path_equals_the_dense_restatement():
    """The host chain's label map against the literal restatement of tests/aff_data_ref.py in float32, on quantised scores (every
    summation order gives the same bits), for plane sets that differ between the stacks and a stack without a background plane."""
    from wseg_amd import aff_data as D
    seen = set()
    for si, (h, w) in enumerate(SIZES * 2):
        la = R.quantised_stack(h, w, (0, 2, 9) if si % 2 else (5, 9), 40 + si)
        ha = R.quantised_stack(h, w, (0, 2, 15), 80 + si)
        seed = 700 + si
        _, label, _ = R.host_chain(R.image(h, w, si), la, ha, seed, CROP)
        random.seed(seed)
        p = D.draw_aff_params(w, h, CROP)
        ref, pooled = R.dense_rule(la, ha, p, CROP, np.float32)
        assert label.dtype == np.uint8 and label.shape == (CROP // 8, CROP // 8)
        assert np.array_equal(label, ref), (h, w, p)
        assert np.array_equal(pooled.astype(np.float64), R.dense_rule(la, ha, p, CROP, np.float64)[1])     # the quantisation does what it is for
        seen |= set(np.unique(label).tolist())
    assert {0, 255} <= seen and len(seen - {0, 255}) >= 2


def test_normalize_lut_f32_is_the_float32_evaluation():
    from wseg_amd import aff_data as D, augment as A
    lut = D.normalize_lut_f32()
    assert lut.dtype == np.float32 and lut.shape == (3, 256)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    v = np.arange(256, dtype=np.float32)
    for c in range(3):
        ref = (v / 255. - mean[c]) / std[c]                     # float32 array with Python floats: float32 arithmetic
        assert ref.dtype == np.float32
        assert np.array_equal(lut[c], ref)
    assert not np.array_equal(lut, A.normalize_lut())           # the contrast chain's table is the float64 evaluation: another table
    assert np.abs(lut.astype(np.float64) - A.normalize_lut()).max() < 1e-6


def test_collate_aligns_every_plane_and_counts_the_bytes():
    from wseg_amd import aff_data as D
    samples = []
    for si, (h, w) in enumerate(SIZES):
        la, ha = _stacks(h, w, si)
        if si == 1:
            ha[0] = 0
        samples.append(D.make_aff_sample("n%d" % si, R.image(h, w, si), la, ha, CROP, rng=random.Random(si)))
    b = D.aff_collate(samples)
    planes, ids = b["planes"].numpy(), b["ids"].numpy()
    for s, p in zip(samples, b["params"]):
        assert p["plane_stride"] % 4 == 0 and p["plane_stride"] >= p["H"] * p["W"]
        for k in range(2):
            assert p["planes_off"][k] % 4 == 0 and p["np"][k] == len(s["ids"][k])
            assert ids[p["ids_off"][k]:p["ids_off"][k] + p["np"][k]].tolist() == s["ids"][k].tolist()
            for j in range(p["np"][k]):
                at = p["planes_off"][k] + j * p["plane_stride"]
                assert np.array_equal(planes[at:at + p["H"] * p["W"]], s["planes"][k][j].reshape(-1))
    assert b["params"][1]["np"] == [3, 2]
    shipped, dense = D.dense_bytes(b)
    assert dense == sum(h * w * (3 + 42 * 4) for h, w in SIZES) and shipped < dense / 4


def test_dataset_reads_the_score_files(tmp_path):
    """VOC12AffDataset (host) and VOC12AffDatasetRaw + the dense rule agree on files laid out as aff_prepare writes them."""
    from wseg_amd import aff_data as D, data as wdata
    from wseg_amd.resnet38_contrast import Normalize
    h, w, name = 50, 100, "2007_000032"
    os.makedirs(tmp_path / "JPEGImages"); os.makedirs(tmp_path / "la"); os.makedirs(tmp_path / "ha")
    PIL.Image.fromarray(R.image(h, w, 3)).save(tmp_path / "JPEGImages" / (name + ".jpg"))
    la, ha = _stacks(h, w, 7)
    np.save(tmp_path / "la" / (name + ".npy"), la); np.save(tmp_path / "ha" / (name + ".npy"), ha)
    (tmp_path / "list.txt").write_text(f"/JPEGImages/{name}.jpg\n")
    model_stub = type("M", (), {"normalize": Normalize()})()
    host = wdata.VOC12AffDataset(str(tmp_path / "list.txt"), str(tmp_path / "la"), str(tmp_path / "ha"), str(tmp_path),
                                 wdata.aff_train_transform(model_stub, CROP))
    raw = D.VOC12AffDatasetRaw(str(tmp_path / "list.txt"), str(tmp_path / "la"), str(tmp_path / "ha"), str(tmp_path), CROP)
    random.seed(11)
    img, label = host[0]
    random.seed(11)
    s = raw[0]
    assert img.shape == (3, CROP, CROP) and img.dtype == np.float32
    assert np.array_equal(label, R.dense_rule(la, ha, s["params"], CROP, np.float32)[0])
    assert s["ids"][0].tolist() == [0, 3, 7] and s["ids"][1].tolist() == [0, 3, 12]
