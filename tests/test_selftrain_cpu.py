"""IDF self-training without a GPU: the restated packer (tests/ref_selftrain.py) against the
offline label route end to end, its random cap, the defects the GPU cases must notice, the new
header against its ctypes table, and EFocalLoss's torch composition."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import ref_selftrain as ref
from conftest import ROOT


# ------------------------------------------------------------------ online rule == offline route
H, W = 192, 320   # non-square, ratio 1.67 inside [0.5, 2]: no crop


def _hand_dets():
    """C = 9, R = 6 rows of original-image coordinates: a box at x = 0 and y = 0, one that starts
    below 1 (the clamp acts), one truncation collapses in x and one in y, fractions on both sides
    of .5, and garbage behind every count."""
    dets = np.full((9, 6, 5), np.nan, np.float32)
    counts = np.zeros(9, np.int32)
    dets[1, :3] = [[0.0, 0.0, 57.9, 40.2, 0.9],          # on both edges
                   [0.7, 12.5, 100.49, 80.51, 0.8],      # xmin below 1
                   [30.2, 20.0, 30.9, 90.0, 0.7]]        # collapses in x
    counts[1] = 3
    dets[4, :2] = [[200.6, 100.4, 319.0, 191.0, 0.95],
                   [10.0, 77.1, 150.0, 77.8, 0.6]]       # collapses in y
    counts[4] = 2
    dets[8, :1] = [[1.0, 1.0, 2.0, 2.0, 0.55]]           # 0-based (0, 0, 1, 1)
    counts[8] = 1
    return dets, counts


def _offline_rows(tmp_path, dets, counts, imdb_cls, seed=0):
    """XML by save_labels's writer from the same rows -> imdb -> roidb -> training loader plan."""
    from tlod.config import cfg, setup_training_cfg
    from tlod.data.imdb import CITYSCAPE_CLASSES
    from tlod.data.loader import roibatchLoader
    from tlod.data.roidb import prepare_roidb, rank_roidb_ratio
    from tlod.eval.pseudo import label_objects, write_label_xml
    setup_training_cfg("vgg16", "cityscape")
    root = tmp_path / imdb_cls.__name__
    d = root / "VOC2007"
    for sub in ("JPEGImages", "ImageSets/Main"):
        os.makedirs(d / sub, exist_ok=True)
    img = np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8)
    Image.fromarray(img).save(d / "JPEGImages" / "target_000000.jpg")
    (d / "ImageSets" / "Main" / "train.txt").write_text("target_000000\n")
    write_label_xml(str(root), "2007", "target_000000", H, W,
                    label_objects(dets, counts, CITYSCAPE_CLASSES))
    imdb = imdb_cls("train", "2007", str(root), CITYSCAPE_CLASSES)
    prepare_roidb(imdb)
    ratio_list, ratio_index = rank_roidb_ratio(imdb.roidb)
    assert imdb.roidb[0]["need_crop"] == 0
    ld = roibatchLoader(imdb.roidb, ratio_list, ratio_index, 1, imdb.num_classes, training=True)
    np.random.seed(seed)
    p = ld.plan(0)
    assert cfg.MAX_NUM_GT_BOXES == 50 and p["gt_boxes"].shape == (50, 5)
    return p["gt_boxes"], p["num_boxes"], p["im_scale"]


def _sorted_rows(a):
    return a[np.lexsort(a.T[::-1])]


def test_restated_packer_equals_the_offline_route(tmp_path):
    from tlod.data.imdb import pascal_voc, pseudo_voc
    dets, counts = _hand_dets()
    gt_off, n_off, im_scale = _offline_rows(tmp_path, dets, counts, pseudo_voc)
    assert im_scale == 600.0 / 192.0
    gt, n = ref.pseudo_gt(dets, counts, im_scale, 50, seed=5)
    assert n == n_off == 4  # six rows, two collapse
    np.testing.assert_array_equal(_sorted_rows(gt[:n]), _sorted_rows(gt_off[:n]))
    assert not gt[n:].any() and not gt_off[n:].any()
    # the rows themselves, by hand: max(trunc(x) - 1, 0) * 3.125
    want = np.array([[0, 0, 56, 39, 1], [0, 11, 99, 79, 1], [199, 99, 318, 190, 4],
                     [0, 0, 1, 1, 8]], np.float64)
    want[:, :4] *= 3.125
    np.testing.assert_array_equal(gt[:n], want.astype(np.float32))
    # the same XML through plain pascal_voc: xmin = 0 -> -1, which the uint16 roidb takes as
    # 65535 or, from numpy 2 on, refuses outright — read wrong either way
    try:
        gt_voc, n_voc, _ = _offline_rows(tmp_path, dets, counts, pascal_voc)
    except OverflowError as e:
        assert "-1" in str(e) and "uint16" in str(e)
        return
    assert n_voc != n_off or not np.array_equal(_sorted_rows(gt_voc[:n_voc]),
                                                _sorted_rows(gt_off[:n_off]))
    assert gt_voc[:n_voc, :4].max() > 60000 * 3.125


def test_get_imdb_reaches_the_labelled_set(tmp_path):
    """pseudo_<year>_<set> through get_imdb / combined_roidb, the images under another devkit."""
    from tlod.config import cfg, setup_training_cfg
    from tlod.data.imdb import CITYSCAPE_CLASSES, get_imdb, pseudo_voc
    from tlod.data.roidb import combined_roidb
    from tlod.data.synthetic import synthetic_voc
    from tlod.eval.pseudo import label_objects, write_label_xml
    images, labels = tmp_path / "target", tmp_path / "labels"
    synthetic_voc(str(images), [(H, W)], CITYSCAPE_CLASSES, seed=3, prefix="target_",
                  image_set="train")
    dets, counts = _hand_dets()
    write_label_xml(str(labels), "2007", "target_000000", H, W,
                    label_objects(dets, counts, CITYSCAPE_CLASSES))
    os.makedirs(labels / "VOC2007" / "ImageSets" / "Main")
    (labels / "VOC2007" / "ImageSets" / "Main" / "train.txt").write_text("target_000000\n")
    imdb = get_imdb("pseudo_2007_train", str(labels), image_devkit=str(images))
    assert isinstance(imdb, pseudo_voc) and imdb.name == "pseudo_2007_train"
    assert imdb.image_path_at(0).startswith(str(images))
    assert imdb.roidb[0]["boxes"].dtype == np.uint16 and imdb.roidb[0]["boxes"].max() < 400
    with pytest.raises(FileNotFoundError):
        get_imdb("pseudo_2007_train", str(labels)).image_path_at(0)
    setup_training_cfg("vgg16", "cityscape")
    cfg.TRAIN.USE_FLIPPED = False
    _, roidb, _, _ = combined_roidb("pseudo_2007_train", str(labels), image_devkit=str(images))
    assert len(roidb) == 1 and len(roidb[0]["boxes"]) == 6


# ------------------------------------------------------------------ the cap
def _uncapped(n, rs=0):
    c = np.zeros(9, np.int64)
    c[1:] = np.diff(np.linspace(0, n, 9).astype(int))
    return ref.make_case("cap", 9, 65, c, 20, ref.SCALES[0], 0, ref.NAN_FILL, rs=rs)


def test_cap_keeps_max_gt_distinct_survivors_in_rank_order():
    case = _uncapped(77)
    rows = ref.survivors(case["dets"], case["counts"], case["im_scale"])
    assert len(rows) == 77 and len(np.unique(rows, axis=0)) == 77
    for seed in ref.SEEDS + (11,):
        gt, n = ref.pseudo_gt(case["dets"], case["counts"], case["im_scale"], 20, seed)
        assert n == 20
        # every output row is a survivor, none twice, and they come in the survivors' order
        idx = [int(np.flatnonzero((rows == g).all(1))[0]) for g in gt]
        assert idx == sorted(set(idx)) and len(idx) == 20
    a = ref.pseudo_gt(case["dets"], case["counts"], case["im_scale"], 20, 1)[0]
    b = ref.pseudo_gt(case["dets"], case["counts"], case["im_scale"], 20, 2)[0]
    assert not np.array_equal(a, b)


def test_cap_is_uniform_over_the_ranks():
    """n = 40 survivors, max_gt = 10, seeds 0 .. 1999: under a uniform random subset each rank is
    kept with probability p = 1/4, so its count over T = 2000 independent seeds is Binomial(T, p)
    with sigma = sqrt(T p (1 - p)) = 19.4.  The bound is 4.5 sigma = 87.2 around T p = 500: a
    two-sided tail of 6.8e-6 per rank, 2.7e-4 for the 40 ranks together (union bound) — and the
    seeds are fixed, so the test is deterministic.  Taking the first rows would put ten counts at
    2000 and thirty at 0."""
    n, k, T = 40, 10, 2000
    hits = np.zeros(n, np.int64)
    for seed in range(T):
        kept = ref.cap(n, k, seed)
        assert len(kept) == k and len(set(kept.tolist())) == k and (np.diff(kept) > 0).all()
        hits[kept] += 1
    sigma = np.sqrt(T * (k / n) * (1 - k / n))
    assert hits.sum() == T * k
    assert np.abs(hits - T * k / n).max() <= 4.5 * sigma, (hits.min(), hits.max())


# ------------------------------------------------------------------ defects the GPU cases notice
def _outputs():
    return [ref.pseudo_gt(c["dets"], c["counts"], c["im_scale"], c["max_gt"], c["seed"])
            for c in ref.packer_cases()]


SOUND = None


def _changed(monkeypatch, name, defect):
    """How many of the GPU test's cases expect something else once ref.<name> is defective."""
    global SOUND
    if SOUND is None:
        SOUND = _outputs()
    monkeypatch.setattr(ref, name, defect)
    with np.errstate(all="ignore"):
        bad = _outputs()
    monkeypatch.undo()
    return sum(1 for (g0, n0), (g1, n1) in zip(SOUND, bad)
               if n0 != n1 or not np.array_equal(g0, g1, equal_nan=True))


DEFECTS = {
    "no -1": ("zero_based", lambda t: np.maximum(t, 0.0)),
    "no clamp": ("zero_based", lambda t: t - 1.0),
    "rounding instead of truncation": ("truncate", lambda x: np.rint(x.astype(np.float64))),
    "im_scale taken as float32": (
        "to_blob", lambda v, s: (v * np.float64(np.float32(s))).astype(np.float32)),
    "product in float32": (
        "to_blob", lambda v, s: v.astype(np.float32) * np.float32(s)),
    "first rows instead of keys": ("cap", lambda n, k, seed: np.arange(k)),
    "keys from another stream": (
        "cap", lambda n, k, seed: ref.pick_order(ref.rng_u64(seed, 0, np.arange(n)), k)),
    "32-bit seed": (
        "cap", lambda n, k, seed: ref.pick_order(
            ref.rng_u64(seed & 0xFFFFFFFF, ref.PSEUDO_STREAM, np.arange(n)), k)),
    "a read past counts[j]": ("rows_of", lambda counts, j: int(counts[j]) + 1),
}


@pytest.mark.parametrize("what", list(DEFECTS))
def test_gpu_cases_notice(monkeypatch, what):
    name, defect = DEFECTS[what]
    assert _changed(monkeypatch, name, defect) > 0, what


def test_gpu_cases_cover_what_the_kernel_branches_on():
    cases = ref.packer_cases()
    assert {c["C"] for c in cases} >= {2, 9, 21}
    assert {c["R"] for c in cases} >= {1, 65, 300, 2048}
    assert {c["max_gt"] for c in cases} == {1, 20, 50}
    assert {c["im_scale"] for c in cases} == set(ref.SCALES)
    assert any(c["seed"] > 1 << 32 for c in cases) and any(c["seed"] > 1 << 63 for c in cases)
    n = [len(ref.survivors(c["dets"], c["counts"], c["im_scale"])) for c in cases]
    rel = {ni - c["max_gt"] for ni, c in zip(n, cases)}
    assert 0 in rel and 1 in rel and 0 in n
    assert any(ni == (c["C"] - 1) * c["R"] == 20 * 2048 for ni, c in zip(n, cases))
    assert any(set(c["counts"].tolist()) >= {64, 65, 129} for c in cases)
    assert any(np.isnan(c["dets"]).any() for c in cases)
    assert any((c["dets"] == np.float32(ref.HUGE_FILL)).any() for c in cases)


# ------------------------------------------------------------------ the header and its table
def _declared():
    src = open(os.path.join(ROOT, "include", "tlod_selftrain.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(tlod_[a-z0-9_]+)\s*\(", src)))


def test_selftrain_header_matches_its_table():
    from tlod import _lib
    syms = _declared()
    assert syms and sorted(_lib.SELFTRAIN_SIGNATURES) == syms
    for other in (_lib.SIGNATURES, _lib.EXT_SIGNATURES, _lib.PA_ATF_SIGNATURES,
                  _lib.ROI_SIGNATURES):
        assert not set(syms) & set(other)
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(L, s) for s in syms)
    bound = _lib.lib()
    for s in syms:
        assert getattr(bound, s).argtypes == _lib.SELFTRAIN_SIGNATURES[s][1]
    # every entry point has a guard-band case in the GPU test
    guard = open(os.path.join(ROOT, "tests", "test_selftrain_gpu.py")).read()
    for s in syms:
        assert re.search(r"\.run\(\s*(L|lib\(\))\." + s + r"\b", guard), s


def test_argument_errors_are_refused_on_the_host():
    """Nothing is launched for a bad argument: these return before touching the device."""
    from tlod import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value

    def pack(C=9, R=300, scale=0.5, max_gt=20, out=p, num=p):
        return L.tlod_pseudo_gt_f32(p, p, C, R, scale, max_gt, 0, out, num, None)
    for kw, word in ((dict(R=2049), b"sizes"), (dict(R=0), b"sizes"), (dict(C=1), b"sizes"),
                     (dict(max_gt=0), b"max_gt"), (dict(scale=0.0), b"im_scale"),
                     (dict(scale=-1.0), b"im_scale"), (dict(scale=float("nan")), b"im_scale"),
                     (dict(out=None), b"null"), (dict(num=None), b"null")):
        assert pack(**kw) == -1, kw
        assert word in L.tlod_last_error(), (kw, L.tlod_last_error())
    assert L.tlod_idf_domain_loss_ef_f32(None, 0, 1, p, 5, 2, 3.0, p, None) == -1
    assert b"labels" in L.tlod_last_error()
    assert L.tlod_idf_domain_loss_ef_bwd_f32(None, 0, 1, p, 5, -1, 3.0, p, None, p, None) == -1
    assert L.tlod_idf_domain_loss_ef_f32(None, 0, 1, p, 0, 1, 3.0, p, None) == -1


# ------------------------------------------------------------------ EFocalLoss, torch forms
@pytest.mark.parametrize("label", [0, 1])
def test_efocal_torch_composition(label):
    from tlod.da import idf
    g = torch.Generator().manual_seed(3 + label)
    z = (torch.randn(37, 2, generator=g) * 3).double()
    z_img = (torch.randn(6, 2, generator=g) * 2).double()
    p = torch.softmax(z, 1)[:, label]
    by_hand = sum(-np.exp(-3.0 * float(v)) * np.log(float(v)) for v in p) / 37
    assert abs(float(ref.efocal_loss(z, label, 3.0)) - by_hand) <= 1e-12 * abs(by_hand)
    assert abs(float(idf.efocal_loss_torch(z, label, 3.0)) - by_hand) <= 1e-12 * abs(by_hand)
    got = idf.domain_losses_torch(z_img, label, z, label, 3.0, ef=True)
    plain = idf.domain_losses_torch(z_img, label, z, label, 3.0)
    assert torch.equal(got[:6], plain[:6]) and got.shape == (7,)
    assert abs(float(got[6]) - by_hand) <= 1e-12 * abs(by_hand)
    assert abs(float(got[6] - plain[6])) > 1e-3
    # no clamp: a row FocalLoss clamps at 1e-6 keeps its own value and gradient here
    zc = torch.tensor([[30.0, 0.0]], dtype=torch.float64, requires_grad=True)
    loss = idf.efocal_loss_torch(zc, 1, 3.0)
    loss.backward()
    assert abs(float(loss.detach()) - 30.0) < 1e-6 and abs(float(zc.grad[0, 1]) + 1.0) < 1e-6
