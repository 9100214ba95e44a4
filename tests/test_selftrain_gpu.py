"""IDF self-training on the device (csrc/selftrain.hip, tlod.eval.pseudo, the ``ef`` switch of
tlod.da.idf and tlod.detector.train.idf_selftrain_step).

  * tlod_pseudo_gt_f32 is np.array_equal to the numpy restatement (tests/ref_selftrain.py) on
    every case of ``packer_cases``, num_boxes included, under tests/abi_guard.Call's guard bands
    and poison: no tolerance, the rule is truncation plus one double product rounded once.
  * the EF domain losses and their backward against the fp64 restatement at 2e-5 of max|ref|,
    the bar tests/test_idf_abi_gpu.py holds the sibling kernels to; the cross entropies bit-equal
    to tlod_idf_domain_loss_f32's.
  * label_image == detect() + the restated packer; the online route == the offline route
    (save_labels -> pseudo_voc -> roidb -> training loader) row set for row set.
  * one idf_selftrain_step that does label, one whose image gets no label, the ef switch, and
    label_image under torch's sync debug mode.
"""
import numpy as np
import pytest
import torch

import ref_selftrain as ref
from abi_guard import Call

pytestmark = pytest.mark.gpu
dev = "cuda"
f32 = torch.float32
TLOD_EINVAL = -1


def lib():
    from tlod import _lib
    return _lib.lib()


def _ok(st, what=""):
    assert st == 0, (what, st, lib().tlod_last_error().decode(errors="replace"))


# ------------------------------------------------------------------ the packer
CASES = ref.packer_cases()


def _pack(c, case, **over):
    a = dict(case, **over)
    gt = c.out((a["max_gt"], 5), f32, "gt_boxes")
    num = c.out((1,), torch.int64, "num_boxes")
    st = c.run(lib().tlod_pseudo_gt_f32, c.inp(torch.from_numpy(a["dets"]), "dets"),
               c.inp(torch.from_numpy(a["counts"]), "counts"), a["C"], a["R"], a["im_scale"],
               a["max_gt"], a["seed"], gt, num)
    return st, gt, num


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_packer_equals_the_restatement(case):
    want, n = ref.pseudo_gt(case["dets"], case["counts"], case["im_scale"], case["max_gt"],
                            case["seed"])
    c = Call()
    st, gt, num = _pack(c, case)
    _ok(st, case["name"])
    c.check()  # guards, const inputs, every output element written
    got = gt.payload.cpu().numpy()
    print(case["name"], "n", n, "num_boxes", int(num.payload[0]))
    assert int(num.payload[0]) == n
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_packer_refuses_bad_arguments_before_any_launch():
    case = CASES[2]
    for over in (dict(R=2049), dict(C=1), dict(max_gt=0), dict(max_gt=-3), dict(im_scale=0.0),
                 dict(im_scale=-0.5)):
        c = Call()
        # the buffers keep the case's real sizes: a refused call touches none of them
        gt = c.out((case["max_gt"], 5), f32, "gt_boxes")
        num = c.out((1,), torch.int64, "num_boxes")
        a = dict(case, **over)
        st = c.run(lib().tlod_pseudo_gt_f32, c.inp(torch.from_numpy(case["dets"]), "dets"),
                   c.inp(torch.from_numpy(case["counts"]), "counts"), a["C"], a["R"],
                   a["im_scale"], a["max_gt"], a["seed"], gt, num)
        assert st == TLOD_EINVAL, over
        c.check_rejected()
    for null in ("gt", "num"):
        c = Call()
        gt = c.out((case["max_gt"], 5), f32, "gt_boxes")
        num = c.out((1,), torch.int64, "num_boxes")
        st = c.run(lib().tlod_pseudo_gt_f32, c.inp(torch.from_numpy(case["dets"]), "dets"),
                   c.inp(torch.from_numpy(case["counts"]), "counts"), case["C"], case["R"],
                   case["im_scale"], case["max_gt"], case["seed"],
                   None if null == "gt" else gt, None if null == "num" else num)
        assert st == TLOD_EINVAL, null
        c.check_rejected()


def test_pseudo_gt_wrapper():
    from tlod.config import cfg, setup_training_cfg
    from tlod.eval.pseudo import pseudo_gt
    setup_training_cfg("vgg16", "cityscape")
    case = CASES[2]
    dets, counts = torch.from_numpy(case["dets"]).to(dev), torch.from_numpy(case["counts"]).to(dev)
    gt, num = pseudo_gt(dets, counts, case["im_scale"], seed=case["seed"])
    assert gt.shape == (1, cfg.MAX_NUM_GT_BOXES, 5) and num.shape == (1,)
    assert gt.dtype == f32 and num.dtype == torch.int64 and gt.is_cuda and num.is_cuda
    want, n = ref.pseudo_gt(case["dets"], case["counts"], case["im_scale"], 50, case["seed"])
    assert int(num) == n and np.array_equal(gt[0].cpu().numpy(), want)
    with pytest.raises(ValueError):
        pseudo_gt(dets, counts, 0.0)


# ------------------------------------------------------------------ EFocalLoss
def _close(got, want, rtol):
    got, want = got.double().cpu(), want.double().cpu()
    err = float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)
    print("rel err", err)
    assert err <= rtol, err


def _logits(n_img, R, label):
    """As tests/test_idf_abi_gpu.py::test_domain_loss_and_backward draws them (|z| <= 20)."""
    g = torch.Generator().manual_seed(6 + R)
    z_img = torch.randn(n_img, 2, generator=g) * 2
    z_ins = torch.randn(R, 2, generator=g) * 3
    z_ins[1] = torch.tensor([18.0, -2.0]) if label == 1 else torch.tensor([-2.0, 18.0])
    return z_img, z_ins, torch.randn(n_img + 1, generator=g)


@pytest.mark.parametrize("n_img,R,label", [(6, 256, 0), (6, 300, 1), (0, 5, 1), (6, 256, 1),
                                           (6, 300, 0), (0, 5, 0)])
def test_ef_domain_loss_and_backward(n_img, R, label):
    import ref_idf
    L = lib()
    z_img, z_ins, g_loss = _logits(n_img, R, label)
    assert float(z_ins.abs().max()) <= 20
    zi, zn = z_img.double().requires_grad_(True), z_ins.double().requires_grad_(True)
    terms = [ref_idf.cross_entropy2(zi[i:i + 1], label) for i in range(n_img)]
    terms.append(ref.efocal_loss(zn, label, 3.0))
    want = torch.stack(terms)
    (want * g_loss.double()).sum().backward()

    c = Call()
    loss = c.out((n_img + 1,), f32, "loss")
    _ok(c.run(L.tlod_idf_domain_loss_ef_f32, c.inp(z_img, "z_img") if n_img else None, n_img,
              label, c.inp(z_ins, "z_ins"), R, label, 3.0, loss))
    c.check()
    _close(loss.payload, want.detach(), 2e-5)
    # the cross entropies: bit for bit the sibling kernel's
    c = Call()
    plain = c.out((n_img + 1,), f32, "loss")
    _ok(c.run(L.tlod_idf_domain_loss_f32, c.inp(z_img, "z_img") if n_img else None, n_img, label,
              c.inp(z_ins, "z_ins"), R, label, 3.0, plain))
    c.check()
    assert torch.equal(loss.payload[:n_img], plain.payload[:n_img])
    assert float(loss.payload[n_img]) != float(plain.payload[n_img])

    c = Call()
    dz_img = c.out((n_img, 2), f32, "dz_img") if n_img else None
    dz_ins = c.out((R, 2), f32, "dz_ins")
    _ok(c.run(L.tlod_idf_domain_loss_ef_bwd_f32, c.inp(z_img, "z_img") if n_img else None, n_img,
              label, c.inp(z_ins, "z_ins"), R, label, 3.0, c.inp(g_loss, "g_loss"), dz_img,
              dz_ins))
    c.check()
    if n_img:
        _close(dz_img.payload, zi.grad, 2e-5)
    _close(dz_ins.payload, zn.grad, 2e-5)
    # no clamp: the row FocalLoss clamps (softmax[label] = 2e-9) keeps its gradient here
    assert torch.count_nonzero(dz_ins.payload[1]).item() == 2

    # a label of 2 is refused before any launch
    c = Call()
    loss = c.out((n_img + 1,), f32, "loss")
    st = c.run(L.tlod_idf_domain_loss_ef_f32, c.inp(z_img, "z_img") if n_img else None, n_img,
               label, c.inp(z_ins, "z_ins"), R, 2, 3.0, loss)
    assert st == TLOD_EINVAL
    c.check_rejected()
    c = Call()
    dz_ins = c.out((R, 2), f32, "dz_ins")
    st = c.run(L.tlod_idf_domain_loss_ef_bwd_f32, None, 0, 2, c.inp(z_ins, "z_ins"), R, label, 3.0,
               c.inp(g_loss[-1:], "g_loss"), None, dz_ins)
    assert st == TLOD_EINVAL
    c.check_rejected()


@pytest.mark.parametrize("n_img,R,label", [(6, 256, 0), (6, 300, 1)])
def test_domain_loss_function_ef_matches_the_torch_composition(monkeypatch, n_img, R, label):
    from tlod.da.idf import _DomainLoss, domain_losses
    z_img, z_ins, g_loss = _logits(n_img, R, label)
    res = []
    for fused in ("1", "0"):
        monkeypatch.setenv("TLOD_FUSED_IDF", fused)
        zi = z_img.to(dev).requires_grad_(True)
        zn = z_ins.to(dev).requires_grad_(True)
        if fused == "1":
            out = _DomainLoss.apply(zi, zn, label, label, 3.0, True)
            assert torch.equal(out, domain_losses(zi, label, zn, label, 3.0, ef=True))
        else:
            out = domain_losses(zi, label, zn, label, 3.0, ef=True)
        (out * g_loss.to(dev)).sum().backward()
        res.append((out.detach(), zi.grad, zn.grad))
    for got, want in zip(res[0], res[1]):
        _close(got, want, 2e-5)
    # the 5-argument form still is the plain focal loss
    monkeypatch.setenv("TLOD_FUSED_IDF", "1")
    plain = _DomainLoss.apply(z_img.to(dev), z_ins.to(dev), label, label, 3.0)
    assert torch.equal(plain[:n_img], res[0][0][:n_img]) and plain[n_img] != res[0][0][n_img]


# ------------------------------------------------------------------ label_image
H, W, SCALE = 192, 320, 600.0 / 192.0
R, C = 300, 9


class StubLabeler(torch.nn.Module):
    """An eval-mode detector that returns hand-built (rois, cls_prob, bbox_pred) triples, one per
    call, round robin."""

    def __init__(self, triples):
        super().__init__()
        self.triples, self.calls = triples, 0
        self.eval()

    def forward(self, im_data, im_info, gt_boxes, num_boxes):
        t = self.triples[self.calls % len(self.triples)]
        self.calls += 1
        return t + (0, 0, 0, 0, None)


def _triple(seed, groups=((1, 5), (4, 4), (8, 3)), loners=((1, 2), (4, 2), (8, 2)), to=None):
    """R = 300 RoIs on a 600 x 1000 blob, background everywhere but for a handful of rows:
    per (class, k) of ``groups`` k jittered copies of one box (the NMS keeps one or two), per
    ``loners`` k far-apart boxes; all with a class score above 0.5.  One group sits on the
    blob's left / top edge."""
    rng = np.random.default_rng(seed)
    Hb, Wb = H * SCALE, W * SCALE
    x1 = rng.uniform(0, Wb - 120, R)
    y1 = rng.uniform(0, Hb - 120, R)
    boxes = np.stack([x1, y1, x1 + rng.uniform(30, 110, R), y1 + rng.uniform(30, 110, R)], 1)
    prob = np.full((R, C), 0.02 / (C - 1), np.float32)
    prob[:, 0] = 0.98
    rows = iter(rng.permutation(R))
    for gi, (j, k) in enumerate(groups):
        base = np.array([0.0, 0.0, 200.0, 150.0]) if gi == 0 else \
            np.array([300.0 * gi, 100.0 * gi, 300.0 * gi + 180.0, 100.0 * gi + 220.0])
        for _ in range(k):
            r = next(rows)
            boxes[r] = np.clip(base + rng.uniform(-6, 6, 4), 0, None)
            s = rng.uniform(0.55, 0.97)
            prob[r] = (1 - s) / (C - 1)
            prob[r, j] = s
    for j, k in loners:
        for _ in range(k):
            r = next(rows)
            s = rng.uniform(0.55, 0.97)
            prob[r] = (1 - s) / (C - 1)
            prob[r, j] = s
    rois = np.concatenate([np.zeros((R, 1)), boxes], 1).astype(np.float32)
    bbox = rng.normal(0, 0.3, (R, 4 * C)).astype(np.float32)
    return tuple(torch.from_numpy(a).to(dev if to is None else to)[None]
                 for a in (rois, prob.astype(np.float32), bbox))


def _image(seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, 3, int(H * SCALE), int(W * SCALE), generator=g).to(dev)


def test_label_image_equals_detect_then_the_restated_packer():
    from tlod.config import setup_training_cfg
    from tlod.eval.detect import detect
    from tlod.eval.pseudo import label_image
    setup_training_cfg("vgg16", "cityscape")
    info = (H * SCALE, W * SCALE, SCALE)
    for seed, max_gt in ((1, None), (2, 5)):
        t = _triple(seed)
        gt, num = label_image(StubLabeler([t]), _image(), info, max_gt=max_gt, seed=77 + seed)
        dets, counts = detect(t[0][0], t[1][0], t[2][0],
                              torch.tensor(info, dtype=f32, device=dev), False, 0.5)
        d, n = dets.cpu().numpy(), counts.cpu().numpy()
        kept = n[1:].sum()
        print("kept per class", n.tolist())
        assert (n > 0).sum() == 3 and 6 <= kept < 18  # three classes; 18 rows score above 0.5
        want, k = ref.pseudo_gt(d, n, SCALE, 50 if max_gt is None else max_gt, 77 + seed)
        assert int(num) == k == min(kept, 50 if max_gt is None else max_gt)
        assert np.array_equal(gt[0].cpu().numpy(), want)
        assert gt.shape[0] == 1 and num.shape == (1,) and num.dtype == torch.int64
    with pytest.raises(RuntimeError):
        label_image(StubLabeler([t]).train(), _image(), info)


def _sorted_rows(a):
    return a[np.lexsort(a.T[::-1])]


def test_online_route_equals_offline_route(tmp_path):
    """save_labels over a two-image target set, then pseudo_voc, the roidb and the training
    loader, against label_image on the same images with the same (stub) labeler outputs."""
    from tlod.config import cfg, setup_training_cfg
    from tlod.data.imdb import CITYSCAPE_CLASSES, get_imdb, pascal_voc
    from tlod.data.loader import roibatchLoader
    from tlod.data.roidb import prepare_roidb, rank_roidb_ratio
    from tlod.data.synthetic import synthetic_voc
    from tlod.eval.pseudo import label_image, save_labels
    setup_training_cfg("vgg16", "cityscape")
    cfg.TRAIN.USE_FLIPPED = False
    images, labels = tmp_path / "target", tmp_path / "labels"
    synthetic_voc(str(images), [(H, W), (H, W)], CITYSCAPE_CLASSES, seed=4, n_objects=3,
                  prefix="target_", image_set="train")
    target = pascal_voc("train", "2007", str(images), CITYSCAPE_CLASSES, prefix="cityscape")
    prepare_roidb(target)
    rl, ri = rank_roidb_ratio(target.roidb)
    test_ld = roibatchLoader(target.roidb, rl, ri, 1, target.num_classes, training=False)
    triples = [_triple(11), _triple(12)]
    written = save_labels(StubLabeler(triples), target, test_ld, str(labels))
    assert len(written) == 2 and all(6 <= w < 18 for w in written)

    online = []
    stub = StubLabeler(triples)
    for i in range(2):
        p = test_ld.plan(i)
        data = test_ld[i][0].unsqueeze(0)
        assert tuple(data.shape[2:]) == (600, 1000) and p["im_scale"] == SCALE
        gt, num = label_image(stub, data, (600, 1000, p["im_scale"]), seed=i)
        online.append(gt[0, :int(num)].cpu().numpy())

    imdb = get_imdb("pseudo_2007_train", str(labels), image_devkit=str(images))
    prepare_roidb(imdb)
    rl, ri = rank_roidb_ratio(imdb.roidb)
    train_ld = roibatchLoader(imdb.roidb, rl, ri, 1, imdb.num_classes, training=True)
    for idx in range(2):
        np.random.seed(idx)
        _, im_info, gt, num = train_ld[idx]
        i = int(ri[idx])
        n = int(num)
        print("image", i, "rows", n, "dropped", written[i] - n)
        assert n == len(online[i]) > 0
        assert np.array_equal(_sorted_rows(gt[:n].cpu().numpy()), _sorted_rows(online[i]))
        assert not gt[n:].any()
        assert float(im_info[2]) == np.float32(SCALE)


# ------------------------------------------------------------------ the training step
def _step_fixture():
    from tlod.detector.train import SyntheticCityscapes, build_model, make_optimizer
    m = build_model("idf", dev)
    labeler = build_model("faster_rcnn", dev, seed=1).eval()
    for p in labeler.parameters():
        p.requires_grad_(False)
    opt = make_optimizer(m, 1e-3)
    data = SyntheticCityscapes(dev, H=H, W=W, G=4, pool=1, seed=7)
    return m, labeler, opt, data.next()


def test_idf_selftrain_step_labels_and_trains():
    from tlod.detector.train import idf_selftrain_step, idf_train_step
    m, labeler, opt, batch = _step_fixture()
    info = (H, W, 600.0 / 1024.0)
    before = {k: v.detach().clone() for k, v in m.named_parameters() if v.requires_grad}
    frozen = {k: v.detach().clone() for k, v in labeler.state_dict().items()}
    loss, num = idf_selftrain_step(m, labeler, opt, batch, thresh=0.05, im_info_host=info)
    print("num_boxes_p", int(num), "loss", float(loss))
    assert int(num) > 0  # a random-init softmax over 9 classes sits near 0.11 > 0.05
    assert torch.isfinite(loss)
    moved = [k for k, v in m.named_parameters() if v.requires_grad
             and not torch.equal(v.detach(), before[k])]
    for part in ("RCNN_rpn_t.", "RCNN_top_t.", "RCNN_cls_score_t.", "RCNN_bbox_pred_t.",
                 "RCNN_base3_b."):
        assert any(k.startswith(part) for k in moved), part
    assert all(torch.equal(v, frozen[k]) for k, v in labeler.state_dict().items())
    assert not labeler.training and m.training

    # an image that gets no label: its detection losses are gated off on the device
    none = StubLabeler([_no_detection()])
    loss, num = idf_selftrain_step(m, none, opt, batch, thresh=0.5, im_info_host=info)
    assert int(num) == 0 and torch.isfinite(loss)
    for k, p in m.RCNN_rpn_t.named_parameters():
        assert p.grad is not None and torch.count_nonzero(p.grad).item() == 0, k
    assert any(torch.count_nonzero(p.grad).item() for p in m.RCNN_rpn.parameters())
    assert any(torch.count_nonzero(p.grad).item() for p in m.netD_3_b.parameters())

    # the ef switch: the same two calls' outputs summed both ways, then one whole step
    from tlod.detector.train import idf_forward
    with torch.no_grad():
        out_s, out_t = idf_forward(m, batch)
        plain = m.total_loss(out_s, out_t)
        ef = m.total_loss(out_s, out_t, ef=True)
        d = sum(m.domain_terms(o, l, 3.0, True)[6] - m.domain_terms(o, l, 3.0)[6]
                for o, l in ((out_s, 0), (out_t, 1)))
    assert torch.isfinite(ef) and float(ef) != float(plain)
    assert abs(float(ef - plain) - 0.25 * float(d)) <= 1e-5 * abs(float(plain))
    assert torch.isfinite(idf_train_step(m, opt, batch, ef=True))


def _no_detection():
    rois, prob, bbox = _triple(5)
    prob = torch.full_like(prob, 0.01 / (C - 1))
    prob[..., 0] = 0.99
    return rois, prob, bbox


def test_label_image_makes_no_host_sync():
    from tlod.detector.train import build_model
    from tlod.eval.pseudo import label_image
    labeler = build_model("faster_rcnn", dev, seed=1).eval()
    data = _image(3)[:, :, :H, :W].contiguous()
    info = (H, W, 600.0 / 1024.0)
    label_image(labeler, data, info, thresh=0.05, seed=1)  # workspaces and constants warm
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        gt, num = label_image(labeler, data, info, thresh=0.05, seed=2)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert int(num) > 0 and bool(torch.isfinite(gt).all())
