"""Regenerate tests/golden/reference_v1.npz by running the reference's own Python layers.

    python tests/golden/make_reference_golden.py <reference checkout>
    TLOD_REFERENCE_DIR=<reference checkout> python tests/golden/make_reference_golden.py

golden_v1.npz freezes the CPU restatement (oracle/); this fixture freezes what the restatement
restates.  The reference checkout's ``lib`` directory is put on sys.path, its modules are
imported from there and run on the CPU on seeded inputs, and the arrays that went in and came
out are stored together with every random draw.  Nothing of the reference's text is copied:
this file holds inputs, calls and bookkeeping only, and the fixture holds arrays only.
tests/test_reference_golden.py reruns ``generate()`` when the checkout is given and requires
the committed file to be reproduced bit for bit.

The reference was written for Python 3.6 / torch 0.4 with compiled CUDA extensions.  To run
its Python layers under a current CPU torch, these stand-ins are installed for the duration of
``generate()`` and removed afterwards (``reference_modules``):

  easydict          not installed here: ``AttrDict``, a dict with attribute access, as
                    ``easydict.EasyDict`` (model/utils/config.py only builds nested dicts by
                    attribute and reads them back by attribute or key).
  torchvision, torchvision.models, cv2, model.roi_crop.functions.roi_crop
                    empty modules (the last with a ``RoICropFunction = None``), so that
                    model/utils/net_utils.py and US_DAF/DA.py import; nothing run here uses them.
  torch.Tensor.index
                    ``lambda self, idx: self[idx]``: the torch 0.4 method that
                    proposal_target_layer_cascade.py:133 calls.
  F.affine_grid     wrapped to pass ``align_corners=True``, the only behaviour of torch 0.4,
                    for which net_utils._affine_grid_gen was written (today's default is False).
  configuration     ``cfg_from_file`` calls ``yaml.load`` without a loader (an error under
                    PyYAML 6), so the keys a case needs are set on the reference's ``cfg`` for
                    the duration of its call and stored in the fixture (``*_cfg`` arrays):
                    TRAIN.BATCH_SIZE 256 (cfgs/vgg16.yml) or 128 (cfgs/res101.yml),
                    TRAIN.BG_THRESH_LO 0.0 (both files; config.py's bare default is 0.1), and
                    RPN_PRE_NMS_TOP_N / RPN_POST_NMS_TOP_N / RPN_NMS_THRESH of the proposal
                    cases.  (config.py's bare BATCH_SIZE is 128: with it the draw counts differ
                    from oracle.rpn.DEFAULT_RCNN's 256, which restates vgg16.yml.)
  random draws      ``np.random.permutation``, ``np.random.rand`` and ``random.sample`` are
                    replaced for the duration of a call by a recorder that draws from a seeded
                    ``RandomState`` and logs every draw in call order (``draws_to_arrays``:
                    kind 0 permutation, 1 rand, 2 sample).
  nms               the reference's NMS is a CUDA extension.  The ``nms`` name that
                    proposal_layer.py and PA_ATF/proposal_layer1.py imported is replaced by a
                    function that calls ``oracle.nms.nms``.  The proposal fixtures therefore pin
                    decode, clip, sort, the pre-NMS top-N rule, the post-NMS / subsample rule,
                    padding and the batch column; they do not pin NMS itself.  (The reference's
                    nms_cpu.py is no authority either: it disagrees with its CUDA kernel.)

The reference's ``torch.sort`` is not stable, so ``generate()`` asserts that every proposal
case has distinct scores, and (because one ulp of ``exp`` must not be able to flip an NMS
decision between implementations) that no IoU between a kept box and a later candidate lies
within 2e-6 of the threshold; a seed that fails either is skipped, deterministically.
"""
import contextlib
import itertools
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from helpers import gt_set, rpn_outputs  # noqa: E402
from oracle import nms as onms  # noqa: E402
from oracle.boxes import iou_pair_cuda  # noqa: E402
from oracle.rpn import Recorder  # noqa: E402

ENV = "TLOD_REFERENCE_DIR"
OUT = os.path.join(HERE, "reference_v1.npz")
SCALES, RATIOS, STRIDE = [4, 8, 16, 32], [0.5, 1, 2], 16
KINDS = {"perm": 0, "rand": 1, "sample": 2}
IOU_MARGIN = 2e-6


# ------------------------------------------------------------------ run-time stand-ins
class AttrDict(dict):
    """easydict.EasyDict for model/utils/config.py: keys are attributes."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    return m


@contextlib.contextmanager
def reference_modules(ref_root):
    """The reference's ``lib`` importable, with the stand-ins of the module docstring; on exit
    sys.path, sys.modules, torch.Tensor and the bytecode setting are as they were (nothing is
    written into the checkout)."""
    lib = os.path.join(os.path.abspath(ref_root), "lib")
    if not os.path.isdir(os.path.join(lib, "model", "rpn")):
        raise SystemExit(f"{ref_root!r} is not a checkout of the reference (no lib/model/rpn)")
    before = dict(sys.modules)
    path = list(sys.path)
    bytecode = sys.dont_write_bytecode
    own_index = torch.Tensor.__dict__.get("index")       # today's Tensor.index is another method
    tops = {os.path.splitext(n)[0] for n in os.listdir(lib)}
    sys.dont_write_bytecode = True
    sys.path.insert(0, lib)
    tv_models = _module("torchvision.models")
    standins = {"easydict": _module("easydict", EasyDict=AttrDict),
                "torchvision": _module("torchvision", models=tv_models),
                "torchvision.models": tv_models,
                "cv2": _module("cv2"),
                "model.roi_crop.functions.roi_crop": _module("model.roi_crop.functions.roi_crop",
                                                             RoICropFunction=None)}
    sys.modules.update(standins)
    torch.Tensor.index = lambda self, idx: self[idx]
    try:
        yield
    finally:
        if own_index is None:
            del torch.Tensor.index
        else:
            torch.Tensor.index = own_index
        for k in list(sys.modules):
            if k in standins or (k not in before and k.split(".")[0] in tops):
                del sys.modules[k]
        sys.modules.update({k: m for k, m in before.items() if k in standins})
        sys.path[:] = path
        sys.dont_write_bytecode = bytecode


@contextlib.contextmanager
def cfg_set(cfg, **values):
    """``cfg_set(cfg, TRAIN__BATCH_SIZE=256)`` sets cfg.TRAIN.BATCH_SIZE for the block."""
    saved = []
    for key, v in values.items():
        node = cfg
        *parents, leaf = key.split("__")
        for p in parents:
            node = node[p]
        saved.append((node, leaf, node[leaf]))
        node[leaf] = v
    try:
        yield
    finally:
        for node, leaf, v in reversed(saved):
            node[leaf] = v


class Draws(Recorder):
    """oracle.rpn.Recorder plus ``random.sample``: the first k of a permutation of the
    population's positions."""

    def sample(self, population, k):
        pop = list(population)
        picks = [pop[i] for i in self.rs.permutation(len(pop))[:k]]
        self.log.append(("sample", np.asarray(picks, np.int64)))
        return picks


@contextlib.contextmanager
def recording(seed):
    rec = Draws(seed)
    saved = np.random.permutation, np.random.rand, random.sample
    np.random.permutation, np.random.rand, random.sample = rec.permutation, rec.rand, rec.sample
    try:
        yield rec
    finally:
        np.random.permutation, np.random.rand, random.sample = saved


@contextlib.contextmanager
def affine_grid_as_torch04():
    import torch.nn.functional as F
    saved = F.affine_grid
    F.affine_grid = lambda theta, size: saved(theta, size, align_corners=True)
    try:
        yield
    finally:
        F.affine_grid = saved


def draws_to_arrays(log):
    """make_golden.py's layout with a third kind: (kinds int8, lens int64, flat float64)."""
    kinds = np.array([KINDS[k] for k, _ in log], np.int8)
    lens = np.array([len(x) for _, x in log], np.int64)
    flat = (np.concatenate([np.asarray(x, np.float64) for _, x in log]) if log
            else np.zeros(0, np.float64))
    return kinds, lens, flat


def _np(t):
    return np.array(t.detach().cpu().numpy(), order="C", copy=True)   # in-place ops follow


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _put_draws(out, prefix, rec):
    out[prefix + "_draw_kinds"], out[prefix + "_draw_lens"], out[prefix + "_draws"] = \
        draws_to_arrays(rec.log)


# ------------------------------------------------------------------ anchor target
def anchor_cases(base):
    """name -> (H, W, gt (B,G,5), im_info (B,3)); see the module docstring of the test."""
    from oracle.boxes import shifted_anchors
    H, W = 12, 15
    imh, imw = H * STRIDE, W * STRIDE
    info1 = np.array([[imh, imw, 1.0]], np.float32)
    cases = {}
    cases["a"] = (H, W, np.zeros((1, 5, 5), np.float32), info1)                 # no box at all
    gt = np.zeros((2, 4, 5), np.float32)
    gt[0, 0] = gt[0, 1] = [40, 30, 150, 140, 3]                                   # argmax ties
    cases["b"] = (H, W, gt, np.repeat(info1, 2, 0))
    gt = np.zeros((1, 5, 5), np.float32)
    gt[0, 0] = [0, 0, imw - 1, imh - 1, 1]                                        # the image
    gt[0, 1] = [50, 60, 50, 60, 2]                                                # one pixel
    gt[0, 2] = [120, 40, 60, 110, 3]                                              # x2 < x1
    cases["c"] = (H, W, gt, info1)
    # d: 18 x 24, the smallest map tried at which more than 128 fg AND more than 128 bg
    # candidates exist (a 12 x 15 map has 320 inside anchors in all), so both draws happen
    rng = np.random.default_rng(41)
    Hd, Wd = 18, 24
    hd, wd = Hd * STRIDE, Wd * STRIDE
    allb = shifted_anchors(base, Hd, Wd, STRIDE)
    inside = allb[(allb[:, 0] >= 0) & (allb[:, 1] >= 0) & (allb[:, 2] < wd) & (allb[:, 3] < hd)]
    big = inside[(inside[:, 2] - inside[:, 0]) >= 100]
    gt = np.zeros((1, 50, 5), np.float32)
    pick = big[rng.integers(0, len(big), 40)] + rng.integers(-2, 3, (40, 4))
    gt[0, :40, :4] = np.clip(pick, 0, [wd - 1, hd - 1, wd - 1, hd - 1])
    gt[0, :40, 4] = rng.integers(1, 9, 40)
    cases["d"] = (Hd, Wd, gt, np.array([[hd, wd, 1.0]], np.float32))
    rng = np.random.default_rng(42)
    gt = np.stack([gt_set(rng, G=3, pad=5, W=imw, H=imh),
                   gt_set(rng, G=2, pad=5, W=imw - 60, H=imh - 50)])
    cases["e"] = (H, W, gt, np.array([[imh, imw, 1.0], [imh - 50, imw - 60, 1.0]], np.float32))
    rng = np.random.default_rng(43)
    H2, W2 = 20, 30
    gt = np.stack([gt_set(rng, G=3, pad=6, W=W2 * STRIDE, H=H2 * STRIDE) for _ in range(2)])
    cases["f"] = (H2, W2, gt, np.array([[H2 * STRIDE, W2 * STRIDE, 1.0]] * 2, np.float32))
    return cases


def run_anchor_target(out, base):
    from model.rpn.anchor_target_layer import _AnchorTargetLayer
    A = base.shape[0]
    for i, (name, (H, W, gt, info)) in enumerate(anchor_cases(base).items()):
        layer = _AnchorTargetLayer(STRIDE, SCALES, RATIOS)
        B = gt.shape[0]
        with recording(100 + i) as rec:
            res = layer((torch.zeros(B, 2 * A, H, W), _t(gt), _t(info), torch.zeros(B)))
        p = "at_" + name
        out[p + "_hw"] = np.array([H, W], np.int64)
        out[p + "_gt"], out[p + "_info"] = gt, info
        for k, v in zip(("labels", "targets", "inside", "outside"), res):
            out[f"{p}_{k}"] = _np(v).astype(np.float32)
        _put_draws(out, p, rec)
    kinds = out["at_d_draw_kinds"]
    assert len(kinds) == 2, "case d must draw the fg and the bg permutation"
    assert int(out["at_d_draw_lens"][0]) > 128, "case d: fg candidates must exceed the quota"


# ------------------------------------------------------------------ proposal target
def proposal_target_cases():
    """name -> (rois (B,R,5), gt (B,G,5), batch size)."""
    rng = np.random.default_rng(51)
    W, H = 600, 400

    def near(gt, n, jitter):
        g = gt[rng.integers(0, len(gt), n), :4]
        return g + rng.normal(0, jitter, (n, 4))

    def far(n):
        b = rng.uniform(0, [W - 70, H - 70], (n, 2))
        return np.concatenate([b, b + rng.uniform(8, 60, (n, 2))], 1)

    def rois_of(rows, R):
        r = np.zeros((R, 5), np.float32)
        rows = np.clip(rows, 0, [W - 1, H - 1, W - 1, H - 1]).astype(np.float32)
        rows[:, 2:] = np.maximum(rows[:, 2:], rows[:, :2] + 1)
        r[:len(rows), 1:] = rows
        return r

    cases = {}
    gt3 = gt_set(rng, G=3, pad=4, W=W, H=H)
    gt3[:3, 2:4] = np.maximum(gt3[:3, 2:4], gt3[:3, :2] + 120)                   # large: jitter keeps IoU
    cases["a"] = (rois_of(near(gt3[:3], 40, 2.0), 40)[None], gt3[None], 256)      # fg only
    cases["b"] = (rois_of(far(60), 60)[None], np.zeros((1, 4, 5), np.float32), 256)   # bg only
    gt5 = gt_set(rng, G=5, pad=8, W=W, H=H)
    gt5[:5, 2:4] = np.maximum(gt5[:5, 2:4], gt5[:5, :2] + 100)
    small = np.zeros((100, 4))                                                    # 4..12 px boxes: IoU < 0.5
    small[:, :2] = rng.uniform(0, [W - 20, H - 20], (100, 2))
    small[:, 2:] = small[:, :2] + rng.uniform(3, 11, (100, 2))
    c = rois_of(np.concatenate([near(gt5[:5], 300, 2.0), small]), 400)[None]
    cases["c"] = (c, gt5[None], 256)                                              # fg > quota
    cases["c128"] = (c, gt5[None], 128)                                           # cfgs/res101.yml
    d0 = rois_of(np.concatenate([near(gt5[:5], 50, 8.0), far(70)]), 120)
    d1 = rois_of(far(120), 120)
    gtd = np.stack([gt5, np.zeros_like(gt5)])
    cases["d"] = (np.stack([d0, d1]), gtd, 256)                                   # ordinary + bg only
    cases["e"] = (rois_of(np.concatenate([near(gt5[:5], 30, 10.0), far(50)]), 128)[None],
                  gt5[None], 256)                                                 # 48 zero rows
    return cases


def run_proposal_target(out, cfg):
    from model.rpn.proposal_target_layer_cascade import _ProposalTargetLayer
    for i, (name, (rois, gt, batch)) in enumerate(proposal_target_cases().items()):
        p = "pt_" + name
        with cfg_set(cfg, TRAIN__BATCH_SIZE=batch, TRAIN__BG_THRESH_LO=0.0):
            layer = _ProposalTargetLayer(9)
            with recording(200 + i) as rec:
                res = layer(_t(rois), _t(gt), torch.zeros(gt.shape[0]))
            out[p + "_cfg"] = np.array([cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO,
                                        cfg.TRAIN.FG_FRACTION, cfg.TRAIN.FG_THRESH,
                                        cfg.TRAIN.BG_THRESH_HI], np.float64)
        out[p + "_rois_in"], out[p + "_gt"] = rois, gt
        for k, v in zip(("rois", "labels", "targets", "inside", "outside"), res):
            out[f"{p}_{k}"] = _np(v).astype(np.float32)
        _put_draws(out, p, rec)
    k = lambda n: list(out[f"pt_{n}_draw_kinds"])
    assert k("a") == [1] and k("b") == [1] and k("c") == [0, 1] and k("d") == [0, 1, 1], \
        "the proposal-target cases must take the branches they are named for"
    assert int(out["pt_c_draw_lens"][0]) > 64 and (out["pt_a_labels"] > 0).all() \
        and (out["pt_b_labels"] == 0).all()


# ------------------------------------------------------------------ proposal layers
def _oracle_nms(survivors):
    def nms(dets, thresh, force_cpu=False):
        d = _np(dets)
        keep = np.asarray(onms.nms(d, thresh), np.int64)
        survivors.append((d, keep, float(thresh)))
        return torch.from_numpy(keep).view(-1, 1)
    return nms


def _clear_margin(survivors):
    """No IoU that greedy NMS compared (a kept box against every later candidate) lies within
    IOU_MARGIN of the threshold."""
    for d, keep, thr in survivors:
        for k in keep:
            iou = iou_pair_cuda(d[k, :4], d[k + 1:, :4])
            if iou.size and float(np.abs(iou - np.float32(thr)).min()) <= IOU_MARGIN:
                return False
    return True


def _proposal_inputs(seed, B, A, H, W, dscale, infos):
    rng = np.random.default_rng(seed)
    prob, deltas = rpn_outputs(rng, B, A, H, W, delta_scale=dscale)
    fg = prob[:, A:].reshape(B, -1)
    distinct = all(len(np.unique(fg[b])) == fg.shape[1] for b in range(B))
    return prob, deltas, np.asarray(infos, np.float32), distinct


def _run_proposal(module, layer_cls, cfg, key, out, prefix, first_seed, B, H, W, pre, post, dscale,
                  infos, accept=None):
    A = len(SCALES) * len(RATIOS)
    for seed in itertools.count(first_seed):
        prob, deltas, info, distinct = _proposal_inputs(seed, B, A, H, W, dscale, infos)
        if not distinct:
            continue
        survivors = []
        saved = module.nms
        module.nms = _oracle_nms(survivors)
        try:
            with cfg_set(cfg, **{key + "__RPN_PRE_NMS_TOP_N": pre, key + "__RPN_POST_NMS_TOP_N": post,
                                 key + "__RPN_NMS_THRESH": 0.7}):
                with recording(seed) as rec:
                    rois = layer_cls(STRIDE, SCALES, RATIOS)((_t(prob), _t(deltas), _t(info), key))
        finally:
            module.nms = saved
        if _clear_margin(survivors):
            break
    counts = np.array([len(k) for _, k, _ in survivors], np.int64)
    if accept is not None:
        assert accept(counts), (prefix, counts)
    out[prefix + "_seed"] = np.array([seed], np.int64)
    out[prefix + "_prob"], out[prefix + "_deltas"], out[prefix + "_info"] = prob, deltas, info
    out[prefix + "_cfg"] = np.array([pre, post, 0.7], np.float64)
    out[prefix + "_survivors"] = counts
    out[prefix + "_rois"] = _np(rois).astype(np.float32)
    return rec


def run_proposal_layers(out, cfg):
    import model.rpn.proposal_layer as pl
    import PA_ATF.proposal_layer1 as pl1
    full = lambda H, W: [H * STRIDE, W * STRIDE, 1.0]
    cases = [(1, 10, 12, 1000, 200, 0.0, [full(10, 12)]),
             (2, 6, 7, 700, 100, 0.3, [full(6, 7)] * 2),       # N = 504 < pre < B * N = 1008
             (1, 6, 7, 300, 100, 3.0, [full(6, 7)]),           # clipped to degenerate boxes
             (2, 10, 12, 1000, 300, 0.2, [full(10, 12), [140, 171, 1.0]])]
    for i, (B, H, W, pre, post, ds, infos) in enumerate(cases):
        _run_proposal(pl, pl._ProposalLayer, cfg, "TRAIN" if i % 2 == 0 else "TEST", out, f"pl_{i}",
                      300 + 10 * i, B, H, W, pre, post, ds, infos)
    # PA-ATF's subsampled form, key 'TEST', by the number of NMS survivors n against
    # head = int(post * 0.25): n <= head, head < n <= post, n > post
    head = lambda post: int(post * 0.25)
    pa = [(1, 3, 4, 3, 16, 0.0, [full(3, 4)], lambda n, p=16: (n <= head(p)).all()),
          (2, 6, 7, 14, 16, 0.2, [full(6, 7)] * 2,
           lambda n, p=16: ((n > head(p) + 3) & (n <= p)).all()),
          (2, 8, 9, 800, 100, 0.2, [full(8, 9), [120, 130, 1.0]],    # PA_ATF/vgg16.yml's 100
           lambda n, p=100: (n > p).all())]
    for i, (B, H, W, pre, post, ds, infos, accept) in enumerate(pa):
        rec = _run_proposal(pl1, pl1._ProposalLayer, cfg, "TEST", out, f"pa_{i}", 400 + 10 * i, B,
                            H, W, pre, post, ds, infos, accept)
        assert [k for k, _ in rec.log] == ["sample"] * B
        _put_draws(out, f"pa_{i}", rec)


# ------------------------------------------------------------------ box primitives
def run_boxes(out):
    from model.rpn import bbox_transform as bt
    rng = np.random.default_rng(61)
    B, N, K = 2, 50, 5
    W, H = 400, 300

    def boxes(n):
        b = rng.uniform(0, [W - 80, H - 80], (n, 2))
        return np.floor(np.concatenate([b, b + rng.uniform(4, 78, (n, 2))], 1)).astype(np.float32)

    anchors = boxes(N)
    anchors[7, 2:] = anchors[7, :2]                                 # zero-area boxes
    anchors[31, 2:] = anchors[31, :2]
    gt = np.zeros((B, K, 5), np.float32)
    for b in range(B):
        gt[b, :, :4] = anchors[rng.integers(0, N, K)] + rng.integers(-6, 7, (K, 4))
        gt[b, :, 4] = rng.integers(1, 9, K)
    gt[0, 3] = 0                                                    # padding row: zero-area gt
    gt[1, 1, 2:4] = gt[1, 1, :2]                                    # a one-pixel gt
    gt[1, 4] = 0
    rois = np.zeros((B, N, 5), np.float32)
    rois[0, :, 1:] = anchors
    rois[1, :, 1:] = boxes(N)
    rois[1, 12] = 0                                                 # a padding roi
    out["box_anchors"], out["box_gt"], out["box_rois"] = anchors, gt, rois
    out["box_ov2"] = _np(bt.bbox_overlaps_batch(_t(anchors), _t(gt)))
    out["box_ov3"] = _np(bt.bbox_overlaps_batch(_t(rois), _t(gt)))
    assign = rng.integers(0, K, (B, N))
    gt_rois = np.stack([gt[b, assign[b], :4] for b in range(B)])
    out["box_gt_rois"] = gt_rois
    out["box_tf2"] = _np(bt.bbox_transform_batch(_t(anchors), _t(gt_rois)))
    out["box_tf3"] = _np(bt.bbox_transform_batch(_t(rois[:, :, 1:5].copy()), _t(gt_rois)))
    deltas = rng.normal(0, 0.5, (B, N, 4)).astype(np.float32)
    deltas[0, :5] = 0
    deltas[1, :4, 2:] = 4.0                                         # grows far past the image
    bx = np.stack([anchors, rois[1, :, 1:]])
    out["box_deltas"], out["box_boxes"] = deltas, bx
    inv = bt.bbox_transform_inv(_t(bx), _t(deltas), B)
    out["box_inv"] = _np(inv)
    info = np.array([[H, W, 1.0], [H - 90, W - 130, 1.0]], np.float32)
    out["box_info"] = info
    out["box_clip"] = _np(bt.clip_boxes(inv.clone(), _t(info), B))


# ------------------------------------------------------------------ net_utils
def run_net_utils(out):
    from model.utils import net_utils as nu
    rng = np.random.default_rng(71)

    def loss_case(prefix, shape, sigma, dim, outside_scale):
        # float32-representable inputs, evaluated in float64
        pred = rng.normal(0, 0.4, shape).astype(np.float32).astype(np.float64)
        tgt = rng.normal(0, 0.4, shape).astype(np.float32).astype(np.float64)
        inside = (rng.uniform(size=shape) < 0.4).astype(np.float64)
        flat_p, flat_t, flat_i = pred.reshape(-1), tgt.reshape(-1), inside.reshape(-1)
        edge = 1.0 / sigma ** 2
        for j, v in enumerate((edge, -edge, edge, -edge)):       # |diff| == 1 / sigma^2 exactly
            flat_t[3 + 5 * j] = 0.0
            flat_p[3 + 5 * j] = v
            flat_i[3 + 5 * j] = 1.0
        outside = inside * outside_scale
        p = _t(pred).requires_grad_(True)
        loss = nu._smooth_l1_loss(p, _t(tgt), _t(inside), _t(outside), sigma=sigma, dim=dim)
        loss.backward()
        assert ((p.detach() - _t(tgt)).abs() == edge).sum() >= 4
        out[prefix + "_pred"], out[prefix + "_tgt"] = pred, tgt
        out[prefix + "_inside"], out[prefix + "_outside"] = inside, outside
        out[prefix + "_sigma"] = np.array([sigma], np.float64)
        out[prefix + "_loss"] = _np(loss).reshape(1)
        out[prefix + "_grad"] = _np(p.grad)

    loss_case("sl1_rpn", (2, 8, 3, 5), 3, [1, 2, 3], 1.0 / 256)
    loss_case("sl1_rcnn", (37, 4), 1, [1], 1.0)

    rois = np.array([[0, 33.5, 20.25, 410.0, 388.75], [0, 0, 0, 991, 591],
                     [0, 700.5, 100.0, 1100.0, 650.5]], np.float32)
    H, W = 37, 62
    out["aff_rois"], out["aff_hw"] = rois, np.array([H, W], np.int64)
    out["aff_theta"] = _np(nu._affine_theta(_t(rois), (H, W)))
    with affine_grid_as_torch04():
        for g in (7, 14):
            out[f"aff_grid{g}"] = _np(nu._affine_grid_gen(_t(rois), (H, W), g))

    class Three(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Parameter(torch.zeros(7, 5))
            self.b = torch.nn.Parameter(torch.zeros(7))
            self.c = torch.nn.Parameter(torch.zeros(3, 7))

    for name, scale in (("big", 3.0), ("small", 0.5)):             # norm above / below 10
        m = Three()
        for k, p in m.named_parameters():
            p.grad = _t(rng.normal(0, scale, tuple(p.shape)).astype(np.float32))
            out[f"clipg_{name}_before_{k}"] = _np(p.grad)
        nu.clip_gradient(m, 10.)
        for k, p in m.named_parameters():
            out[f"clipg_{name}_after_{k}"] = _np(p.grad)
    n = lambda name: np.sqrt(sum(float((out[f"clipg_{name}_before_{k}"].astype(np.float64) ** 2)
                                       .sum()) for k in "abc"))
    assert n("big") > 10 > n("small")


# ------------------------------------------------------------------ second tier
def run_second_tier(out):
    from MAF.drm import DRM
    from US_DAF.DA import _ImageDA
    rng = np.random.default_rng(81)
    x = rng.normal(0, 1, (1, 8, 6, 8)).astype(np.float32)
    w = rng.normal(0, 0.5, (4, 8, 1, 1)).astype(np.float32)
    out["drm_x"], out["drm_w"] = x, w
    for scale in (2, 4):                                            # 4: rows 4..5 are cropped
        m = DRM(8, 4, scale).double()
        with torch.no_grad():
            m.conv_low_dim.weight.copy_(_t(w).double())
        out[f"drm_y{scale}"] = _np(m(_t(x).double()))
    x = rng.normal(0, 1, (1, 8, 5, 6)).astype(np.float32)
    w1 = rng.normal(0, 0.3, (512, 8, 1, 1)).astype(np.float32)
    w2 = rng.normal(0, 0.1, (1, 512, 1, 1)).astype(np.float32)
    m = _ImageDA(8).double()
    with torch.no_grad():
        m.Conv1.weight.copy_(_t(w1).double())
        m.Conv2.weight.copy_(_t(w2).double())
    xi = _t(x).double().requires_grad_(True)
    y = m(xi)
    gy = rng.normal(0, 1, tuple(y.shape)).astype(np.float32)
    y.backward(_t(gy).double())
    out["ida_x"], out["ida_w1"], out["ida_w2"], out["ida_gy"] = x, w1, w2, gy
    out["ida_y"], out["ida_gx"] = _np(y), _np(xi.grad)


# ------------------------------------------------------------------ driver
def generate(ref_root):
    """Every array of reference_v1.npz, in memory."""
    out = {}
    with reference_modules(ref_root):
        from model.rpn.generate_anchors import generate_anchors
        from model.utils.config import cfg
        base = generate_anchors(scales=np.array(SCALES), ratios=np.array(RATIOS)).astype(np.float32)
        out["anchors_base"] = base
        with cfg_set(cfg, TRAIN__RPN_BATCHSIZE=256, TRAIN__RPN_POSITIVE_OVERLAP=0.7):
            run_anchor_target(out, base)
        run_proposal_target(out, cfg)
        run_proposal_layers(out, cfg)
        run_boxes(out)
        run_net_utils(out)
        run_second_tier(out)
    return out


def main(argv):
    ref = argv[1] if len(argv) > 1 else os.environ.get(ENV)
    if not ref:
        raise SystemExit(f"usage: {os.path.basename(argv[0])} <reference checkout>   (or set {ENV})")
    out = generate(ref)
    np.savez_compressed(OUT, **out)
    print("wrote", len(out), "arrays,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv)
