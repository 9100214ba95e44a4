"""US-DAF without a GPU: the method is listed and constructs on both backbones with the
reference's state_dict names, the dead modules are frozen and unknown to the optimizer, the
CPU restatement (tests/ref_us_daf.py) loads the model's weights, its vectorised scale labels
equal the literal loops, and BCEloss_margin follows the gate rule on hand-computed rows."""
import math

import numpy as np
import pytest
import torch


@pytest.mark.parametrize("R", [1, 3, 256, 300])
def test_vectorised_labels_equal_the_literal_loops(R):
    from ref_us_daf import PLANTED_LABELS, planted_rois, scale_labels, scale_labels_vec
    r = planted_rois(R)
    loop, vec = scale_labels(r), scale_labels_vec(r)
    assert torch.equal(loop, vec)
    assert loop[:len(PLANTED_LABELS)].tolist() == PLANTED_LABELS[:R]
    assert (loop.sum(1) == 1).all()


def test_method_is_listed():
    from tlod.detector.train import METHODS
    assert "us_daf" in METHODS


@pytest.mark.parametrize("net,din,dfeat", [("vgg16", 512, 4096), ("res101", 1024, 2048)])
def test_state_dict_has_the_reference_names(net, din, dfeat):
    from tlod.detector.train import build_model, make_optimizer
    m = build_model("us_daf", "cpu", net)
    sd = m.state_dict()
    want = {"RCNN_imageDA.Conv1.weight": (512, din, 1, 1),
            "RCNN_imageDA.Conv2.weight": (1, 512, 1, 1),
            "RCNN_imageDA_class.Conv1.weight": (512, din, 1, 1),
            "RCNN_imageDA_class.Conv2.weight": (1, 512, 1, 1),
            "RCNN_instanceDA.dc_ip1.weight": (1024, dfeat),
            "RCNN_instanceDA.dc_ip2.weight": (1024, 1024),
            "RCNN_instanceDA.clssifer.weight": (4, 1024),
            "RCNN_instanceDA.clssifer.bias": (4,),
            "RCNN_cls_score_img.weight": (m.n_classes, 1),
            "RCNN_cls_score_img.bias": (m.n_classes,)}
    for k, shape in want.items():
        assert k in sd and tuple(sd[k].shape) == shape, (k, sd.get(k, torch.empty(0)).shape)
    da = {k for k in sd if k.startswith(("RCNN_imageDA", "RCNN_instanceDA", "RCNN_cls_score_img"))}
    assert da == set(want) | {"RCNN_instanceDA.dc_ip1.bias", "RCNN_instanceDA.dc_ip2.bias"}, da

    # the dead modules are frozen and unknown to the optimizer
    dead = [p for k, p in m.named_parameters()
            if k.startswith(("RCNN_imageDA_class.", "RCNN_cls_score_img."))]
    assert len(dead) == 4 and not any(p.requires_grad for p in dead)
    for opt in ("sgd", "adam"):
        groups = make_optimizer(m, 1e-3, fused=False, optimizer=opt).param_groups
        ids = {id(p) for g in groups for p in g["params"]}
        assert not any(id(p) in ids for p in dead)
        assert id(m.RCNN_instanceDA.clssifer.weight) in ids
        assert id(m.RCNN_imageDA.Conv2.weight) in ids


@pytest.mark.parametrize("net", ["vgg16", "res101"])
def test_oracle_loads_the_model_state_dict(net):
    from ref_us_daf import OracleUSDAF
    from tlod.detector.train import build_model
    m = build_model("us_daf", "cpu", net)
    o = OracleUSDAF(dropout=0.0, backbone=net)
    o.load_state_dict(m.state_dict(), strict=True)
    frozen = {k for k, p in o.named_parameters() if not p.requires_grad}
    assert {"RCNN_imageDA_class.Conv1.weight", "RCNN_cls_score_img.bias"} <= frozen


def test_voc2clipart_config_builds_the_published_model():
    from tlod.config import cfg
    from tlod.data.imdb import VOC_CLASSES
    from tlod.detector.train import build_model
    m = build_model("us_daf", "cpu", "res101", classes=VOC_CLASSES, dataset="VOC2clipart")
    assert cfg.MAX_NUM_GT_BOXES == 20 and list(cfg.ANCHOR_SCALES) == [8, 16, 32]
    assert m.RCNN_rpn.nc_score_out == 2 * 9  # 3 scales x 3 ratios
    assert m.n_classes == 21 and m.RCNN_cls_score.out_features == 21
    assert m.RCNN_cls_score_img.out_features == 21


def test_forward_argument_counts():
    from tlod.detector.train import build_model
    m = build_model("us_daf", "cpu")
    with pytest.raises(RuntimeError):  # 4 arguments are the eval-mode detector
        m(*[torch.zeros(1)] * 4)
    with pytest.raises(TypeError):
        m(*[torch.zeros(1)] * 9)


def test_bce_margin_gate_by_hand():
    """Rows well on both sides of the gate: source s = 0.55 (-log 0.55 = 0.598 > 0.5: on) and
    0.70 (0.357: off); target s = 0.45 (on) and 0.30 (off).  Gated-off rows drop their domain
    column and still count in the 4 R denominator; the module's torch composition agrees."""
    from ref_us_daf import BCEloss_margin
    from tlod.da.us_daf import bce_margin
    for y, s0 in ((1.0, (0.55, 0.70)), (0.0, (0.45, 0.30))):
        s = torch.tensor([[s0[0], 0.5, 0.5, 0.5], [s0[1], 0.5, 0.5, 0.5]], requires_grad=True)
        lab = torch.tensor([[y, 1.0, 0.0, 0.0], [y, 0.0, 0.0, 1.0]])
        loss, gate, col0 = BCEloss_margin(s, lab)
        assert gate.tolist() == [1.0, 0.0]
        e_on = -math.log(0.55)
        assert abs(col0[0].item() - e_on) < 1e-6 and abs(col0[1].item() + math.log(0.7)) < 1e-6
        want = (e_on + 6 * math.log(2.0)) / 8.0
        assert abs(loss.item() - want) < 1e-6
        loss.backward()
        assert s.grad[1, 0].item() == 0.0 and s.grad[0, 0].item() != 0.0
        mine, g2 = bce_margin(s.detach(), lab)
        assert abs(mine.item() - loss.item()) < 1e-7 and torch.equal(g2, gate)
        # an override flips the gates
        flipped, own, _ = BCEloss_margin(s.detach(), lab, gate=torch.tensor([0.0, 1.0]))
        assert own.tolist() == [1.0, 0.0]
        assert abs(flipped.item() - (-math.log(0.7) + 6 * math.log(2.0)) / 8.0) < 1e-6


def test_oracle_losses_by_hand():
    """nn.BCELoss of a constant map and the -100 clamp; the instance loss of one small RoI."""
    from ref_us_daf import da_losses_from_sigmoid
    rois = np.array([[0, 0, 0, 10, 10]], np.float32)  # area 100: small
    s_ins = torch.tensor([[0.5, 0.5, 0.5, 0.5]])
    img, ins, gate, _ = da_losses_from_sigmoid(torch.full((1, 1, 2, 3), 0.25), 1.0, s_ins, rois)
    assert abs(img.item() + math.log(0.25)) < 1e-6
    assert abs(ins.item() - math.log(2.0)) < 1e-6 and gate.tolist() == [1.0]
    img, _, _, _ = da_losses_from_sigmoid(torch.ones(1, 1, 2, 3), 0.0, s_ins, rois)
    assert img.item() == 100.0
