"""PT-MAF without a GPU: the model constructs with the reference's head names, and the CPU
restatement (tests/ref_pt_maf.py) follows the empty-map rule and the conv3 quirk on
hand-computed 2x3 maps."""
import math

import torch

HEAD_NAMES = ("RCNN_imageDA_3_f", "RCNN_imageDA_3_b", "RCNN_imageDA_4_f", "RCNN_imageDA_4_b",
              "RCNN_imageDA_f", "RCNN_imageDA_b")


def test_method_is_listed_and_constructs():
    from tlod.detector.train import METHODS, build_model
    assert "pt_maf" in METHODS
    m = build_model("pt_maf", "cpu")
    keys = set(m.state_dict())
    for name in HEAD_NAMES:
        assert f"{name}.Conv1.weight" in keys and f"{name}.Conv2.weight" in keys
        if "_3_" in name or "_4_" in name:
            assert f"{name}.DRM.conv_low_dim.weight" in keys
    assert not any(k.startswith(("RCNN_imageDA.", "RCNN_imageDA_3.", "RCNN_imageDA_4."))
                   for k in keys)
    assert "RCNN_instanceDA.clssifer.weight" in keys
    assert m.RCNN_instanceDA.dc_ip1.in_features == 4096 + m.n_classes
    assert m.num_anchor == 12


def test_oracle_loads_the_model_state_dict():
    from ref_pt_maf import OraclePTMAF
    from tlod.detector.train import build_model
    m = build_model("pt_maf", "cpu")
    sd = {k: v for k, v in m.state_dict().items()
          if not k.startswith(("conv3.", "conv34.", "conv45."))}
    OraclePTMAF(dropout=0.0).load_state_dict(sd, strict=True)


def test_oracle_maps_and_empty_map_rule_by_hand():
    from ref_pt_maf import fgbg_maps, masked_nll
    # A = 2: object channels 2, 3; t = their max per cell
    obj = torch.tensor([[[0.9, 0.05, 0.5], [0.6, 0.2, 0.08]],
                        [[0.1, 0.02, 0.64], [0.3, 0.09, 0.01]]])
    prob = torch.cat([1 - obj, obj], 0)[None]
    f, b, m, ratio_f, ratio_b = fgbg_maps(prob, 2, 0.7, 0.1)
    # t = [[.9, .05, .64], [.6, .2, .08]], m = .9: f = t > .63, b = t < .09
    assert m.item() == obj.max().item()
    assert f[0].tolist() == [[1, 0, 1], [0, 0, 0]]
    assert b[0].tolist() == [[0, 1, 0], [0, 0, 1]]
    assert ratio_f.item() == 0.5 and ratio_b.item() == 0.5

    score = torch.tensor([[[[1.0, 0.0, 2.0], [0.0, 0.0, 0.0]],
                           [[0.0, 0.0, 0.0], [3.0, 0.0, 1.0]]]], requires_grad=True)
    # label 1 over f's cells (0,0) and (0,2): -log softmax[1] = log(1 + e^1), log(1 + e^2)
    loss = masked_nll(score, 1, f)
    want = 0.5 * (math.log1p(math.e) + math.log1p(math.e ** 2))
    assert abs(loss.item() - want) < 1e-6
    loss.backward()
    assert score.grad[0, :, 1].abs().sum() == 0  # row 1 holds no f cell
    assert abs(score.grad[0, 0, 0, 0].item() - 0.5 * math.e / (1 + math.e)) < 1e-6
    # an empty map: exactly 0, zero gradient, no NaN
    score.grad = None
    empty = masked_nll(score, 0, torch.zeros(1, 2, 3))
    empty.backward()
    assert empty.item() == 0.0 and torch.count_nonzero(score.grad).item() == 0


def test_oracle_conv3_quirk_by_hand():
    """The source conv3 b term is NLL(score3_f, labels from b): with a 3_b head whose score
    would give a different value, the oracle's term equals the hand value from score3_f."""
    from ref_pt_maf import masked_nll
    b = torch.tensor([[[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]])
    s3f = torch.zeros(1, 2, 2, 3)
    s3f[0, 1, 0, 1] = 2.0  # cell (0,1): -log softmax[1] = log(1 + e^-2); cell (1,2): log 2
    s3b = torch.full((1, 2, 2, 3), 5.0)
    s3b[0, 1] = -5.0
    quirk = masked_nll(s3f, 1, b)
    assert abs(quirk.item() - 0.5 * (math.log1p(math.exp(-2.0)) + math.log(2.0))) < 1e-6
    assert abs(masked_nll(s3b, 1, b).item() - quirk.item()) > 1.0


def test_oracle_gt_cell_mask_and_kd_by_hand():
    from ref_pt_maf import gt_cell_mask, kd_sum
    gt = torch.zeros(1, 3, 5)
    gt[0, 0] = torch.tensor([16.0, 0.0, 47.0, 31.9, 1.0])   # cells x 1..1, y 0..0
    gt[0, 1] = torch.tensor([0.0, 16.0, 15.0, 32.0, 2.0])   # empty x range
    gt[0, 2] = torch.tensor([0.0, 0.0, 48.0, 32.0, 3.0])    # past num_boxes
    assert gt_cell_mask(gt, 2, 2, 3).tolist() == [[0, 1, 0], [0, 0, 0]]
    # student == teacher: both parts 0
    rpn = torch.randn(1, 2, 2 * 2, 3)
    cls = torch.randn(4, 5)
    lab = torch.tensor([1, 0, 3, 0])
    assert kd_sum(rpn, cls, rpn, cls, torch.ones(2, 3), lab, 3.0, 2).item() == 0.0
    # one positive RoI of two classes against a uniform teacher, T = 1, empty cell mask:
    # p1 = (.75, .25): KL = .75 log 1.5 + .25 log .5, over pos.sum() + 1 = 2
    s = torch.tensor([[math.log(3.0), 0.0]])
    kd = kd_sum(rpn, s, rpn, torch.zeros(1, 2), torch.zeros(2, 3), torch.tensor([2]), 1.0, 2)
    want = 0.5 * (0.75 * math.log(1.5) + 0.25 * math.log(0.5))
    assert abs(kd.item() - want) < 1e-6
