"""CPU restatement of the US-DAF training step (test infrastructure only).

lib/US_DAF/{DA,faster_rcnn}.py + methods/US_DAF/US_DAF_train.py:428-431 on top of the DAF
oracle (oracle/daf_step.py: detector, image / instance heads behind GRL(0.1)), in plain torch:
the literal Python loops of the scale labels, BCEloss_margin verbatim and nn.BCELoss of the
one-channel image map.

Decisions where the reference is loose (the same as tlod.da.us_daf):
  * the instance head takes the backbone's feature width (the reference hard-codes 2048);
  * RCNN_imageDA_class and RCNN_cls_score_img exist on both backbones as frozen parameters
    that no computation reads;
  * label_img / image_softmax are dead code there and are not restated.

rois_override takes the device's proposals, as in the DAF oracle.  gate_override = (gate_s,
gate_t) takes the device's BCEloss_margin gates for the same reason: an element loss within
rounding of 0.5 must not fork the two implementations.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.daf_step import _GRL, OracleDAF, forced_relu

LOSSES = ("rpn_loss_cls", "rpn_loss_box", "RCNN_loss_cls", "RCNN_loss_bbox", "DA_img_loss_cls",
          "DA_ins_loss_cls", "tgt_DA_img_loss_cls", "tgt_DA_ins_loss_cls")


def planted_rois(R, seed=0):
    """R random RoIs whose first rows sit on the label boundaries: area exactly 400 and exactly
    10000 (20 x 20, 100 x 100), the fp32 neighbours of both areas on both sides (height 1, so
    the area is the planted width itself), a zero-padded row, a row with one negative extent
    (area < 0) and one with two (area > 0).  PLANTED_LABELS holds their labels."""
    rng = np.random.default_rng(seed)
    r = np.zeros((R, 5), np.float32)
    r[:, 0] = rng.integers(0, 2, R)
    r[:, 1:3] = rng.uniform(0, 300, (R, 2))
    r[:, 3:5] = r[:, 1:3] + rng.uniform(1, 200, (R, 2)).astype(np.float32)
    f = np.float32
    planted = [(0, 0, 20, 20), (0, 0, 100, 100),
               (0, 0, np.nextafter(f(400), f(0)), 1), (0, 0, np.nextafter(f(400), f(1e9)), 1),
               (0, 0, np.nextafter(f(10000), f(0)), 1), (0, 0, np.nextafter(f(10000), f(1e9)), 1),
               (0, 0, 0, 0), (50, 10, 30, 200), (50, 200, 30, 10)]
    for i, p in enumerate(planted[:R]):
        r[i, 1:] = p
    return r


PLANTED_LABELS = [[1, 0, 0], [0, 0, 1], [1, 0, 0], [0, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0],
                  [1, 0, 0], [0, 1, 0]]


def scale_labels_loop(rois):
    """faster_rcnn.py:104-126 (and :207-231), literally: rois (1, R, 5) or (R, 5) fp32 ->
    (small, middle, large), each (R, 1)."""
    roi_small = []
    roi_middle = []
    roi_large = []
    rois2 = torch.as_tensor(rois, dtype=torch.float32).reshape(-1, 5)
    for i in range(len(rois2)):
        x1 = rois2[i][1]
        y1 = rois2[i][2]
        x2 = rois2[i][3]
        y2 = rois2[i][4]
        area = (x2 - x1) * (y2 - y1)
        if area <= 400:
            roi_small.append(i)
        elif (area > 400) & (area < 10000):
            roi_middle.append(i)
        elif area >= 10000:
            roi_large.append(i)
    small = torch.zeros(len(rois2), 1)
    small[roi_small] = 1
    middle = torch.zeros(len(rois2), 1)
    middle[roi_middle] = 1
    large = torch.zeros(len(rois2), 1)
    large[roi_large] = 1
    return small, middle, large


def scale_labels(rois):
    """(R, 3) = [small, middle, large] of scale_labels_loop."""
    return torch.cat(scale_labels_loop(rois), 1)


def scale_labels_vec(rois):
    """The same rule vectorised (what the torch composition of tlod.da.us_daf computes)."""
    r = torch.as_tensor(rois, dtype=torch.float32).reshape(-1, 5)
    area = (r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2])
    return torch.stack([area <= 400, (area > 400) & (area < 10000), area >= 10000], 1).float()


def BCEloss_margin(x_sigmoid, label, gate=None):
    """faster_rcnn.py:25-33 verbatim (on the input's device); gate: the column-0 weights to use
    instead of its own.  Returns (loss, its own gate (n), the column-0 element losses (n))."""
    NEAR_0 = 1e-10
    scale_weight = torch.ones(len(label), 3).to(x_sigmoid)
    BCEloss = -(label * torch.log(x_sigmoid + NEAR_0) + (1 - label) * torch.log(1 - x_sigmoid + NEAR_0))
    n = len(BCEloss)
    a = (BCEloss[:, 0] > 0.5).reshape(n, -1).float()
    own = a
    if gate is not None:
        a = torch.as_tensor(gate).to(BCEloss).reshape(n, -1)
    weight = torch.cat([a, scale_weight], dim=1)
    col0 = BCEloss[:, 0].detach()
    BCEloss = BCEloss * weight
    return BCEloss.mean(), own.view(-1), col0


def da_losses_from_sigmoid(s_img, y, s_ins, rois, gate=None):
    """The two DA losses of one domain from the sigmoid outputs (any dtype): nn.BCELoss of
    the image map against the constant label y, BCEloss_margin of the instance outputs against
    [y, scale labels].  Returns (img, ins, own gate, column-0 element losses)."""
    img = nn.BCELoss()(s_img.reshape(-1, 1), torch.full_like(s_img, y).reshape(-1, 1))
    lab = torch.cat([torch.full((s_ins.shape[0], 1), y), scale_labels(rois)], 1).to(s_ins)
    ins, own, col0 = BCEloss_margin(s_ins, lab, gate)
    return img, ins, own, col0


class OracleUSDAF(OracleDAF):
    def __init__(self, n_classes=9, dropout=0.5, backbone="vgg16"):
        super().__init__(n_classes, dropout, backbone)
        din = self.RCNN_imageDA.Conv1.in_channels
        self.RCNN_imageDA.Conv2 = nn.Conv2d(512, 1, 1, bias=False)
        self.RCNN_instanceDA.clssifer = nn.Linear(1024, 4)
        dead = nn.Module()
        dead.Conv1 = nn.Conv2d(din, 512, 1, bias=False)
        dead.Conv2 = nn.Conv2d(512, 1, 1, bias=False)
        self.RCNN_imageDA_class = dead
        self.RCNN_cls_score_img = nn.Linear(1, n_classes)
        for p in list(dead.parameters()) + list(self.RCNN_cls_score_img.parameters()):
            p.requires_grad = False

    def _instance_logits(self, x):
        """_InstanceDA.forward (DA.py:83-89) up to the sigmoid; activation sites ip1 / ip2."""
        m = self.RCNN_instanceDA
        x = _GRL.apply(x, 0.1)
        x = F.dropout(forced_relu(self.forced, "ip1", m.dc_ip1(x)), self.dropout, self.training)
        x = F.dropout(forced_relu(self.forced, "ip2", m.dc_ip2(x)), self.dropout, self.training)
        return m.clssifer(x)

    def forward(self, batch, rng, rois_override=None, gate_override=None):
        d = self._detect(batch, rng, rois_override)
        t_rois = rois_override[1] if rois_override is not None else d["t_props"]
        out = {k: d[k] for k in ("rpn_loss_cls", "rpn_loss_box", "RCNN_loss_cls", "RCNN_loss_bbox",
                                 "rois")}
        out["t_rois"] = t_rois
        for n, (pre, key, y, rois) in enumerate((("", "", 1.0, d["rois"]),
                                                 ("t_", "tgt_", 0.0, t_rois))):
            s_img = torch.sigmoid(self._image_da(d[pre + "base"]))
            z_ins = self._instance_logits(d[pre + "fc7"])
            gate = None if gate_override is None else gate_override[n]
            img, ins, own, col0 = da_losses_from_sigmoid(s_img, y, torch.sigmoid(z_ins), rois,
                                                         gate)
            out[key + "DA_img_loss_cls"], out[key + "DA_ins_loss_cls"] = img, ins
            out[pre + "gate"], out[pre + "col0"] = own, col0
            out[pre + "z0"] = z_ins[:, 0].detach()
        return out


def total_loss(o, lamda=0.1):
    """US_DAF_train.py:428-431."""
    return (o["rpn_loss_cls"] + o["rpn_loss_box"] + o["RCNN_loss_cls"] + o["RCNN_loss_bbox"]
            + lamda * (o["DA_img_loss_cls"] + o["DA_ins_loss_cls"] + o["tgt_DA_img_loss_cls"]
                       + o["tgt_DA_ins_loss_cls"]))
