"""CPU restatement of IDF (test infrastructure only): lib/IDF/{faster_rcnn,vgg16,net_utils}.py
and the loss sum of methods/IDF/IDF_train.py:223-339, in plain torch on top of the numpy
restatements under oracle/ (proposal layer, anchor / proposal targets, RoIAlign).  Runs in fp32
and fp64, on the CPU or with its torch parts on the GPU.

Per image the model is called once (source: target=False; target: target=True):
  * two VGG16 stacks, RCNN_base{1,2,3} and RCNN_base{1,2,3}_b (features[:14], [14:21], [21:-1]);
  * domain_k = netD_k(grad_reverse(feat_k, eta)), domain_k_b = netD_k_b(feat_k_b);
  * at levels 2 and 3: att = dam(feat.detach()) for both stacks, dist = the mean channel-axis
    distance of the two maps weighted by the branch's att, loss_se = 0.001 dist, then
    a <- a (1 + att_b), b <- b (1 + att_a);
  * the main stack's RPN proposals (TRAIN), proposal target and fc6 / fc7 feed netD_da through
    a gradient reversal; with target=False they also give the four detection losses, with
    target=True the _b / _t detector does, on the pseudo boxes, while the main stack's
    proposal target sees one all-zero box (its RPN losses are discarded there: not computed).

The distance's axis: PyTorch 0.4.0 (the reference's pin) computes pairwise_distance as
norm(x1 - x2 + eps, p, dim=1): over channels for a 4-D map, eps added to the difference.  It is
spelled out below and F.pairwise_distance (last axis in current torch) is not called.

Replayed draws are consumed in this order: source call anchor target, proposal target; target
call anchor target (RCNN_rpn_t), the main stack's proposal target, the branch's.

rois_override = (source proposals, target main-stack proposals, target branch proposals) and
att_override = (att2, att2_b, att3, att3_b) x (source, target) take the device run's values, so
a score or a cell 1 ulp from a threshold cannot fork the two implementations.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import rpn as orpn
from oracle.daf_step import (CFG, VGG16_CFG, SitePool, SiteReLU, _GRL, _RoIAlignAvgCPU, _np,
                             _smooth_l1, _t, forced_relu)

EPS = 1e-6
DET = ("rpn_loss_cls", "rpn_loss_box", "RCNN_loss_cls", "RCNN_loss_bbox")
DOM = ("d1", "d2", "d3", "d1_b", "d2_b", "d3_b")


# ---------------------------------------------------------------- the restated ops
def dam(feat):
    """net_utils.py:300-306 per image: (N, C, H, W) -> (N, 1, H, W)."""
    s = torch.sigmoid(feat)
    avg = torch.mean(s, dim=1, keepdim=True)
    thr = avg.mean(dim=(1, 2, 3), keepdim=True)
    return torch.where(avg < thr, torch.full_like(avg, 0), avg)


def dam_parts(feat):
    """(avg, thr) of dam: what the 1e-5 thr band of the comparisons needs."""
    avg = torch.mean(torch.sigmoid(feat), dim=1, keepdim=True)
    return avg, avg.mean(dim=(1, 2, 3), keepdim=True)


def distance(a, b, att=None):
    """mean(pairwise_distance(a att, b att, 2, keepdim=True)) of PyTorch 0.4 per image: (N)."""
    diff = (a - b) if att is None else (a - b) * att
    return torch.norm(diff + EPS, 2, dim=1, keepdim=True).mean(dim=(1, 2, 3))


def modulate(a, b, att_a, att_b):
    return a * (1 + att_b), b * (1 + att_a)


def focal_loss(z, label, gamma=3.0):
    """FocalLoss(class_num=2, gamma) (net_utils.py:134-180; alpha = 1, mean over rows)."""
    P = F.softmax(z, dim=1).clamp(1e-6, 1)
    mask = torch.zeros_like(P)
    mask[:, int(label)] = 1.0
    probs = (P * mask).sum(1).view(-1, 1)
    return (-(torch.pow(1 - probs, gamma)) * probs.log()).mean()


def cross_entropy2(z, label):
    y = torch.full((z.shape[0],), int(label), dtype=torch.long, device=z.device)
    return F.cross_entropy(z, y)


# ---------------------------------------------------------------- the model
def _vgg_pieces(forced, prefix):
    layers, cin = [], 3
    for v in VGG16_CFG:
        if v == "M":
            layers.append(SitePool(forced, f"{prefix}.{len(layers)}"))
        else:
            layers += [nn.Conv2d(cin, v, 3, padding=1), SiteReLU(forced, f"{prefix}.{len(layers) + 1}")]
            cin = v
    return (nn.Sequential(*layers[:14]), nn.Sequential(*layers[14:21]), nn.Sequential(*layers[21:]))


def _net_d(cin, mid, k, stride):
    m = nn.Module()
    m.conv1 = nn.Conv2d(cin, mid, k, stride=stride, padding=k // 2, bias=False)
    m.bn1 = nn.BatchNorm2d(mid)
    m.conv2 = nn.Conv2d(mid, 128, k, stride=stride, padding=k // 2, bias=False)
    m.bn2 = nn.BatchNorm2d(128)
    m.conv3 = nn.Conv2d(128, 128, k, stride=stride, padding=k // 2, bias=False)
    m.bn3 = nn.BatchNorm2d(128)
    m.fc = nn.Linear(128, 2)
    return m


def _rpn_module():
    rpn = nn.Module()
    rpn.RPN_Conv = nn.Conv2d(512, 512, 3, padding=1)
    rpn.RPN_cls_score = nn.Conv2d(512, 24, 1)
    rpn.RPN_bbox_pred = nn.Conv2d(512, 48, 1)
    return rpn


class OracleIDF(nn.Module):
    def __init__(self, n_classes=9, dropout=0.5):
        super().__init__()
        self.forced = {}
        self.dropout = dropout
        self.rcnn_cfg = dict(orpn.DEFAULT_RCNN)
        self.RCNN_base1, self.RCNN_base2, self.RCNN_base3 = _vgg_pieces(self.forced, "base")
        self.RCNN_base1_b, self.RCNN_base2_b, self.RCNN_base3_b = _vgg_pieces(self.forced, "base_t")
        for base in (self.RCNN_base1, self.RCNN_base1_b):
            for i in range(10):
                for p in base[i].parameters():
                    p.requires_grad = False
        self.netD_1, self.netD_1_b = _net_d(256, 256, 1, 1), _net_d(256, 256, 1, 1)
        self.netD_2, self.netD_2_b = _net_d(512, 512, 3, 2), _net_d(512, 512, 3, 2)
        self.netD_3, self.netD_3_b = _net_d(512, 512, 3, 2), _net_d(512, 512, 3, 2)
        da = nn.Module()
        da.fc1, da.bn1 = nn.Linear(4096, 100), nn.BatchNorm1d(100)
        da.fc2, da.bn2 = nn.Linear(100, 100), nn.BatchNorm1d(100)
        da.fc3 = nn.Linear(100, 2)
        self.netD_da = da
        fuse = nn.Module()
        fuse.conv3 = nn.Conv2d(512, 512, 3, padding=1, bias=False)
        fuse.bn1 = nn.BatchNorm2d(512)
        fuse.conv1 = nn.Conv2d(512, 512, 1, bias=False)
        for p in fuse.parameters():
            p.requires_grad = False
        self.fuse_3 = fuse
        for tag in ("", "_t"):
            setattr(self, "RCNN_top" + tag, nn.Sequential(
                nn.Linear(25088, 4096), SiteReLU(self.forced, "fc6" + tag), nn.Dropout(dropout),
                nn.Linear(4096, 4096), SiteReLU(self.forced, "fc7" + tag), nn.Dropout(dropout)))
            setattr(self, "RCNN_cls_score" + tag, nn.Linear(4096, n_classes))
            setattr(self, "RCNN_bbox_pred" + tag, nn.Linear(4096, 4 * n_classes))
            setattr(self, "RCNN_rpn" + tag, _rpn_module())
        self.base_anchors = orpn.make_base_anchors(CFG["scales"], CFG["ratios"])

    # ---- pieces
    def _disc(self, name, x):
        """netD_k.forward (vgg16.py:38-45): one activation site per discriminator, its three
        ReLUs in call order."""
        m = getattr(self, name)
        for conv, bn in ((m.conv1, m.bn1), (m.conv2, m.bn2), (m.conv3, m.bn3)):
            x = F.dropout(forced_relu(self.forced, name, bn(conv(x))), self.dropout, self.training)
        x = F.avg_pool2d(x, (x.size(2), x.size(3))).view(-1, 128)
        return m.fc(x)

    def _disc_da(self, x):
        m = self.netD_da
        x = F.dropout(forced_relu(self.forced, "netD_da", m.bn1(m.fc1(x))), self.dropout, self.training)
        x = F.dropout(forced_relu(self.forced, "netD_da", m.bn2(m.fc2(x))), self.dropout, self.training)
        return m.fc3(x)

    def _rpn(self, rpn, site, feat):
        x = forced_relu(self.forced, site, rpn.RPN_Conv(feat))
        score = rpn.RPN_cls_score(x)
        B, C, H, W = score.shape
        sr = score.view(B, 2, C * H // 2, W)
        prob = F.softmax(sr, 1).view(B, C, H, W)
        return sr, prob, rpn.RPN_bbox_pred(x)

    def _proposals(self, prob, bbox, info, override):
        if override is not None:
            return np.asarray(override)
        c = CFG
        return orpn.proposal_layer(_np(prob.float()), _np(bbox.float()), _np(info), self.base_anchors,
                                   c["stride"], c["pre_train"], c["post_train"], c["nms"])

    def _rpn_losses(self, sr, bbox, gt, info, rng):
        H, W = bbox.shape[2:]
        lab, tgt, iw, ow = orpn.anchor_target(H, W, _np(gt), _np(info), self.base_anchors,
                                              CFG["stride"], rng)
        lab_t = _t(lab, bbox).view(-1)
        keep = lab_t != -1
        s2 = sr.permute(0, 2, 3, 1).contiguous().view(-1, 2)
        return (F.cross_entropy(s2[keep], lab_t[keep].long()),
                _smooth_l1(bbox, _t(tgt, bbox), _t(iw, bbox), _t(ow, bbox), sigma=3, dim=[1, 2, 3]))

    def _sample_pool(self, feat, rois, gt, rng, top):
        r, rl, rt, riw, row = orpn.proposal_target(rois, _np(gt), rng, self.rcnn_cfg)
        pooled = _RoIAlignAvgCPU.apply(feat, _t(r, feat).view(-1, 5))
        fc7 = top(pooled.view(pooled.size(0), -1))
        return r, _t(rl, feat).view(-1).long(), rt, riw, row, fc7

    @staticmethod
    def _rcnn_losses(fc7, cls_score, bbox_pred, rl, rt, riw, row):
        bp = bbox_pred(fc7).view(fc7.size(0), -1, 4)
        bp = torch.gather(bp, 1, rl.view(-1, 1, 1).expand(-1, 1, 4)).squeeze(1)
        cls = cls_score(fc7)
        return (F.cross_entropy(cls, rl),
                _smooth_l1(bp, _t(rt, bp).view(-1, 4), _t(riw, bp).view(-1, 4), _t(row, bp).view(-1, 4)))

    def _level(self, a, b, att_override, out):
        """faster_rcnn.py:77-85 / 95-101.  The own maps are always computed (and kept); the
        override, when given, is what the distance and the modulation use."""
        att_a, att_b = dam(a.detach()), dam(b.detach())
        out["att"] += [att_a[:, 0], att_b[:, 0]]
        out["att_parts"] += [dam_parts(a.detach()), dam_parts(b.detach())]
        if att_override is not None:
            att_a, att_b = (x.to(a).view_as(att_a) for x in att_override)
        dist = torch.norm((a - b) * att_b + 1e-6, 2, dim=1, keepdim=True).mean()
        a, b = modulate(a, b, att_a, att_b)
        return a, b, dist

    def call(self, im, info, gt, gt_p, target, rng, rois_override=None, att_override=None, eta=1.0):
        """One forward of the reference model (faster_rcnn.py:52-224) as a dict."""
        info, gt = info.float(), gt.float()
        out = {"att": [], "att_parts": []}
        f1, f1_b = self.RCNN_base1(im), self.RCNN_base1_b(im)
        out["d1"] = self._disc("netD_1", _GRL.apply(f1, eta))
        out["d1_b"] = self._disc("netD_1_b", f1_b)
        out["dist1"] = torch.norm(f1 - f1_b + 1e-6, 2, dim=1, keepdim=True).mean().detach()
        f2, f2_b = self.RCNN_base2(f1), self.RCNN_base2_b(f1_b)
        out["d2"] = self._disc("netD_2", _GRL.apply(f2, eta))
        out["d2_b"] = self._disc("netD_2_b", f2_b)
        ov = att_override
        f2, f2_b, out["dist2"] = self._level(f2, f2_b, None if ov is None else ov[0:2], out)
        f3, f3_b = self.RCNN_base3(f2), self.RCNN_base3_b(f2_b)
        out["d3"] = self._disc("netD_3", _GRL.apply(f3, eta))
        out["d3_b"] = self._disc("netD_3_b", f3_b)
        f3, f3_b, out["dist3"] = self._level(f3, f3_b, None if ov is None else ov[2:4], out)
        out["loss_se_2"], out["loss_se_3"] = 0.001 * out["dist2"], 0.001 * out["dist3"]

        sr, prob, bbox = self._rpn(self.RCNN_rpn, "rpn", f3)
        if target:
            gt_p = gt_p.float()
            sr_t, prob_t, bbox_t = self._rpn(self.RCNN_rpn_t, "rpn_t", f3_b)
            out["rpn_loss_cls"], out["rpn_loss_box"] = self._rpn_losses(sr_t, bbox_t, gt_p, info, rng)
        else:
            out["rpn_loss_cls"], out["rpn_loss_box"] = self._rpn_losses(sr, bbox, gt, info, rng)
        ro = rois_override
        props = self._proposals(prob, bbox, info, None if ro is None else ro[0])
        r, rl, rt, riw, row, fc7 = self._sample_pool(f3, props, gt, rng, self.RCNN_top)
        out["rois_main"] = r
        out["ins"] = self._disc_da(_GRL.apply(fc7, eta))
        if target:
            props_t = self._proposals(prob_t, bbox_t, info, None if ro is None else ro[1])
            r, rl, rt, riw, row, fc7_t = self._sample_pool(f3_b, props_t, gt_p, rng, self.RCNN_top_t)
            out["RCNN_loss_cls"], out["RCNN_loss_bbox"] = self._rcnn_losses(
                fc7_t, self.RCNN_cls_score_t, self.RCNN_bbox_pred_t, rl, rt, riw, row)
        else:
            out["RCNN_loss_cls"], out["RCNN_loss_bbox"] = self._rcnn_losses(
                fc7, self.RCNN_cls_score, self.RCNN_bbox_pred, rl, rt, riw, row)
        out["rois"], out["rois_label"] = r, rl
        return out

    def forward(self, batch, rng, rois_override=None, att_override=None, gamma=3.0, eta=1.0):
        """The training step's two calls over the project's 10-tuple (the target gt_boxes slot
        carries the pseudo boxes; the main stack sees one all-zero box there,
        IDF_train.py:277-280).  Returns (source dict, target dict), each with its seven
        unweighted domain losses under "dom" (label 0 source, 1 target)."""
        im, info, gt, _, _, t_im, t_info, t_gt, _, _ = batch
        ro, ao = rois_override, att_override
        s = self.call(im, info, gt, gt, False, rng, None if ro is None else ro[0:1],
                      None if ao is None else ao[0:4], eta)
        zero = torch.zeros((1, 1, 5), dtype=t_gt.dtype, device=t_gt.device)
        t = self.call(t_im, t_info, zero, t_gt.view(1, -1, 5), True, rng,
                      None if ro is None else ro[1:3], None if ao is None else ao[4:8], eta)
        for o, label in ((s, 0), (t, 1)):
            o["dom"] = [cross_entropy2(o[k], label) for k in DOM] + [focal_loss(o["ins"], label, gamma)]
        return s, t


def total_loss(s, t, separation=True):
    """IDF_train.py:229-335."""
    loss = sum(s[k] for k in DET) + 0.5 * sum(t[k] for k in DET)
    for o in (s, t):
        loss = loss + 0.5 * sum(o["dom"][:6]) + 0.25 * o["dom"][6]
    if separation:
        loss = loss + s["loss_se_2"] + s["loss_se_3"] + t["loss_se_2"] + t["loss_se_3"]
    return loss
