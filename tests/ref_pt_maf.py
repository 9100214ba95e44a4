"""CPU restatement of the PT-MAF VGG16 training step (test infrastructure only).

lib/PT_MAF/{faster_rcnn,faster_rcnn_kd}.py + methods/PT_MAF/PT_MAF_train.py:434-456 on top
of the MAF oracle (oracle/maf_step.py: detector, DRM, weighted-GRL instance head), in plain
torch: the foreground / background maps from the RPN probabilities, six image heads behind
a gradient reversal of 0.1 * ratio with the NLL over their map's cells, the literal
ground-truth cell loops of the teacher and the KD sum of softmax quotients.

Decisions where the reference is loose (the same as tlod.da.pt_maf):
  * a term whose map is empty is 0 with a 0 gradient (masked_nll);
  * the source conv3 b term reads conv3_score_f (faster_rcnn.py:298); conv3_score_b is
    computed and dropped, so RCNN_imageDA_3_b gets gradient from the target image only;
  * the anchor count is the model's own.

maps_override = (f_s, b_s, f_t, b_t) takes the maps of the device run, for the reason
rois_override exists: a probability 1 ulp from a threshold must not fork the two
implementations.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import rpn as orpn
from oracle.daf_step import _RoIAlignAvgCPU, _np, _t, forced_relu
from oracle.frcnn_step import OracleFRCNN
from oracle.maf_step import OracleMAF, drm_chunks

HEADS = (("3", 256, 64, 4), ("4", 512, 256, 2), ("", 512, None, None))
LOSSES = ("rpn_loss_cls", "rpn_loss_box", "RCNN_loss_cls", "RCNN_loss_bbox", "DA_img_loss_cls",
          "DA_ins_loss_cls", "tgt_DA_img_loss_cls", "tgt_DA_ins_loss_cls")


class _GRLRatio(torch.autograd.Function):
    """faster_rcnn.py:24-35: alpha = ratio * 0.1; backward grad.neg() * alpha."""

    @staticmethod
    def forward(ctx, x, ratio):
        ctx.alpha = ratio * 0.1
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.neg() * ctx.alpha, None


def fgbg_maps(prob, A, high, low):
    """faster_rcnn.py:132-148 for one image: (f, b, m, ratio_f, ratio_b)."""
    t, _ = torch.max(prob[:, A:, :, :], dim=1)
    m = torch.max(t)
    f = torch.where(t.gt(m * high), torch.full_like(t, 1), torch.full_like(t, 0))
    b = torch.where(t.lt(m * low), torch.full_like(t, 1), torch.full_like(t, 0))
    ratio_f = f.sum() / (b.sum() + f.sum())
    ratio_b = b.sum() / (b.sum() + f.sum())
    return f, b, m, ratio_f, ratio_b


def masked_nll(score, label, cells):
    """nll_loss(log_softmax(score, 1), label where cells == 1 else -1, ignore_index=-1); an
    empty map gives 0 with a 0 gradient (never NaN)."""
    lab = torch.where(cells == 1, torch.full_like(cells, label).long(),
                      torch.full_like(cells, -1).long())
    if int((cells == 1).sum()) == 0:
        return score.sum() * 0.0
    return F.nll_loss(F.log_softmax(score, dim=1), lab, ignore_index=-1)


def gt_cell_mask(gt_boxes, num_boxes, H, W):
    """faster_rcnn_kd.py:58-65, literally."""
    mask = np.zeros((H, W))
    for k in range(int(num_boxes)):
        bb = gt_boxes[0, k, :4]
        bb = bb / 16.
        for i in range(int(bb[0]), int(bb[2])):
            for j in range(int(bb[1]), int(bb[3])):
                mask[j, i] = 1
    return torch.from_numpy(mask).float()


def kd_sum(rpn1, cls1, rpn2, cls2, mask, rois_label, T, A):
    """PT_MAF_train.py:446-451 from the raw scores: rpn (1, 2, A*H, W), cls (R, C)."""
    rpn_prob1, rpn_prob2 = F.softmax(rpn1 / T, 1), F.softmax(rpn2 / T, 1)
    cls_prob1, cls_prob2 = F.softmax(cls1 / T, 1), F.softmax(cls2 / T, 1)
    rpn_prob1 = rpn_prob1.view(1, A * 2, rpn_prob1.size(2) // A, rpn_prob1.size(3))
    rpn_prob2 = rpn_prob2.view(1, A * 2, rpn_prob2.size(2) // A, rpn_prob2.size(3))
    pos = torch.where(rois_label > 0, torch.ones(rois_label.size()), torch.zeros(rois_label.size()))
    pos, mask = pos.to(cls1), mask.to(cls1)
    return ((1. / (pos.sum() + 1)) * (pos.unsqueeze(1) * cls_prob1
                                      * torch.log(cls_prob1 / cls_prob2)).sum()
            + (1. / (mask.sum() + 1)) * (mask * rpn_prob1 * torch.log(rpn_prob1 / rpn_prob2)).sum())


@torch.no_grad()
def teacher_outputs(teacher, batch, rois):
    """The teacher (an eval-mode OracleFRCNN holding the source-only weights) on the source
    image and the student's sampled rois (faster_rcnn_kd.py:43-108): (RPN scores
    (1, 2, A*H, W), RoI class scores (R, C), the gt cell mask (H, W))."""
    assert not teacher.training
    im, _, gt, num = batch[:4]
    base = teacher.RCNN_base(im)
    x = F.relu(teacher.RCNN_rpn.RPN_Conv(base))
    score = teacher.RCNN_rpn.RPN_cls_score(x)
    B, C, H, W = score.shape
    sr = score.view(B, 2, C * H // 2, W)
    pooled = _RoIAlignAvgCPU.apply(base, _t(np.asarray(rois), base).view(-1, 5))
    cls = teacher.RCNN_cls_score(teacher._head_to_tail(pooled))
    return sr, cls, gt_cell_mask(gt.float(), int(num.view(-1)[0]), H, W)


def make_teacher(n_classes=9):
    return OracleFRCNN(n_classes, scales=(4, 8, 16, 32), dropout=0.0).eval()


class OraclePTMAF(OracleMAF):
    def __init__(self, n_classes=9, dropout=0.5, backbone="vgg16"):
        super().__init__(n_classes, dropout, backbone)
        del self.RCNN_imageDA_3, self.RCNN_imageDA_4, self.RCNN_imageDA
        for side in ("f", "b"):
            for lvl, dim, inner, scale in HEADS:
                m = nn.Module()
                if inner is not None:
                    m.DRM = nn.Module()
                    m.DRM.conv_low_dim = nn.Conv2d(dim, inner, 1, bias=False)
                    m.scale = scale
                    dim = inner * scale * scale
                m.Conv1 = nn.Conv2d(dim, 512, 1, bias=False)
                m.Conv2 = nn.Conv2d(512, 2, 1, bias=False)
                setattr(self, f"RCNN_imageDA_{lvl}_{side}" if lvl else f"RCNN_imageDA_{side}", m)
        self.A = self.RCNN_rpn.RPN_cls_score.out_channels // 2
        self.kept = []

    def _rpn(self, feat):
        """Keeps the score / probability maps of _detect's two calls (source, then target)."""
        out = super()._rpn(feat)
        self.kept.append(out)
        return out

    def _head(self, lvl, side, feat, ratio):
        """_ImageDA_drm / _ImageDA.forward (faster_rcnn.py:49-77); activation sites
        drm{lvl}_{side} / ida{lvl}_{side}."""
        m = getattr(self, f"RCNN_imageDA_{lvl}_{side}" if lvl else f"RCNN_imageDA_{side}")
        x = _GRLRatio.apply(feat, ratio)
        if lvl:
            x = drm_chunks(forced_relu(self.forced, f"drm{lvl}_{side}", m.DRM.conv_low_dim(x)),
                           m.scale)
        return m.Conv2(forced_relu(self.forced, f"ida{lvl}_{side}", m.Conv1(x)))

    def forward(self, batch, rng, rois_override=None, maps_override=None, T=3.0, high=0.7,
                low=0.1, alpha=1.0, beta=1.0, gamma=1.0):
        self.kept = []
        d = self._detect(batch, rng, rois_override)
        (_, s_sr, s_prob, _), (_, _, t_prob, _) = self.kept
        self.kept = []  # graph tensors: the module must stay deep-copyable
        out = {k: d[k] for k in ("rpn_loss_cls", "rpn_loss_box", "RCNN_loss_cls", "RCNN_loss_bbox",
                                 "rois")}
        out["maps"], out["t"], out["m"] = [], [], []
        for n, (pre, lab, prob) in enumerate((("", 1, s_prob), ("t_", 0, t_prob))):
            f, b, m, ratio_f, ratio_b = fgbg_maps(prob.detach(), self.A, high, low)
            out["maps"] += [f, b]
            out["t"].append(torch.max(prob.detach()[:, self.A:], dim=1)[0])
            out["m"].append(m)
            if maps_override is not None:
                f, b = (x.to(prob) for x in maps_override[2 * n:2 * n + 2])
                ratio_f = f.sum() / (b.sum() + f.sum())
                ratio_b = b.sum() / (b.sum() + f.sum())
            c3, c4, c5 = d[pre + "c3"], d[pre + "c4"], d[pre + "base"]
            s3f, s3b = self._head("3", "f", c3, ratio_f), self._head("3", "b", c3, ratio_b)
            s4f, s4b = self._head("4", "f", c4, ratio_f), self._head("4", "b", c4, ratio_b)
            s5f, s5b = self._head("", "f", c5, ratio_f), self._head("", "b", c5, ratio_b)
            if lab == 1:
                s3b = s3f  # faster_rcnn.py:298: the source b term reads conv3_score_f
            img = (alpha * (masked_nll(s3b, lab, b) + masked_nll(s3f, lab, f))
                   + beta * (masked_nll(s4b, lab, b) + masked_nll(s4f, lab, f))
                   + gamma * (masked_nll(s5f, lab, f) + masked_nll(s5b, lab, b)))
            fc7 = d[pre + "fc7"]
            cls_prob = F.softmax(self.RCNN_cls_score(fc7), 1)
            logits = self._instance_da_w(torch.cat((fc7, cls_prob), 1), lab)
            y = torch.zeros(logits.shape[0], dtype=torch.long, device=logits.device)
            y[:256] = lab
            key = "" if lab == 1 else "tgt_"
            out[key + "DA_img_loss_cls"] = img
            out[key + "DA_ins_loss_cls"] = F.cross_entropy(logits, y)
        # rois_label > 0 <=> the sampled RoI is a foreground RoI (overlap >= FG_THRESH with a
        # gt box; the gt classes are >= 1): proposal_target keeps its labels to itself
        gt = _np(batch[2].float())
        ov = orpn.bbox_overlaps(out["rois"][0, :, 1:5], gt[0])
        out["rois_label"] = torch.from_numpy((ov.max(1) >= np.float32(0.5)).astype(np.int64))
        out["kd_scores"] = (s_sr, d["cls"])
        return out

    def kd(self, out, teacher_out, T=3.0):
        t_rpn, t_cls, mask = (x.to(out["kd_scores"][1]) for x in teacher_out)
        return kd_sum(out["kd_scores"][0], out["kd_scores"][1], t_rpn, t_cls, mask,
                      out["rois_label"], T, self.A)


def total_loss(o, lamda=0.1, kd=0.0, tgt=1.0):
    """PT_MAF_train.py:453-456; tgt = 0 drops the target image's DA terms (the conv3 quirk
    test)."""
    return (o["rpn_loss_cls"] + o["rpn_loss_box"] + o["RCNN_loss_cls"] + o["RCNN_loss_bbox"]
            + lamda * (o["DA_img_loss_cls"] + o["DA_ins_loss_cls"]
                       + tgt * (o["tgt_DA_img_loss_cls"] + o["tgt_DA_ins_loss_cls"])) + kd)
