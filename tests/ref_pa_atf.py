"""PA-ATF on the CPU (test infrastructure): a literal restatement of
lib/PA_ATF/faster_rcnn.py:182-409, proposal_layer1.py:152-160 and
methods/PA_ATF/PA_ATF_train.py:405-408 over oracle/ (OracleATF's backbones, RPN passes, sampling
and head), in the dtype of its parameters (fp32, or fp64 after .double()).

Every branch and image gets its own pass, every loss its own torch composition: BCELoss of the
sigmoid (elementwise over equal element counts), torch.abs(x (R, 1) - label (R)).mean() with
its (R, R) broadcast, nll_loss(log_softmax) for CLUB.

rois_override: (s proposals, t proposals, the target's kept survivors (1, cap, 4), the target's
picked RoIs) from the device run, so a float-order difference in a score sort cannot fork the
two runs; ``count`` is then the device's survivor count, and the pick is redone here from the
replayed draw and compared by the test.  arg_override: the device's gate arguments per level
((2, C): the source's row, then the target's), for the same reason: a near-tie between two
cells of a mask-net plane would otherwise route one channel's mask through another cell (the
rule tests/ref_idf.py states for its attention maps).  pp_override: the device's prototype
pooling argmax per level, likewise (a near-tied bin maximum).

Activation sites for tests/helpers.pattern_grad_bar (forced masks / pool indices, recorded or
replayed through the model's ``forced`` dict as in oracle/daf_step.py), besides OracleATF's:
ida3 / ida4 / ida (the Conv1 ReLUs), m1_3 / m1_4 / m1_5 (the Convm1 ReLUs), mp3 / mp4 / mp5 (the
mask nets' 2x2 max-pools), club3a / club3b ... club5b (CLUB's two ReLUs, same then diff), ip1,
ip2.  Every site is visited source first, then target.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import roi as oroi
from oracle import rpn as orpn
from oracle.atf_step import OracleATF
from oracle.daf_step import CFG, SitePool, _GRL, _RoIAlignAvgCPU, _np, _t, forced_relu
from oracle.nms import nms as onms

VIEWS = ("conv3_s.", "conv3_t.", "conv34_s.", "conv34_t.", "conv45_s.", "conv45_t.")
POST = 256  # rois.size(1): the RCNN batch


def _image_da(dim):
    m = nn.Module()
    m.Conv1 = nn.Conv2d(dim, dim // 2, 1, bias=False)
    m.Conv2 = nn.Conv2d(dim // 2, 1, 1, bias=False)
    m.Convm1 = nn.Conv2d(dim, dim, 5, stride=3)
    m.Convm2 = nn.Conv2d(dim, dim, 3, stride=2)
    return m


def _club(dim):
    m = nn.Module()
    m.out_score = nn.Sequential(nn.Conv2d(2 * dim, dim, 3, stride=2), nn.ReLU(),
                                nn.Conv2d(dim, 128, 1), nn.ReLU())
    m.fc = nn.Linear(3 * 3 * 128, 2)
    return m


def subsample(keep, post, rng):
    """proposal_layer1.py:152-160 on a list of survivors, the draw replayed as
    rng.permutation(len(other))[:k]."""
    other = keep[int(post * 0.25):]
    first = keep[:int(post * 0.25)]
    k = min(len(other), int(post * 0.75))
    idx = rng.permutation(len(other))[:k] if len(other) else []
    return list(first) + [other[i] for i in idx]


class OraclePAATF(OracleATF):
    def __init__(self, n_classes=9, dropout=0.5):
        super().__init__(n_classes, dropout, "vgg16")
        self.RCNN_imageDA_3, self.RCNN_imageDA_4 = _image_da(256), _image_da(512)
        self.RCNN_imageDA = _image_da(512)
        self.club3, self.club4, self.club5 = _club(256), _club(512), _club(512)
        self.mp3, self.mp4, self.mp5 = (SitePool(self.forced, f"mp{i}") for i in (3, 4, 5))

    def load_from(self, model):
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()
              if not k.startswith(VIEWS)}
        self.load_state_dict(sd, strict=True)

    # -------------------------------------------------------------- the pieces
    def _gated(self, lvl, feat, label, arg=None, weight=0.1):
        m = {3: self.RCNN_imageDA_3, 4: self.RCNN_imageDA_4, 5: self.RCNN_imageDA}[lvl]
        pool = {3: self.mp3, 4: self.mp4, 5: self.mp5}[lvl]
        ida = "ida" if lvl == 5 else f"ida{lvl}"
        xx = _GRL.apply(feat, weight)
        z = m.Convm2(pool(forced_relu(self.forced, f"m1_{lvl}", m.Convm1(xx))))
        N, C, h, w = z.shape
        if arg is None:
            mx = F.adaptive_max_pool2d(z, (1, 1))
        else:
            mx = z.reshape(N, C, -1).gather(2, arg.long().to(z.device).view(N, C, 1)
                                            ).view(N, C, 1, 1)
        mask = torch.sigmoid(mx)
        p = torch.sigmoid(m.Conv2(forced_relu(self.forced, ida, m.Conv1(xx * mask))))
        return F.binary_cross_entropy(p, torch.full_like(p, float(label))), mask

    def _instance(self, x, label):
        m = self.RCNN_instanceDA
        x = _GRL.apply(x, 0.1)
        x = F.dropout(forced_relu(self.forced, "ip1", m.dc_ip1(x)), self.dropout, self.training)
        x = F.dropout(forced_relu(self.forced, "ip2", m.dc_ip2(x)), self.dropout, self.training)
        x = torch.sigmoid(m.clssifer(x))                                  # (R, 1)
        y = torch.full((x.shape[0],), float(label), dtype=x.dtype, device=x.device)   # (R,)
        return torch.abs(x - y).mean()                                    # (R, R) broadcast

    def _proto(self, lvl, feat, gt_rois, scale, cw, perm, argmax=None):
        """_RoIPooling(7, 7, scale) as a gather through its argmax (its own, from the fp32
        geometry and values of oracle.roi.roi_pool_fwd, or the device's), so it differentiates
        in the dtype of feat; then CLUB.forward (:125-147)."""
        club = {3: self.club3, 4: self.club4, 5: self.club5}[lvl]
        if argmax is None:
            argmax = oroi.roi_pool_fwd(_np(feat.float()), gt_rois, 7, 7, scale)[1]
        am = torch.as_tensor(np.asarray(argmax)).long().to(feat.device)
        p = feat.reshape(-1)[am.clamp(min=0)] * (am >= 0).to(feat.dtype)
        a, s = p * cw.detach(), p * (1 - cw.detach())
        x11, x22 = _GRL.apply(a, 0.1), _GRL.apply(s, 0.1)
        r_index = torch.as_tensor(np.asarray(perm)).long().to(feat.device)

        def score(x):
            x = forced_relu(self.forced, f"club{lvl}a", club.out_score[0](x))
            x = forced_relu(self.forced, f"club{lvl}b", club.out_score[2](x))
            return club.fc(x.view(x.size(0), -1))
        same = score(torch.cat((x11, x22), 1))
        diff = score(torch.cat((x11, x22[r_index]), 1))
        G = same.shape[0]
        one = torch.ones(G, dtype=torch.long, device=feat.device)
        return (F.nll_loss(F.log_softmax(same, 1), one)
                + F.nll_loss(F.log_softmax(diff, 1), torch.zeros_like(one)))

    def _target_keep(self, prob, bbox, info):
        """Every NMS survivor of the eval-mode RPN, in score order."""
        c = CFG
        scores, props = orpn.decode_clip(_np(prob.float()), _np(bbox.float()), _np(info),
                                         self.base_anchors, c["stride"])
        order = np.argsort(-scores[0], kind="stable")[:c["pre_test"]]
        keep = onms(np.concatenate([props[0][order], scores[0][order, None]], 1), c["nms"])
        return props[0][order][keep]

    # -------------------------------------------------------------- the step
    def forward(self, batch, rng, rois_override=None, arg_override=None, count=None,
                pp_override=None, own_keep=True):
        (im, info, gt, num, need, t_im, t_info, t_gt, t_num, t_need) = batch
        ov = rois_override or (None, None, None, None)
        args = arg_override or (None, None, None)
        pp = pp_override or (None, None, None)

        def row(a, i):
            return None if a is None or a.shape[0] <= i else a[i:i + 1]
        _, e3, e4 = self.splits
        base = self.RCNN_base(im)
        c3_t = self.RCNN_base_t[:e3](im)
        c4_t = self.RCNN_base_t[e3:e4](c3_t)
        base_t = self.RCNN_base_t[e4:](c4_t)
        rois_domain, props_s, l1c, l1b = self._rpn_train(base, gt, info, rng, ov[0])
        rois_domain_t, props_st, l2c, l2b = self._rpn_train(base_t, gt, info, rng, ov[1])

        def sample(r):
            r, rl, rt, riw, row = orpn.proposal_target(r, _np(gt.float()), rng, self.rcnn_cfg)
            return (r, _t(rl, base).view(-1).long(), _t(rt, base).view(-1, 4),
                    _t(riw, base).view(-1, 4), _t(row, base).view(-1, 4))
        r_s, rl_s, rt_s, riw_s, row_s = sample(rois_domain)
        r_t, rl_t, rt_t, riw_t, row_t = sample(rois_domain_t)

        def head(feat, rois):
            return self._head_to_tail(_RoIAlignAvgCPU.apply(feat, _t(rois, feat).view(-1, 5)))
        fc7_s, fc7_t = head(base, r_s), head(base_t, r_t)
        cls_s, box_s = self._det_losses(fc7_s, rl_s, rt_s.to(base.dtype), riw_s.to(base.dtype),
                                        row_s.to(base.dtype))
        cls_t, box_t = self._det_losses(fc7_t, rl_t, rt_t.to(base.dtype), riw_t.to(base.dtype),
                                        row_t.to(base.dtype))

        # the target: s branch, eval-mode RPN, post-NMS top-N := rois.size(1), subsampled
        t_c3, t_c4, t_base = self._backbone(t_im)
        _, _, t_prob, t_bbox = self._rpn(t_base)
        own = self._target_keep(t_prob, t_bbox, t_info.float()) \
            if own_keep or ov[2] is None else None
        kept = own if ov[2] is None else ov[2][0][:count]
        rows = subsample(list(range(len(kept))), POST, rng)
        t_rois = np.zeros((1, POST, 5), np.float32)
        t_rois[0, :len(rows), 1:] = kept[rows]
        fc7_tgt = head(t_base, t_rois)

        da3, cw3 = self._gated(3, c3_t, 1, row(args[0], 0))
        da4, cw4 = self._gated(4, c4_t, 1, row(args[1], 0))
        da5, cw5 = self._gated(5, base_t, 1, row(args[2], 0))
        t_da = sum(self._gated(lvl, f, 0, row(a, 1))[0]
                   for lvl, f, a in ((3, t_c3, args[0]), (4, t_c4, args[1]), (5, t_base, args[2])))
        da_ins = self._instance(fc7_t, 1)
        t_da_ins = self._instance(fc7_tgt, 0)

        G = int(num.view(-1)[0])
        gt_rois = np.concatenate([np.zeros((G, 1), np.float32), _np(gt.float())[0, :G, :4]], 1)
        pm = sum(self._proto(lvl, f, gt_rois, s, cw, rng.permutation(G), am)
                 for lvl, f, s, cw, am in ((3, c3_t, 1 / 4, cw3, pp[0]), (4, c4_t, 1 / 8, cw4, pp[1]),
                                           (5, base_t, 1 / 16, cw5, pp[2])))
        return dict(rpn_loss_cls=l1c + l2c, rpn_loss_box=l1b + l2b, RCNN_loss_cls=cls_s + cls_t,
                    RCNN_loss_bbox=box_s + box_t, DA_img_loss_cls=da3 + da4 + da5,
                    tgt_DA_img_loss_cls=t_da, DA_ins_loss_cls=da_ins, tgt_DA_ins_loss_cls=t_da_ins,
                    pm_loss=pm, rois=r_t, rois_label=_np(rl_t), t_rois=t_rois, t_kept=own,
                    props_s=props_s, props_st=props_st)


def total_loss(o, lamda=0.1, beta=0.1):
    """methods/PA_ATF/PA_ATF_train.py:405-408."""
    return (o["rpn_loss_cls"] + o["rpn_loss_box"] + o["RCNN_loss_cls"] + o["RCNN_loss_bbox"]
            + lamda * (o["DA_img_loss_cls"] + o["DA_ins_loss_cls"] + o["tgt_DA_img_loss_cls"]
                       + o["tgt_DA_ins_loss_cls"]) + beta * o["pm_loss"])
