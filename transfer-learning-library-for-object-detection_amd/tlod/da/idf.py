"""IDF (dual-branch VGG16 with domain attention maps and a separation loss) on the tlod
kernels — lib/IDF/{faster_rcnn,vgg16,net_utils}.py and the loss sum of
methods/IDF/IDF_train.py:223-339.

``vgg16(classes).create_architecture()`` then, once per image as in the reference,
``model(im_data, im_info, gt_boxes, num_boxes, gt_boxes_p, num_boxes_p, isSeparation=False,
target=False, eta=1.0)`` returns the reference's 20-tuple (faster_rcnn.py:189-191, 222-224):
rois, cls_prob, bbox_pred, rpn_loss_cls, rpn_loss_bbox, RCNN_loss_cls, RCNN_loss_bbox,
rois_label, domain_1, domain_2, domain_3, domain_ins, domain_1_b, domain_2_b, domain_3_b,
loss_se_2, loss_se_3, dist1, dist2, dist3.  In eval mode the first four arguments alone give
the main stack's detections (what tlod.eval.detect needs).

Two VGG16 stacks (``RCNN_base{1,2,3}`` and ``RCNN_base{1,2,3}_b``) run on the image.  At the
conv4_2 and conv5_3 outputs each stack's map gets a domain attention map (DAM: the channel
mean of its sigmoid, zeroed below its own image mean), the separation distance is taken
between the two maps weighted by the branch's DAM, and each map is multiplied by one plus the
other stack's DAM before the next block.  ``target=False`` trains the main detector on the
ground truth, ``target=True`` the ``_b`` / ``_t`` detector on the pseudo boxes; both calls run
the main stack's RPN proposals, proposal target and fc6 / fc7 for the instance discriminator.

Device ops (csrc/idf.hip, include/tlod_idf.h): one DAM launch pair per map, and one autograd
function (``_Separation``) for distance + both modulations, forward and backward one entry
each; the seven domain losses of an image are one launch each way (``_DomainLoss``; with
``ef=True`` the instance term is EFocalLoss, csrc/selftrain.hip).
``TLOD_FUSED_IDF=0`` takes the torch compositions of the same math instead.

The distance reduces over the channel axis with eps added to the difference — PyTorch 0.4's
pairwise_distance on a 4-D map, the release the reference pins (IDF section).

Scheduling (same math as the reference's two single-image calls, less work):
  * the frozen conv1 / conv2 prefix is one set of modules shared by both stacks (both sets of
    state_dict keys exist) and runs once per image;
  * in the target call the main stack's anchor target and RPN losses, which the reference
    computes against one all-zero box and discards, are not computed; its proposal target
    still samples against that zero box (256 background RoIs);
  * dist1 is only logged: it is computed without a graph.

Deviations, documented: ``fuse_3`` (vgg16.py:288) is constructed and never called: frozen
parameters.  The discriminator trunks (1x1 / strided 3x3 convs, training-mode batch norm,
dropout) are torch modules.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from ..config import cfg
from ..detector.losses import fused_losses, rcnn_losses, smooth_l1_loss
from ..detector.vgg16 import vgg16_base, vgg16_top
from ..roi_align import RoIAlignAvg
from ..roi_pool import _RoIPooling
from ..rpn.proposal import proposals_on_side_streams
from ..rpn.proposal_target import _ProposalTargetLayer
from ..rpn.rpn_head import _RPN
from .daf import grad_reverse

EPS = 1e-6        # pairwise_distance's eps
SE_WEIGHT = 0.001  # faster_rcnn.py:82, 98


def fused_idf():
    """TLOD_FUSED_IDF (default 1): the libtlod DAM / separation / domain-loss kernels; 0 = the
    torch compositions below (A/B comparison and tests)."""
    return _lib.env("TLOD_FUSED_IDF", "1") != "0"


# ------------------------------------------------------------------------------ torch forms
def dam_torch(x):
    """net_utils.py:300-306 with a threshold per image: (N, C, H, W) -> (N, H, W)."""
    avg = torch.sigmoid(x).mean(1)
    thr = avg.mean((1, 2), keepdim=True)
    return torch.where(avg < thr, torch.zeros_like(avg), avg)


def separation_torch(a, b, att_a, att_b, modulate=True):
    """(a_out, b_out, d (N, H, W), dist (N)); att_b None: weight 1."""
    diff = (a - b) if att_b is None else (a - b) * att_b.unsqueeze(1)
    d = torch.norm(diff + EPS, 2, dim=1)
    dist = d.mean((1, 2))
    if not modulate:
        return None, None, d, dist
    return a * (1 + att_b.unsqueeze(1)), b * (1 + att_a.unsqueeze(1)), d, dist


def focal_loss_torch(z, label, gamma):
    """FocalLoss(class_num=2, gamma) (net_utils.py:151-177) for one label."""
    P = F.softmax(z, dim=1).clamp(1e-6, 1)
    p = P[:, int(label)]
    return (-(1 - p).pow(gamma) * p.log()).mean()


def efocal_loss_torch(z, label, gamma):
    """EFocalLoss(class_num=2, gamma) (net_utils.py:73-102, IDF_train.py --ef) for one label:
    mean -exp(-gamma p) log p, alpha 1 and, unlike FocalLoss, no clamp."""
    p = F.softmax(z, dim=1)[:, int(label)]
    return (-torch.exp(-gamma * p) * p.log()).mean()


def domain_losses_torch(z_img, label_img, z_ins, label_ins, gamma, ef=False):
    y = torch.full((z_img.shape[0],), int(label_img), dtype=torch.long, device=z_img.device)
    ce = F.cross_entropy(z_img, y, reduction="none")
    ins = (efocal_loss_torch if ef else focal_loss_torch)(z_ins, label_ins, gamma)
    return torch.cat([ce, ins.view(1)])


# ------------------------------------------------------------------------------ device ops
def dam(x):
    """Domain attention map of every image of x (N, C, H, W) -> (N, H, W); no gradient."""
    x = x.detach()
    if not fused_idf():
        return dam_torch(x)
    _lib.require_cuda(x)
    x = x.contiguous().float()
    N, C, H, W = x.shape
    att = torch.empty((N, H, W), dtype=torch.float32, device=x.device)
    L = _lib.lib()
    ws = _lib.workspace(L.tlod_idf_dam_workspace_bytes(N, H, W), x.device, "idf_dam")
    _lib.check(L.tlod_idf_dam_f32(_lib.ptr(x), N, C, H, W, _lib.ptr(att), _lib.ptr(ws),
                                  ws.numel(), _lib.stream_of(x)), "idf_dam")
    return att


def _sep_fwd(a, b, att_a, att_b, modulate):
    N, C, H, W = a.shape
    a_out = torch.empty_like(a) if modulate else None
    b_out = torch.empty_like(b) if modulate else None
    d = torch.empty((N, H, W), dtype=torch.float32, device=a.device)
    dist = torch.empty(N, dtype=torch.float32, device=a.device)
    L = _lib.lib()
    ws = _lib.workspace(L.tlod_idf_sep_fwd_workspace_bytes(N, H, W), a.device, "idf_sep")
    _lib.check(L.tlod_idf_sep_fwd_f32(
        _lib.ptr(a), _lib.ptr(b), _lib.ptr(att_a), _lib.ptr(att_b), N, C, H, W, _lib.ptr(a_out),
        _lib.ptr(b_out), _lib.ptr(d), _lib.ptr(dist), _lib.ptr(ws), ws.numel(),
        _lib.stream_of(a)), "idf_sep_fwd")
    return a_out, b_out, d, dist


class _Separation(torch.autograd.Function):
    """(a, b, att_a, att_b) -> (a (1 + att_b), b (1 + att_a), dist (N)): tlod_idf_sep_fwd_f32 /
    _bwd_f32.  att carries no gradient (the reference detaches it)."""

    @staticmethod
    def forward(ctx, a, b, att_a, att_b):
        _lib.require_cuda(a, b, att_a, att_b)
        a_, b_ = a.detach().contiguous().float(), b.detach().contiguous().float()
        ta, tb = att_a.detach().contiguous().float(), att_b.detach().contiguous().float()
        assert a_.shape == b_.shape and ta.shape == tb.shape == (a_.shape[0],) + a_.shape[2:]
        a_out, b_out, d, dist = _sep_fwd(a_, b_, ta, tb, True)
        ctx.save_for_backward(a_, b_, ta, tb, d)
        ctx.set_materialize_grads(False)
        return a_out, b_out, dist

    @staticmethod
    def backward(ctx, g_a_out, g_b_out, g_dist):
        a, b, ta, tb, d = ctx.saved_tensors
        if g_a_out is None and g_b_out is None and g_dist is None:
            return None, None, None, None
        N, C, H, W = a.shape
        if (g_a_out is None) != (g_b_out is None):
            g_a_out = torch.zeros_like(a) if g_a_out is None else g_a_out
            g_b_out = torch.zeros_like(b) if g_b_out is None else g_b_out
        if g_a_out is not None:
            g_a_out, g_b_out = g_a_out.contiguous().float(), g_b_out.contiguous().float()
        g_dist = (torch.zeros(N, dtype=torch.float32, device=a.device) if g_dist is None
                  else g_dist.contiguous().float())
        g_a, g_b = torch.empty_like(a), torch.empty_like(b)
        _lib.check(_lib.lib().tlod_idf_sep_bwd_f32(
            _lib.ptr(a), _lib.ptr(b), _lib.ptr(ta), _lib.ptr(tb), _lib.ptr(d), _lib.ptr(g_a_out),
            _lib.ptr(g_b_out), _lib.ptr(g_dist), N, C, H, W, _lib.ptr(g_a), _lib.ptr(g_b),
            _lib.stream_of(a)), "idf_sep_bwd")
        return g_a, g_b, None, None


def separation(a, b, att_a, att_b):
    """The level's three outputs: a (1 + att_b), b (1 + att_a), dist (N) = the per-image mean
    over cells of ||(a - b) att_b + 1e-6||_2 (channel axis)."""
    if not fused_idf():
        a_out, b_out, _, dist = separation_torch(a, b, att_a, att_b)
        return a_out, b_out, dist
    return _Separation.apply(a, b, att_a, att_b)


@torch.no_grad()
def plain_distance(a, b):
    """dist1 (faster_rcnn.py:67): the unweighted distance, logged only — no graph."""
    if not fused_idf():
        return separation_torch(a, b, None, None, modulate=False)[3]
    _lib.require_cuda(a, b)
    return _sep_fwd(a.contiguous().float(), b.contiguous().float(), None, None, False)[3]


class _DomainLoss(torch.autograd.Function):
    """z_img (n, 2), z_ins (R, 2) -> (n + 1) losses: tlod_idf_domain_loss_f32 / _bwd_f32, or
    with ``ef`` tlod_idf_domain_loss_ef_f32 / _ef_bwd_f32 (include/tlod_selftrain.h)."""

    @staticmethod
    def forward(ctx, z_img, z_ins, label_img, label_ins, gamma, ef=False):
        _lib.require_cuda(z_img, z_ins)
        zi, zn = z_img.detach().contiguous().float(), z_ins.detach().contiguous().float()
        assert zi.dim() == 2 and zi.shape[1] == 2 and zn.dim() == 2 and zn.shape[1] == 2
        loss = torch.empty(zi.shape[0] + 1, dtype=torch.float32, device=zi.device)
        L = _lib.lib()
        _lib.check((L.tlod_idf_domain_loss_ef_f32 if ef else L.tlod_idf_domain_loss_f32)(
            _lib.ptr(zi), zi.shape[0], int(label_img), _lib.ptr(zn), zn.shape[0], int(label_ins),
            float(gamma), _lib.ptr(loss), _lib.stream_of(zi)), "idf_domain_loss")
        ctx.args = (int(label_img), int(label_ins), float(gamma), bool(ef))
        ctx.save_for_backward(zi, zn)
        return loss

    @staticmethod
    def backward(ctx, g):
        zi, zn = ctx.saved_tensors
        label_img, label_ins, gamma, ef = ctx.args
        g = g.contiguous().float()
        dzi, dzn = torch.empty_like(zi), torch.empty_like(zn)
        L = _lib.lib()
        _lib.check((L.tlod_idf_domain_loss_ef_bwd_f32 if ef else L.tlod_idf_domain_loss_bwd_f32)(
            _lib.ptr(zi), zi.shape[0], label_img, _lib.ptr(zn), zn.shape[0], label_ins, gamma,
            _lib.ptr(g), _lib.ptr(dzi), _lib.ptr(dzn), _lib.stream_of(zi)), "idf_domain_loss_bwd")
        return dzi, dzn, None, None, None, None


def domain_losses(z_img, label_img, z_ins, label_ins, gamma=3.0, ef=False):
    """The n two-logit cross entropies of z_img (n, 2) against label_img and the focal loss of
    z_ins (R, 2) against label_ins (``ef``: EFocalLoss, IDF_train.py:162-165) as one (n + 1)
    vector; weights not folded in."""
    if not fused_idf():
        return domain_losses_torch(z_img, label_img, z_ins, label_ins, gamma, ef)
    return _DomainLoss.apply(z_img, z_ins, label_img, label_ins, gamma, ef)


# ------------------------------------------------------------------------------ modules
class _NetD(nn.Module):
    """The image discriminators (vgg16.py:28-186): three conv + BatchNorm (training mode) +
    ReLU + dropout, global average pooling, Linear(128, 2).  netD_1 / netD_1_b: 1x1 convs
    256 -> 256 -> 128 -> 128; netD_2 / netD_3 and their _b twins: 3x3 stride-2 convs
    512 -> 512 -> 128 -> 128."""

    def __init__(self, cin, mid, k, stride):
        super().__init__()
        pad = k // 2
        self.conv1 = nn.Conv2d(cin, mid, k, stride=stride, padding=pad, bias=False)
        self.bn1 = nn.BatchNorm2d(mid)
        self.conv2 = nn.Conv2d(mid, 128, k, stride=stride, padding=pad, bias=False)
        self.bn2 = nn.BatchNorm2d(128)
        self.conv3 = nn.Conv2d(128, 128, k, stride=stride, padding=pad, bias=False)
        self.bn3 = nn.BatchNorm2d(128)
        self.fc = nn.Linear(128, 2)
        self.drop_p = 0.5   # F.dropout's default in the reference
        self.act_tap = None  # tests: a list receiving each ReLU output

    def _act(self, x):
        x = F.relu(x)
        if self.act_tap is not None:
            self.act_tap.append(x.detach().clone())
        return F.dropout(x, self.drop_p, self.training)

    def forward(self, x):
        x = self._act(self.bn1(self.conv1(x)))
        x = self._act(self.bn2(self.conv2(x)))
        x = self._act(self.bn3(self.conv3(x)))
        x = F.avg_pool2d(x, (x.size(2), x.size(3))).view(-1, 128)
        return self.fc(x)


class _NetDda(nn.Module):
    """netD_da (vgg16.py:225-237): Linear(feat_d, 100) BN ReLU dropout, Linear(100, 100) BN
    ReLU dropout, Linear(100, 2)."""

    def __init__(self, feat_d):
        super().__init__()
        self.fc1 = nn.Linear(feat_d, 100)
        self.bn1 = nn.BatchNorm1d(100)
        self.fc2 = nn.Linear(100, 100)
        self.bn2 = nn.BatchNorm1d(100)
        self.fc3 = nn.Linear(100, 2)
        self.drop_p = 0.5
        self.act_tap = None

    _act = _NetD._act

    def forward(self, x):
        x = self._act(self.bn1(self.fc1(x)))
        x = self._act(self.bn2(self.fc2(x)))
        return self.fc3(x)


class _FuseAdd(nn.Module):
    """fuse_add_3 (vgg16.py:188-197): constructed by the reference and never called.
    Parameters only (frozen), so a reference checkpoint loads with strict=True."""

    def __init__(self):
        super().__init__()
        self.conv3 = nn.Conv2d(512, 512, 3, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(512)
        self.conv1 = nn.Conv2d(512, 512, 1, bias=False)


class _fasterRCNN(nn.Module):
    """lib/IDF/faster_rcnn.py:25-252."""

    clip_norm = 0.0  # IDF_train.py has no clip_gradient (tlod.detector.train.default_clip)

    def __init__(self, classes, class_agnostic):
        super().__init__()
        self.classes = classes
        self.n_classes = len(classes)
        self.class_agnostic = class_agnostic
        self.RCNN_loss_cls = 0
        self.RCNN_loss_bbox = 0
        self.RCNN_rpn = _RPN(self.dout_base_model)
        self.RCNN_proposal_target = _ProposalTargetLayer(self.n_classes)
        self.RCNN_roi_pool = _RoIPooling(cfg.POOLING_SIZE, cfg.POOLING_SIZE, 1.0 / 16.0)
        self.RCNN_roi_align = RoIAlignAvg(cfg.POOLING_SIZE, cfg.POOLING_SIZE, 1.0 / 16.0)
        # the additional network for the pseudo-labelled target (faster_rcnn.py:43-50)
        self.RCNN_loss_cls_t = 0
        self.RCNN_loss_bbox_t = 0
        self.RCNN_rpn_t = _RPN(self.dout_base_model)
        self.RCNN_proposal_target_t = _ProposalTargetLayer(self.n_classes)
        self.RCNN_roi_pool_t = _RoIPooling(cfg.POOLING_SIZE, cfg.POOLING_SIZE, 1.0 / 16.0)
        self.RCNN_roi_align_t = RoIAlignAvg(cfg.POOLING_SIZE, cfg.POOLING_SIZE, 1.0 / 16.0)
        self.replay_rng = None  # tests: np.random-like object -> reference-exact sampling
        self.capture = None     # tests: dict receiving the proposals and the attention maps

    # ------------------------------------------------------------------ pieces
    def _pool(self, feat, rois, t=False):
        if cfg.POOLING_MODE == "align":
            return (self.RCNN_roi_align_t if t else self.RCNN_roi_align)(feat, rois)
        if cfg.POOLING_MODE == "pool":
            return (self.RCNN_roi_pool_t if t else self.RCNN_roi_pool)(feat, rois)
        raise ValueError(f"IDF pools with 'align' or 'pool', not {cfg.POOLING_MODE!r} "
                         "(faster_rcnn.py:133-136)")

    def _backbone(self, im_data, eta, heads=True):
        """Both stacks with the two attention / separation levels.  Returns the modulated
        conv5 maps of the main stack and the branch, the six image-discriminator logits (None
        without heads), (dist1, dist2, dist3) and the four attention maps."""
        z = self.RCNN_base1[:self.shared](im_data)  # frozen conv1 / conv2: one pass for both
        f1 = self.RCNN_base1[self.shared:](z)
        f1_b = self.RCNN_base1_b[self.shared:](z)
        dom = None
        if heads:
            dom = [self.netD_1(grad_reverse(f1, eta)), self.netD_1_b(f1_b)]
        dist1 = plain_distance(f1, f1_b) if heads else None
        f2 = self.RCNN_base2(f1)
        f2_b = self.RCNN_base2_b(f1_b)
        if heads:
            dom += [self.netD_2(grad_reverse(f2, eta)), self.netD_2_b(f2_b)]
        att2, att2_b = dam(f2), dam(f2_b)
        f2, f2_b, dist2 = separation(f2, f2_b, att2, att2_b)
        f3 = self.RCNN_base3(f2)
        f3_b = self.RCNN_base3_b(f2_b)
        if heads:
            dom += [self.netD_3(grad_reverse(f3, eta)), self.netD_3_b(f3_b)]
        att3, att3_b = dam(f3), dam(f3_b)
        f3, f3_b, dist3 = separation(f3, f3_b, att3, att3_b)
        return f3, f3_b, dom, (dist1, dist2, dist3), (att2, att2_b, att3, att3_b)

    @staticmethod
    def _flat(roi_data):
        rois, label, target, inside, outside = roi_data
        return (rois, label.view(-1).long(), target.view(-1, target.size(2)),
                inside.view(-1, inside.size(2)), outside.view(-1, outside.size(2)))

    def _head_losses(self, feat, cls_score, bbox_pred, sampled):
        """cls_prob, bbox_pred and the two RCNN losses of one detector (faster_rcnn.py:172-186,
        197-216)."""
        _, label, target, inside, outside = sampled
        bbox = bbox_pred(feat)
        if fused_losses():
            return rcnn_losses(cls_score(feat), bbox, label, target, inside, outside,
                               self.class_agnostic)
        if not self.class_agnostic:
            view = bbox.view(bbox.size(0), int(bbox.size(1) / 4), 4)
            bbox = torch.gather(view, 1, label.view(-1, 1, 1).expand(-1, 1, 4)).squeeze(1)
        score = cls_score(feat)
        return (F.softmax(score, 1), bbox, F.cross_entropy(score, label),
                smooth_l1_loss(bbox, target, inside, outside))

    # ---------------------------------------------------------------- eval (4 arguments)
    def _detect(self, im_data, im_info):
        batch_size = im_data.size(0)
        base, _, _, _, _ = self._backbone(im_data, 1.0, heads=False)
        _, _, prob, bbox = self.RCNN_rpn.head(base)
        rois = self.RCNN_rpn.RPN_proposal((prob.detach(), bbox.detach(), im_info.detach(),
                                           "TEST"))
        feat = self._head_to_tail(self._pool(base, rois.view(-1, 5)))
        cls_prob = F.softmax(self.RCNN_cls_score(feat), 1).view(batch_size, rois.size(1), -1)
        bbox_pred = self.RCNN_bbox_pred(feat).view(batch_size, rois.size(1), -1)
        return rois, cls_prob, bbox_pred, 0, 0, 0, 0, None

    # ---------------------------------------------------------------- forward
    def forward(self, im_data, im_info, gt_boxes, num_boxes, gt_boxes_p=None, num_boxes_p=None,
                isSeparation=False, target=False, eta=1.0):
        if not self.training:
            return self._detect(im_data, im_info)
        if gt_boxes_p is None:
            raise RuntimeError("IDF trains through the 6-argument forward (gt_boxes_p, "
                               "num_boxes_p); the 4-argument form is the eval-mode detector")
        batch_size = im_data.size(0)
        im_info = im_info.detach()
        gt_boxes = gt_boxes.detach()
        base, base_b, dom, dists, atts = self._backbone(im_data, eta)
        dist1, dist2, dist3 = dists

        # ---- RPN heads and proposal layers (side streams); the main stack's RPN losses feed
        # an output only in the source call
        rpn, rpn_t = self.RCNN_rpn, self.RCNN_rpn_t
        score, score_r, prob, bbox = rpn.head(base)
        jobs = [(prob.detach(), bbox.detach(), im_info, "TRAIN")]
        if target:
            gt_boxes_p = gt_boxes_p.detach()
            score_t, score_r_t, prob_t, bbox_t = rpn_t.head(base_b)
            jobs.append((prob_t.detach(), bbox_t.detach(), im_info, "TRAIN"))
        pending = proposals_on_side_streams(rpn.RPN_proposal, jobs)
        if target:
            rpn_loss_cls, rpn_loss_bbox, _ = rpn_t.losses(
                score_t, score_r_t, bbox_t, gt_boxes_p, im_info, num_boxes_p, rng=self.replay_rng)
        else:
            rpn_loss_cls, rpn_loss_bbox, _ = rpn.losses(
                score, score_r, bbox, gt_boxes, im_info, num_boxes, rng=self.replay_rng)
        props = pending.join()
        if self.capture is not None:  # keys s_* (source call) / t_* (target call)
            pre = "t_" if target else "s_"
            self.capture[pre + "rois"] = props[0].detach().clone()
            self.capture[pre + "att"] = tuple(a.detach().clone() for a in atts)
            if target:
                self.capture["t_rois_b"] = props[1].detach().clone()

        # ---- main stack: sampled RoIs -> fc6 / fc7 -> instance discriminator (:113-140)
        sampled = self._flat(self.RCNN_proposal_target(props[0], gt_boxes, num_boxes,
                                                       rng=self.replay_rng))
        rois = sampled[0]
        pooled_feat = self._head_to_tail(self._pool(base, rois.view(-1, 5)))
        domain_ins = self.netD_da(grad_reverse(pooled_feat, eta))

        if target:  # the _b / _t detector on the pseudo boxes (:144-191)
            sampled = self._flat(self.RCNN_proposal_target_t(props[1], gt_boxes_p, num_boxes_p,
                                                             rng=self.replay_rng))
            rois = sampled[0]
            feat_t = self._head_to_tail_t(self._pool(base_b, rois.view(-1, 5), t=True))
            cls_prob, bbox_pred, RCNN_loss_cls, RCNN_loss_bbox = self._head_losses(
                feat_t, self.RCNN_cls_score_t, self.RCNN_bbox_pred_t, sampled)
        else:
            cls_prob, bbox_pred, RCNN_loss_cls, RCNN_loss_bbox = self._head_losses(
                pooled_feat, self.RCNN_cls_score, self.RCNN_bbox_pred, sampled)
        cls_prob = cls_prob.view(batch_size, rois.size(1), -1)
        bbox_pred = bbox_pred.view(batch_size, rois.size(1), -1)
        # torch.mean over a batch of one (faster_rcnn.py:81, 97)
        dist2, dist3 = dist2.mean(), dist3.mean()
        return (rois, cls_prob, bbox_pred, rpn_loss_cls, rpn_loss_bbox, RCNN_loss_cls,
                RCNN_loss_bbox, sampled[1], dom[0], dom[2], dom[4], domain_ins, dom[1], dom[3],
                dom[5], SE_WEIGHT * dist2, SE_WEIGHT * dist3, dist1.mean(), dist2, dist3)

    @staticmethod
    def domain_terms(out, label, gamma=3.0, ef=False):
        """The seven unweighted domain losses of one call's outputs: CE of domain_1, domain_2,
        domain_3, domain_1_b, domain_2_b, domain_3_b against ``label`` and the focal loss of
        domain_ins (IDF_train.py:242-270, 302-327; ``ef``: EFocalLoss, :162-165)."""
        return domain_losses(torch.cat(out[8:11] + out[12:15], 0), label, out[11], label, gamma,
                             ef)

    @classmethod
    def total_loss(cls, out_s, out_t, separation=True, gamma=3.0, ef=False, target_gate=None):
        """IDF_train.py:229-335: the source detection losses, 0.5 x the target call's, 0.5 x
        every image-level cross entropy (label 0 source, 1 target), 0.25 x the two focal
        losses (``ef``: EFocalLoss) and, when ``separation``, the four loss_se terms.
        target_gate: a device scalar (0 or 1) multiplied into the target call's four detection
        losses (tlod.detector.train.idf_selftrain_step: an image without a pseudo label)."""
        scalars = list(out_s[3:7]) + list(out_t[3:7])
        if target_gate is not None:
            gate = target_gate.reshape(()).to(out_t[3].dtype)
            scalars[4:] = [x.reshape(()) * gate for x in scalars[4:]]
        weights = [1.0] * 4 + [0.5] * 4
        if separation:
            scalars += [out_s[15], out_s[16], out_t[15], out_t[16]]
            weights += [1.0] * 4
        t = torch.cat([torch.stack([x.reshape(()) for x in scalars]),
                       cls.domain_terms(out_s, 0, gamma, ef),
                       cls.domain_terms(out_t, 1, gamma, ef)])
        return _dot(t, weights + ([0.5] * 6 + [0.25]) * 2)

    def _init_weights(self):
        """faster_rcnn.py:226-248 (normal_init, truncated=False)."""
        def normal_init(m, mean, std):
            m.weight.data.normal_(mean, std)
            m.bias.data.zero_()
        for rpn in (self.RCNN_rpn, self.RCNN_rpn_t):
            normal_init(rpn.RPN_Conv, 0, 0.01)
            normal_init(rpn.RPN_cls_score, 0, 0.01)
            normal_init(rpn.RPN_bbox_pred, 0, 0.01)
        normal_init(self.RCNN_cls_score, 0, 0.01)
        normal_init(self.RCNN_bbox_pred, 0, 0.001)
        normal_init(self.RCNN_cls_score_t, 0, 0.01)
        normal_init(self.RCNN_bbox_pred_t, 0, 0.001)

    def create_architecture(self):
        self._init_modules()
        self._init_weights()


_W = {}


def _dot(t, weights):
    """sum_i weights[i] t[i] with a cached device weight vector (one dot product)."""
    key = (str(t.device), tuple(float(w) for w in weights))
    w = _W.get(key)
    if w is None:
        w = _W[key] = torch.tensor(key[1], dtype=t.dtype, device=t.device)
    return torch.dot(t, w)


class vgg16(_fasterRCNN):
    """lib/IDF/vgg16.py:241-326 (random init: the pretrained caffe weights are external)."""

    shared = 10  # features[:10] (conv1_x, conv2_x) are frozen in both stacks (:294-296)

    def __init__(self, classes, pretrained=False, class_agnostic=False):
        self.dout_base_model = 512
        self.pretrained = pretrained
        self.class_agnostic = class_agnostic
        _fasterRCNN.__init__(self, classes, class_agnostic)

    def _init_modules(self):
        # no tap reads a map in front of a max-pool (the taps are conv3_2, conv4_2, conv5_3),
        # so all four pools fold into their convs
        main = list(vgg16_base(fuse_pools=(1, 2, 3, 4)))
        branch = list(vgg16_base(fuse_pools=(1, 2, 3, 4)))
        branch[:self.shared] = main[:self.shared]  # one frozen prefix, both key sets
        self.RCNN_base1 = nn.Sequential(*main[:14])
        self.RCNN_base2 = nn.Sequential(*main[14:21])
        self.RCNN_base3 = nn.Sequential(*main[21:])
        self.netD_1 = _NetD(256, 256, 1, 1)
        self.netD_2 = _NetD(512, 512, 3, 2)
        self.netD_3 = _NetD(512, 512, 3, 2)
        self.netD_da = _NetDda(4096)
        self.RCNN_base1_b = nn.Sequential(*branch[:14])
        self.RCNN_base2_b = nn.Sequential(*branch[14:21])
        self.RCNN_base3_b = nn.Sequential(*branch[21:])
        self.netD_1_b = _NetD(256, 256, 1, 1)
        self.netD_2_b = _NetD(512, 512, 3, 2)
        self.netD_3_b = _NetD(512, 512, 3, 2)
        self.fuse_3 = _FuseAdd()
        for p in self.fuse_3.parameters():
            p.requires_grad = False
        self.RCNN_top = vgg16_top()
        self.RCNN_top_t = vgg16_top()
        nbox = 4 if self.class_agnostic else 4 * self.n_classes
        self.RCNN_cls_score = nn.Linear(4096, self.n_classes)
        self.RCNN_bbox_pred = nn.Linear(4096, nbox)
        self.RCNN_cls_score_t = nn.Linear(4096, self.n_classes)
        self.RCNN_bbox_pred_t = nn.Linear(4096, nbox)

    def train(self, mode=True):
        """fuse_3's BatchNorm is never called: keep its running statistics untouched."""
        nn.Module.train(self, mode)
        self.fuse_3.eval()
        return self

    def _head_to_tail(self, pool5):
        return self.RCNN_top(pool5.view(pool5.size(0), -1))

    def _head_to_tail_t(self, pool5):
        return self.RCNN_top_t(pool5.view(pool5.size(0), -1))
