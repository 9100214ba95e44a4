"""PT-MAF (MAF with RPN-masked image discriminators and a distilled source-only teacher) on
the tlod kernels — lib/PT_MAF/{faster_rcnn,faster_rcnn_kd,rpn_cls,DA,drm}.py and the training
step of methods/PT_MAF/PT_MAF_train.py:434-464.

``vgg16(classes).create_architecture()`` then ``model(<MAF's ten arguments>, T, high, low,
alpha, beta, gamma)`` returns the reference's 14-tuple (faster_rcnn.py:410-411): MAF's 12
values, then kd_rpn_prob (1, 2, A*H, W) and kd_cls_prob (256, n_classes).

Beyond MAF, per image (source, then target):
  * the RPN's object probabilities give a foreground map f = t > max(t) * high and a
    background map b = t < max(t) * low, t = max over anchors (faster_rcnn.py:132-148,
    232-248), and the ratios sum f / (sum f + sum b), sum b / (sum f + sum b): one launch
    (tlod_fgbg_maps_f32);
  * six image discriminators, RCNN_imageDA{_3,_4,}_{f,b}, each MAF's head behind a gradient
    reversal scaled by 0.1 * the image's own ratio (a device scalar), each with the NLL of
    its domain label over its map's cells only: one forward and one backward launch for all
    of them (tlod_masked_nll2_f32);
  * a frozen source-only teacher sees the source image and the student's sampled RoIs; the
    KL between the temperature-softened student and teacher outputs — RoI class scores over
    the foreground RoIs, two-way RPN scores over the ground-truth cells — is added to the
    loss (tlod_kd_kl_f32, tlod_gt_cell_mask_f32).

Decisions where the reference is loose:
  * a term whose map is empty is 0 with a 0 gradient (with low = 0.1 the b map of an
    untrained RPN is empty; current torch returns NaN for an all-ignored nll_loss, the torch
    the reference was written for returned 0);
  * the source conv3 b term reads conv3_score_f (faster_rcnn.py:298), so RCNN_imageDA_3_b
    learns from the target image only — reproduced, see _img_terms;
  * the anchor count is the model's own A (the training script hard-codes 12);
  * the teacher runs under no_grad in eval mode and never reaches the optimizer;
  * the KD term differentiates the student's RPN scores after the forward has returned, so
    the early RPN backward of tlod.da.daf is never used here.
Nothing in the forward or the step synchronises with the host.
"""
import torch
import torch.nn.functional as F

from .. import _lib
from ..detector.losses import fused_losses, smooth_l1_loss, weighted_loss_sum
from ..rpn.proposal import proposals_on_side_streams
from . import maf
from .daf import _ImageDA as _DAFImageDA
from .maf import instance_label_w


# ------------------------------------------------------------------------------ device ops
def fgbg_maps(prob, A, high, low):
    """prob (B, 2A, H, W) RPN probabilities -> (f, b, stats): f = t > m * high, b = t < m * low
    as float (B, H, W) 0 / 1 maps with t = max over the A object channels and m = max t per
    image; stats (B, 5) = [m, sum f, sum b, ratio_f, ratio_b].  No gradient (the reference's
    maps come out of torch.where on constants)."""
    prob = prob.detach()
    B, twoA, H, W = prob.shape
    assert twoA == 2 * A
    if not fused_losses():
        t = prob[:, A:].max(1)[0]
        m = t.amax((1, 2))
        f = torch.where(t.gt((m * high).view(-1, 1, 1)), torch.full_like(t, 1),
                        torch.full_like(t, 0))
        b = torch.where(t.lt((m * low).view(-1, 1, 1)), torch.full_like(t, 1),
                        torch.full_like(t, 0))
        sf, sb = f.sum((1, 2)), b.sum((1, 2))
        return f, b, torch.stack([m, sf, sb, sf / (sf + sb), sb / (sf + sb)], 1)
    _lib.require_cuda(prob)
    prob = prob.contiguous().float()
    f = torch.empty((B, H, W), dtype=torch.float32, device=prob.device)
    b = torch.empty_like(f)
    stats = torch.empty((B, 5), dtype=torch.float32, device=prob.device)
    _lib.check(_lib.lib().tlod_fgbg_maps_f32(_lib.ptr(prob), B, A, H, W, float(high), float(low),
                                             _lib.ptr(f), _lib.ptr(b), _lib.ptr(stats),
                                             _lib.stream_of(prob)), "fgbg_maps")
    return f, b, stats


def _ptr_array(tensors):
    return (_lib.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class MaskedNLL2Function(torch.autograd.Function):
    """K (score, map) pairs of one H x W level -> the (K, B) per-image masked NLLs:
    tlod_masked_nll2_f32 / _bwd_f32, one launch each way."""

    @staticmethod
    def forward(ctx, need, K, *t):
        _lib.require_cuda(*t)
        scores = [x.detach().contiguous().float() for x in t[:K]]
        maps = [x.detach().contiguous().float() for x in t[K:]]
        B, two, H, W = scores[0].shape
        assert two == 2 and len(maps) == K
        assert all(s.shape == (B, 2, H, W) for s in scores), [s.shape for s in scores]
        assert all(m.shape == (B, H, W) for m in maps), [m.shape for m in maps]
        need = need.detach().to(scores[0].device).contiguous().float().view(-1)
        assert need.numel() == B
        out = torch.empty((2, K, B), dtype=torch.float32, device=need.device)  # loss, count
        _lib.check(_lib.lib().tlod_masked_nll2_f32(
            _ptr_array(scores), _ptr_array(maps), K, _lib.ptr(need), B, H, W, _lib.ptr(out[0]),
            _lib.ptr(out[1]), _lib.stream_of(need)), "masked_nll2")
        ctx.K = K
        ctx.save_for_backward(need, out, *scores, *maps)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        need, out, *t = ctx.saved_tensors
        K = ctx.K
        scores, maps = t[:K], t[K:]
        B, _, H, W = scores[0].shape
        g = g.contiguous().float()
        d = [torch.empty_like(s) for s in scores]
        _lib.check(_lib.lib().tlod_masked_nll2_bwd_f32(
            _ptr_array(scores), _ptr_array(maps), K, _lib.ptr(need), B, H, W, _lib.ptr(g),
            _lib.ptr(out[1]), _ptr_array(d), _lib.stream_of(need)), "masked_nll2_bwd")
        return (None, None, *d, *([None] * K))


def masked_nll2(need, pairs):
    """pairs: [(score (B, 2, H, W), map (B, H, W))] -> (K, B): for pair k and image b the mean
    over map == 1 of -log_softmax(score, 1)[need[b]] (nll_loss with the cells off the map
    ignored); 0, with a 0 gradient, where the map is empty."""
    scores, maps = [p[0] for p in pairs], [p[1] for p in pairs]
    if fused_losses():
        return MaskedNLL2Function.apply(need, len(pairs), *scores, *maps)
    rows = []
    for s, m in pairs:
        lab = need.view(-1, 1, 1, 1).to(s.device).long().expand(-1, 1, *s.shape[2:])
        sel = F.log_softmax(s, 1).gather(1, lab).squeeze(1)
        rows.append(-(sel * m).sum((1, 2)) / m.sum((1, 2)).clamp(min=1))
    return torch.stack(rows)


class KDKLFunction(torch.autograd.Function):
    """sum_r w_r KL(softmax(student_r / T) || softmax(teacher_r / T)) / (sum w + 1) over
    strided rows: tlod_kd_kl_f32 / _bwd_f32.  Gradient for the student only."""

    @staticmethod
    def forward(ctx, student, teacher, weight, R, C, rs, cs, wmod, T):
        _lib.require_cuda(student, teacher, weight)
        s, t = student.detach().contiguous().float(), teacher.detach().contiguous().float()
        w = weight.detach().contiguous().float().view(-1)
        assert s.numel() == t.numel() == R * C and (R - 1) * rs + (C - 1) * cs < s.numel()
        assert w.numel() == wmod and 0 < wmod <= R
        out = torch.empty(2, dtype=torch.float32, device=s.device)  # loss, sum w + 1
        _lib.check(_lib.lib().tlod_kd_kl_f32(_lib.ptr(s), _lib.ptr(t), _lib.ptr(w), R, C, rs, cs,
                                             wmod, float(T), _lib.ptr(out), _lib.stream_of(s)),
                   "kd_kl")
        ctx.meta = (R, C, rs, cs, wmod, float(T), student.shape)
        ctx.save_for_backward(s, t, w, out)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        s, t, w, out = ctx.saved_tensors
        R, C, rs, cs, wmod, T, shape = ctx.meta
        g = g.reshape(1).contiguous().float()
        d = torch.empty_like(s)  # R * C = numel: every element is written
        _lib.check(_lib.lib().tlod_kd_kl_bwd_f32(_lib.ptr(s), _lib.ptr(t), _lib.ptr(w), R, C, rs,
                                                 cs, wmod, T, _lib.ptr(g), _lib.ptr(out),
                                                 _lib.ptr(d), _lib.stream_of(s)), "kd_kl_bwd")
        return (d.view(shape),) + (None,) * 8


def kd_kl_rows(student, teacher, weight, T):
    """student / teacher (R, C) class scores, weight (R): the RoI part of the KD loss."""
    R, C = student.shape
    if fused_losses():
        return KDKLFunction.apply(student, teacher, weight, R, C, C, 1, R, T)
    p1, p2 = F.softmax(student / T, 1), F.softmax(teacher.detach() / T, 1)
    return (weight.view(-1, 1) * p1 * torch.log(p1 / p2)).sum() / (weight.sum() + 1)


def kd_kl_rpn(student, teacher, g, T):
    """student / teacher (1, 2, A*H, W) two-way RPN scores, g (H, W) cell weights shared by
    the A anchors: the RPN part of the KD loss."""
    assert student.shape[:2] == (1, 2) and student.shape == teacher.shape
    H, W = g.shape
    AHW = student.shape[2] * student.shape[3]
    assert AHW % (H * W) == 0 and student.shape[3] == W
    if fused_losses():
        return KDKLFunction.apply(student, teacher, g, AHW, 2, 1, AHW, H * W, T)
    A = AHW // (H * W)
    p1 = F.softmax(student / T, 1).view(1, 2 * A, H, W)
    p2 = F.softmax(teacher.detach() / T, 1).view(1, 2 * A, H, W)
    return (g * p1 * torch.log(p1 / p2)).sum() / (g.sum() + 1)


def gt_cell_mask(gt_boxes, num_boxes, H, W):
    """faster_rcnn_kd.py:58-65 without its host loops and .item(): gt_boxes (1, G, 5),
    num_boxes a device tensor -> g (H, W) float, 1 on the stride-16 cells inside one of the
    first num_boxes boxes."""
    _lib.require_cuda(gt_boxes, num_boxes)
    gt = gt_boxes.detach().contiguous().float()
    assert gt.dim() == 3 and gt.shape[0] == 1 and gt.shape[2] == 5
    nb = num_boxes.detach().to(gt.device).contiguous().long().view(-1)
    g = torch.empty((H, W), dtype=torch.float32, device=gt.device)
    _lib.check(_lib.lib().tlod_gt_cell_mask_f32(_lib.ptr(gt), _lib.ptr(nb), gt.shape[1], H, W,
                                                _lib.ptr(g), _lib.stream_of(gt)), "gt_cell_mask")
    return g


# ------------------------------------------------------------------------------ modules
class GRLayerScaled(torch.autograd.Function):
    """lib/PT_MAF/faster_rcnn.py:24-35: identity forward; backward -(0.1 * ratio[b]) * grad,
    ratio a (B,) device tensor — one scale per image, so the batched source + target pass
    carries each image's own ratio."""

    @staticmethod
    def forward(ctx, x, ratio):
        ctx.save_for_backward(ratio)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        (ratio,) = ctx.saved_tensors
        return g.neg() * (ratio * 0.1).view(-1, *([1] * (g.dim() - 1))), None


def grad_reverse_scaled(x, ratio):
    return GRLayerScaled.apply(x, ratio.detach().view(-1))


class _ImageDA(_DAFImageDA):
    """lib/PT_MAF/faster_rcnn.py:40-54: MAF's conv5 head behind the ratio-scaled GRL."""

    def score(self, x, ratio):
        return self.Conv2(self.Conv1(grad_reverse_scaled(x, ratio)))

    def forward(self, x, need_backprop, ratio):
        x = self.score(x, ratio)
        return x, maf.image_label(x, need_backprop)


class _ImageDA_drm(maf._ImageDA_drm):
    """lib/PT_MAF/faster_rcnn.py:56-77: MAF's DRM head behind the ratio-scaled GRL."""

    def score(self, x, ratio):
        return self.Conv2(self.Conv1(self.DRM(grad_reverse_scaled(x, ratio))))

    def forward(self, x, need_backprop, ratio):
        x = self.score(x, ratio)
        return x, maf.image_label(x, need_backprop)


_TERM_WEIGHTS = {}


def _term_weights(rows, device):
    """A cached device matrix of per-term weights (the alpha / beta / gamma sums as one
    multiply + one sum instead of a kernel per product and addition)."""
    key = (str(device), rows)
    w = _TERM_WEIGHTS.get(key)
    if w is None:
        w = _TERM_WEIGHTS[key] = torch.tensor(rows, dtype=torch.float32, device=device)
    return w


class _fasterRCNN(maf._fasterRCNN):
    """lib/PT_MAF/faster_rcnn.py:79-411 on MAF's detector plumbing."""

    def __init__(self, classes, class_agnostic):
        super().__init__(classes, class_agnostic)
        del self.RCNN_imageDA_3, self.RCNN_imageDA_4, self.RCNN_imageDA
        self.RCNN_imageDA_3_f = _ImageDA_drm(256, 64, 4)
        self.RCNN_imageDA_4_f = _ImageDA_drm(512, 256, 2)
        self.RCNN_imageDA_f = _ImageDA(self.dout_base_model)
        self.RCNN_imageDA_3_b = _ImageDA_drm(256, 64, 4)
        self.RCNN_imageDA_4_b = _ImageDA_drm(512, 256, 2)
        self.RCNN_imageDA_b = _ImageDA(self.dout_base_model)
        self.kd_scores = None  # (source RPN scores, source RoI class scores), on the graph

    @property
    def num_anchor(self):
        return self.RCNN_rpn.nc_score_out // 2

    # ---------------------------------------------------------------- eval (4 arguments)
    def _detect(self, im_data, im_info, gt_boxes, num_boxes):
        """Test-time detector (what tlod.eval.detect.im_detect calls): the source-only
        forward of tlod.detector.faster_rcnn in eval mode, no domain heads."""
        batch_size = im_data.size(0)
        base = self.RCNN_base(im_data)
        _, _, prob, bbox = self.RCNN_rpn.head(base)
        rois = self.RCNN_rpn.RPN_proposal((prob.detach(), bbox.detach(), im_info.detach(),
                                           "TEST"))
        feat = self._head_to_tail(self._pool(base, rois.view(-1, 5)))
        cls_prob = F.softmax(self.RCNN_cls_score(feat), 1).view(batch_size, rois.size(1), -1)
        bbox_pred = self.RCNN_bbox_pred(feat).view(batch_size, rois.size(1), -1)
        return rois, cls_prob, bbox_pred, 0, 0, 0, 0, None

    # ---------------------------------------------------------------- image DA terms
    def _img_terms(self, feats, f, b, stats, need, source, target):
        """The masked NLLs of the six heads over one backbone pass of B images: feats =
        (conv3, conv4, conv5) features, f / b (B, H, W) maps, stats (B, 5).  source /
        target: the batch entries that are a source / a target image (None: absent).
        Returns the (K, B) losses and, for the source and the target domain, the rows of
        that matrix holding the domain's terms in the order [c3_f, c3_b, c4_f, c4_b, c5_f,
        c5_b] (the c3_b row is None for an absent domain)."""
        ratio_f, ratio_b = stats[:, 3], stats[:, 4]
        s3f = self.RCNN_imageDA_3_f.score(feats[0], ratio_f)
        s4f = self.RCNN_imageDA_4_f.score(feats[1], ratio_f)
        s4b = self.RCNN_imageDA_4_b.score(feats[1], ratio_b)
        s5f = self.RCNN_imageDA_f.score(feats[2], ratio_f)
        s5b = self.RCNN_imageDA_b.score(feats[2], ratio_b)
        assert s3f.shape[2:] == f.shape[1:] == s4f.shape[2:] == s5f.shape[2:], \
            (s3f.shape, s4f.shape, s5f.shape, f.shape)
        pairs = [(s3f, f), (s4f, f), (s4b, b), (s5f, f), (s5b, b)]
        # The source image's conv3 b term reads conv3_score_f (faster_rcnn.py:298:
        # log_softmax(conv3_score_f) under the b labels), so RCNN_imageDA_3_b gets gradient
        # from target images only; its pass is skipped when the batch holds no target image.
        src3b = tgt3b = None
        if source is not None:
            src3b = len(pairs)
            pairs.append((s3f, b))
        if target is not None:
            tgt3b = len(pairs)
            pairs.append((self.RCNN_imageDA_3_b.score(feats[0], ratio_b), b))
        losses = masked_nll2(need, pairs)
        return losses, [(0, src3b, 1, 2, 3, 4), (0, tgt3b, 1, 2, 3, 4)]

    @staticmethod
    def _img_sum(losses, rows, image, alpha, beta, gamma):
        """alpha (c3_f + c3_b) + beta (c4_f + c4_b) + gamma (c5_f + c5_b) of batch entry
        ``image`` (faster_rcnn.py:329, 398)."""
        K, B = losses.shape
        w = [[0.0] * B for _ in range(K)]
        for k, c in zip(rows, (alpha, alpha, beta, beta, gamma, gamma)):
            w[k][image] = float(c)
        return (losses * _term_weights(tuple(map(tuple, w)), losses.device)).sum()

    # ---------------------------------------------------------------- forward
    def forward(self, im_data, im_info, gt_boxes, num_boxes, need_backprop=None,
                tgt_im_data=None, tgt_im_info=None, tgt_gt_boxes=None, tgt_num_boxes=None,
                tgt_need_backprop=None, T=3.0, high=0.7, low=0.1, alpha=1.0, beta=1.0,
                gamma=1.0):
        if tgt_im_data is None:
            if self.training:
                raise RuntimeError("PT-MAF trains on a source and a target image: the "
                                   "4-argument forward is the eval-mode detector")
            return self._detect(im_data, im_info, gt_boxes, num_boxes)
        batch_size = im_data.size(0)
        im_info = im_info.detach()
        gt_boxes = gt_boxes.detach()
        A = self.num_anchor
        same = (im_data.shape == tgt_im_data.shape) and batch_size == 1
        rpn = self.RCNN_rpn
        if same:
            feats = [self._backbone(torch.cat([im_data, tgt_im_data], 0))]
            score2, score_r2, prob2, bbox2 = rpn.head(feats[0][2])
            s_score, s_score_r, s_prob, s_bbox = score2[:1], score_r2[:1], prob2[:1], bbox2[:1]
            t_prob, t_bbox = prob2[1:], bbox2[1:]
            maps = [fgbg_maps(prob2, A, high, low)]
        else:
            feats = [self._backbone(im_data), self._backbone(tgt_im_data)]
            s_score, s_score_r, s_prob, s_bbox = rpn.head(feats[0][2])
            _, _, t_prob, t_bbox = rpn.head(feats[1][2])
            maps = [fgbg_maps(s_prob, A, high, low), fgbg_maps(t_prob, A, high, low)]

        # proposal layers on side streams, overlapping the anchor target / RPN losses; no
        # early RPN backward: the KD loss differentiates s_score_r after this returns
        pending = proposals_on_side_streams(rpn.RPN_proposal, [
            (s_prob.detach(), s_bbox.detach(), im_info, "TRAIN"),
            (t_prob.detach(), t_bbox.detach(), tgt_im_info.detach(), "TEST")])
        rpn_loss_cls, rpn_loss_bbox, _ = rpn.losses(s_score, s_score_r, s_bbox, gt_boxes, im_info,
                                                    num_boxes, rng=self.replay_rng)

        # image-level DA on conv3 / conv4 / conv5 under the f / b maps (independent of the
        # proposals: runs while the side streams do the NMS)
        if same:
            f2, b2, stats2 = maps[0]
            need2 = torch.cat([need_backprop.view(-1)[:1], tgt_need_backprop.view(-1)[:1]]).float()
            losses, (rows_s, rows_t) = self._img_terms(feats[0], f2, b2, stats2, need2, 0, 1)
            DA_img_loss_cls = self._img_sum(losses, rows_s, 0, alpha, beta, gamma)
            tgt_DA_img_loss_cls = self._img_sum(losses, rows_t, 1, alpha, beta, gamma)
        else:
            (f_s, b_s, st_s), (f_t, b_t, st_t) = maps
            l_s, (rows_s, _) = self._img_terms(feats[0], f_s, b_s, st_s, need_backprop, 0, None)
            l_t, (_, rows_t) = self._img_terms(feats[1], f_t, b_t, st_t, tgt_need_backprop, None, 0)
            DA_img_loss_cls = self._img_sum(l_s, rows_s, 0, alpha, beta, gamma)
            tgt_DA_img_loss_cls = self._img_sum(l_t, rows_t, 0, alpha, beta, gamma)

        rois, tgt_rois = pending.join()
        if self.capture is not None:
            if same:
                cap = (f2[:1], b2[:1], f2[1:], b2[1:], stats2[:1], stats2[1:])
            else:
                cap = (f_s, b_s, f_t, b_t, st_s, st_t)
            self.capture.update(s_rois=rois.detach().clone(), t_rois=tgt_rois.detach().clone(),
                                maps=tuple(x.detach().clone() for x in cap[:4]),
                                stats=tuple(x.detach().clone() for x in cap[4:]),
                                s_prob=s_prob.detach().clone(), t_prob=t_prob.detach().clone())

        rois, rois_label, rois_target, rois_inside_ws, rois_outside_ws = \
            self.RCNN_proposal_target(rois, gt_boxes, num_boxes, rng=self.replay_rng)
        rois_label = rois_label.view(-1).long()
        rois_target = rois_target.view(-1, rois_target.size(2))
        rois_inside_ws = rois_inside_ws.view(-1, rois_inside_ws.size(2))
        rois_outside_ws = rois_outside_ws.view(-1, rois_outside_ws.size(2))

        n_s = rois.size(1)
        if same:
            t_rois = tgt_rois.view(-1, 5).clone()
            t_rois[:, 0] = 1.0  # the target image is batch entry 1 of the batched features
            feat2 = self._head_to_tail(self._pool(feats[0][2],
                                                  torch.cat([rois.view(-1, 5), t_rois], 0)))
        else:
            feat2 = torch.cat([self._head_to_tail(self._pool(feats[0][2], rois.view(-1, 5))),
                               self._head_to_tail(self._pool(feats[1][2], tgt_rois.view(-1, 5)))], 0)
        pooled_feat = feat2[:n_s]

        # detection head: one cls_score GEMM over source + target rows (per-row op)
        cls_score2 = self.RCNN_cls_score(feat2)
        cls_prob2 = F.softmax(cls_score2, 1)
        cls_score = cls_score2[:n_s]
        bbox_pred = self.RCNN_bbox_pred(pooled_feat)
        if not self.class_agnostic:
            view = bbox_pred.view(bbox_pred.size(0), int(bbox_pred.size(1) / 4), 4)
            bbox_pred = torch.gather(view, 1, rois_label.view(-1, 1, 1).expand(-1, 1, 4)).squeeze(1)
        RCNN_loss_cls = F.cross_entropy(cls_score, rois_label)
        RCNN_loss_bbox = smooth_l1_loss(bbox_pred, rois_target, rois_inside_ws, rois_outside_ws)
        cls_prob = cls_prob2[:n_s].view(batch_size, n_s, -1)
        bbox_pred = bbox_pred.view(batch_size, n_s, -1)

        # instance DA on [fc7 || cls_prob], MAF's head unchanged (faster_rcnn.py:331-336,
        # 401-408)
        n_t = feat2.shape[0] - n_s
        dom = torch.cat([need_backprop.view(-1)[:1].long().expand(n_s),
                         tgt_need_backprop.view(-1)[:1].long().expand(n_t)])
        logits, _ = self.RCNN_instanceDA(torch.cat((feat2, cls_prob2), 1), dom)
        DA_ins_loss_cls = F.cross_entropy(logits[:n_s], instance_label_w(n_s, need_backprop))
        tgt_DA_ins_loss_cls = F.cross_entropy(logits[n_s:],
                                              instance_label_w(n_t, tgt_need_backprop))

        # distillation: the probabilities the reference returns, and the scores the fused KD
        # loss reads (kd_loss), both still on the graph
        self.kd_scores = (s_score_r, cls_score)
        kd_rpn_prob = F.softmax(s_score_r / T, 1)
        kd_cls_prob = F.softmax(cls_score / T, 1)
        return (rois, cls_prob, bbox_pred, rpn_loss_cls, rpn_loss_bbox, RCNN_loss_cls,
                RCNN_loss_bbox, rois_label, DA_img_loss_cls, DA_ins_loss_cls, tgt_DA_img_loss_cls,
                tgt_DA_ins_loss_cls, kd_rpn_prob, kd_cls_prob)

    @staticmethod
    def total_loss(out, lamda=0.1, kd=None):
        """methods/PT_MAF/PT_MAF_train.py:453-456 (kd None: the sum without the KD term)."""
        terms = tuple(out[3:7]) + tuple(out[8:12])
        weights = (1, 1, 1, 1, lamda, lamda, lamda, lamda)
        if kd is not None:
            terms, weights = terms + (kd,), weights + (1,)
        return weighted_loss_sum(terms, weights)


@torch.no_grad()
def kd_teacher(teacher, im_data, im_info, gt_boxes, num_boxes, rois, T=3.0):
    """The teacher's side of the distillation (lib/PT_MAF/faster_rcnn_kd.py:43-108): a frozen
    tlod.detector.faster_rcnn.vgg16 in eval mode on the source image and the student's
    sampled RoIs.  Returns (RPN scores (1, 2, A*H, W), RoI class scores (R, n_classes),
    g (H, W) the ground-truth cell mask); the temperature is applied in kd_loss, T is kept
    for the reference's signature."""
    assert not teacher.training, "the teacher runs in eval mode (PT_MAF_train.py:407)"
    base = teacher.RCNN_base(im_data)
    _, score_r, _, _ = teacher.RCNN_rpn.head(base)
    feat = teacher._head_to_tail(teacher._pool(base, rois.detach().view(-1, 5)))
    cls_score = teacher.RCNN_cls_score(feat)
    g = gt_cell_mask(gt_boxes, num_boxes, base.shape[2], base.shape[3])
    return score_r, cls_score, g


def kd_loss(model, teacher_out, rois_label, T=3.0):
    """PT_MAF_train.py:449-451: sum_r pos_r sum_c p1 log(p1 / p2) / (sum pos + 1) over the
    RoI class scores (pos = rois_label > 0) plus sum g p1 log(p1 / p2) / (sum g + 1) over the
    two-way RPN scores, p1 / p2 the student's / teacher's softmax at temperature T."""
    s_rpn, s_cls = model.kd_scores
    t_rpn, t_cls, g = teacher_out
    pos = (rois_label.view(-1) > 0).float()
    return kd_kl_rows(s_cls, t_cls, pos, T) + kd_kl_rpn(s_rpn, t_rpn, g, T)


class vgg16(_fasterRCNN):
    """lib/PT_MAF/vgg16.py: as tlod.da.maf.vgg16 (the reference's PT-MAF teacher exists for
    VGG16 only, so there is no ResNet variant)."""

    FUSE_POOLS = maf.vgg16.FUSE_POOLS

    def __init__(self, classes, pretrained=False, class_agnostic=False):
        self.dout_base_model = 512
        self.instance_dim = 4096
        self.pretrained = pretrained
        self.class_agnostic = class_agnostic
        _fasterRCNN.__init__(self, classes, class_agnostic)

    def _init_modules(self):
        maf.vgg16._init_modules(self)

    def _head_to_tail(self, pool5):
        return self.RCNN_top(pool5.view(pool5.size(0), -1))
