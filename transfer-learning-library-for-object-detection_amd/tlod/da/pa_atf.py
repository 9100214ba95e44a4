"""PA-ATF (lib/PA_ATF/{faster_rcnn,vgg16,proposal_layer1}.py, methods/PA_ATF) on the tlod
kernels: ATF with gated image discriminators, an L1 instance discriminator over the sampled
RoIs, a subsampled target proposal layer and the CLUB prototype loss.  VGG16 only, one image
per domain.

``vgg16(classes).create_architecture()`` carries the reference's module names (a reference
checkpoint loads with strict=True); ``model(im_data, im_info, gt_boxes, num_boxes,
need_backprop, tgt_im_data, tgt_im_info, tgt_gt_boxes, tgt_num_boxes, tgt_need_backprop,
weight=0.1)`` returns the reference's 13-tuple (faster_rcnn.py:408-409: ATF's 12 plus pm_loss);
in eval mode the first four arguments alone give the s-branch detections
(methods/PA_ATF/PA_ATF_test.py evaluates the plain detector).  ``total_loss(out, lamda, beta)``
is PA_ATF_train.py:405-408: no 7x on the image terms, beta * pm_loss.

What differs from ATF, as read from the reference:
  * ``_ImageDA(dim)`` (:68-103): xx = GRL(x, weight); mask = sigmoid(adaptive_max_pool2d(
    Convm2(maxpool2x2(relu(Convm1(xx)))), 1)) with Convm1 dim->dim 5x5 stride 3 and Convm2 3x3
    stride 2 (``tlod.conv.StridedConv2d``, the gate is ``gate``); p = sigmoid(Conv2(relu(Conv1(
    xx * mask)))); BCELoss(p, label).  The reference hands BCELoss an (N, H, W) target for an
    (N, 1, H, W) input, which current torch refuses: stated here as the elementwise BCE over
    equal element counts, with BCELoss's log clamp at -100.
  * ``_InstanceDA`` (:43-66) ends in torch.abs(x (R, 1) - label (R)).mean(), which broadcasts to
    (R, R): mean_i mean_j |x_i - l_j| (with R = 256 and one image the label is constant and
    this is the plain mean).  The source term reads the fc7 rows of the t branch's 256 sampled
    RoIs, not the 2000 proposals.
  * the target RoIs come from the eval-mode RPN with post-NMS top-N = 256 (rois.size(1), :312;
    passed to the target's job, the global cfg is left alone) through proposal_layer1.py:152-160:
    the first 64 NMS survivors, then 192 of the others drawn without replacement
    (``tlod.rpn.proposal.proposal_subsample``).
  * pm_loss (:387-406): _RoIPooling(7, 7, 1/4 | 1/8 | 1/16) of the source gt boxes on the t
    branch's conv3 / conv4 / conv5 maps, times the level's detached source mask and its
    complement, into CLUB(dim) (:105-147) — ``proto_pool`` and ``CLUB``.
  * DA and CLUB modules keep PyTorch's default init (_init_weights touches the RPN and the two
    heads only).

Scheduling, the same math in fewer passes, as tlod.da.atf: the frozen conv1 / conv2 prefix runs
once for both images; the s branch runs source + target batched; the three RPN heads run as one
batch; the proposal layers run on side streams while the main stream computes the RPN losses;
one RoIAlign and one fc6 / fc7 pass serve the three 256-row RoI sets (s sampled, t sampled,
target); each gated head runs once over its (source, target) pair with N = 2 and a mask per
image; CLUB scores its ``same`` and ``diff`` inputs as one batch; the 14 scalar terms are one
launch each way (``losses``).

Deviations: the reference asserts need_backprop == 1 and tgt_need_backprop == 0 (a host
synchronisation per step); here the labels are those constants and the tensors are not read.
``gt_boxes.squeeze()[:num_boxes]`` needs the gt count on the host: one ``int(num_boxes)`` late
in the forward, after the detector's work is queued.  A source image without gt boxes gives
pm_loss 0 (the reference's mean over zero rows is NaN).

``replay_rng`` (tests): a numpy RandomState whose draws are consumed in this order — anchor
target s, anchor target t, proposal target s, proposal target t, the target's subsample as
``rng.permutation(len(rest))[:k]``, then ``rng.permutation(G)`` for club3, club4, club5.  The
reference draws the last two with Python's random.sample and torch.randperm, streams a
RandomState cannot replay: the distributions are the same, the streams are not.  Without it the
subsample uses libtlod's counter-based generator and the shuffles torch.randperm.  ``capture``
(tests) receives the proposal sets, the target's kept and picked RoIs, the gate arguments of
the three levels (source row, target row), the prototype pooling's argmax and the shuffles.

``TLOD_FUSED_PA_ATF=0`` takes the torch compositions of the gate, the prototype pooling and
the losses (``gate_torch``, ``proto_pool_torch``, ``losses_torch``) instead of the kernels of
include/tlod_pa_atf.h; ``TLOD_SCONV=0`` runs the strided convolutions on F.conv2d.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from ..config import cfg
from ..conv import Conv2d, StridedConv2d
from ..detector.losses import smooth_l1_loss, weighted_loss_sum
from ..roi_pool import _RoIPooling
from ..rpn.proposal import (proposal_keep, proposal_pick, proposal_subsample,
                            proposals_on_side_streams, subsample_head)
from . import atf as _atf
from .daf import _InstanceDA as _DAFInstanceDA
from .daf import early_rpn, early_rpn_backward, grad_reverse
from ..linear import relu_dropout


def fused_pa_atf():
    """TLOD_FUSED_PA_ATF (default 1): the libtlod gate / prototype-pooling kernels; 0 = the
    torch compositions."""
    return _lib.env("TLOD_FUSED_PA_ATF", "1") != "0"


# ------------------------------------------------------------------ torch compositions
def gate_torch(z):
    """(mask (N, C, 1, 1), arg (N, C) int32) as the reference composes them."""
    m, arg = F.adaptive_max_pool2d(z, 1, return_indices=True)
    return torch.sigmoid(m), arg.view(z.shape[0], z.shape[1]).to(torch.int32)


def proto_pool_torch(feat, gt_rois, scale, mask, perm, alpha=0.1, pooled=None):
    """(same, diff): CLUB's two (G, 2C, 7, 7) inputs, behind its gradient reversals.
    pooled: the (G, C, 7, 7) RoI pooling when the caller has it already (a test without a GPU
    pools on the CPU); default _RoIPooling(7, 7, scale)(feat, gt_rois)."""
    p = _RoIPooling(7, 7, scale)(feat, gt_rois) if pooled is None else pooled
    m = mask.detach().view(1, -1, 1, 1)
    a = grad_reverse(p * m, alpha)
    s = grad_reverse(p * (1 - m), alpha)
    return torch.cat((a, s), 1), torch.cat((a, s[perm.long()]), 1)


def losses_torch(img, img_labels, ins, ins_ones, club, club_labels):
    """The 14 unweighted terms as torch compositions of the reference's formulas: BCELoss of
    the sigmoid (elementwise over equal element counts: the reference's (N, H, W) target for an
    (N, 1, H, W) input is refused by current torch), torch.abs(x (R, 1) - label (R)).mean()
    with its (R, R) broadcast, and nll_loss(log_softmax)."""
    terms = []
    for z, lab in zip(img, img_labels):
        p = torch.sigmoid(z.reshape(-1))
        terms.append(F.binary_cross_entropy(p, torch.full_like(p, float(lab))))
    for z, ones in zip(ins, ins_ones):
        x = torch.sigmoid(z.reshape(-1, 1))
        label = torch.zeros(x.shape[0], dtype=x.dtype, device=x.device)
        label[:int(ones)] = 1
        terms.append(torch.abs(x - label).mean())
    for z, lab in zip(club, club_labels):
        target = torch.full((z.shape[0],), int(lab), dtype=torch.long, device=z.device)
        terms.append(F.nll_loss(F.log_softmax(z, 1), target))
    return torch.stack(terms)


def _int_array(values):
    import ctypes
    return (ctypes.c_int * len(values))(*[int(v) for v in values])


def _ptr_array(tensors):
    return (_lib.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class _Losses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, n, label, *z):
        _lib.require_cuda(*z)
        z = [t.detach().contiguous().float() for t in z]
        out = torch.empty(len(z), dtype=torch.float32, device=z[0].device)
        ctx.tables = (_int_array(n), _int_array(label))
        _lib.check(_lib.lib().tlod_pa_atf_loss_f32(_ptr_array(z), *ctx.tables, _lib.ptr(out),
                                                   _lib.stream_of(out)), "pa_atf_loss")
        ctx.save_for_backward(*z)
        return out

    @staticmethod
    def backward(ctx, g):
        z = ctx.saved_tensors
        g = g.contiguous().float()
        dz = [torch.empty_like(t) for t in z]
        _lib.check(_lib.lib().tlod_pa_atf_loss_bwd_f32(_ptr_array(z), *ctx.tables, _lib.ptr(g),
                                                       _ptr_array(dz), _lib.stream_of(g)),
                   "pa_atf_loss_bwd")
        return (None, None, *dz)


def losses(img, img_labels, ins, ins_ones, club, club_labels):
    """The 14 unweighted scalar terms of a step as one (14,) tensor, one launch each way:
    img: six logit maps (any shape) with their constant labels (0 / 1); ins: two (R, 1) logit
    columns with the number of ones among each one's R labels; club: six (G, 2) logit pairs with
    their labels (same: 1, diff: 0).  The weights are the caller's one dot product."""
    if not (len(img) == len(img_labels) == 6 and len(ins) == len(ins_ones) == 2
            and len(club) == len(club_labels) == 6):
        raise ValueError("losses: six image, two instance and six CLUB terms")
    if not fused_pa_atf():
        return losses_torch(img, img_labels, ins, ins_ones, club, club_labels)
    n = [t.numel() for t in img] + [t.numel() for t in ins] + [t.shape[0] for t in club]
    label = list(img_labels) + list(ins_ones) + list(club_labels)
    return _Losses.apply(n, label, *img, *ins, *club)


# ------------------------------------------------------------------ channel gate
class _Gate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z):
        _lib.require_cuda(z)
        z = z.contiguous()
        N, C, h, w = z.shape
        mask = torch.empty((N, C, 1, 1), dtype=torch.float32, device=z.device)
        arg = torch.empty((N, C), dtype=torch.int32, device=z.device)
        _lib.check(_lib.lib().tlod_pa_gate_f32(_lib.ptr(z), N, C, h, w, _lib.ptr(mask),
                                               _lib.ptr(arg), _lib.stream_of(z)), "pa_gate")
        ctx.shape = (N, C, h, w)
        ctx.save_for_backward(mask, arg)
        ctx.mark_non_differentiable(arg)
        return mask, arg

    @staticmethod
    def backward(ctx, dmask, _darg=None):
        mask, arg = ctx.saved_tensors
        N, C, h, w = ctx.shape
        dmask = dmask.contiguous()
        dz = torch.empty(ctx.shape, dtype=torch.float32, device=dmask.device)
        _lib.check(_lib.lib().tlod_pa_gate_bwd_f32(_lib.ptr(dmask), _lib.ptr(mask), _lib.ptr(arg),
                                                   N, C, h, w, _lib.ptr(dz),
                                                   _lib.stream_of(dmask)), "pa_gate_bwd")
        return dz


def gate(z):
    """(mask (N, C, 1, 1), arg (N, C) int32) of the mask net's output z (N, C, h, w)."""
    if not fused_pa_atf():
        return gate_torch(z)
    return _Gate.apply(z)


# ------------------------------------------------------------------ prototype pooling
class _ProtoPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, gt_rois, scale, mask, perm, alpha):
        _lib.require_cuda(feat, gt_rois, mask, perm)
        if feat.shape[0] != 1:
            raise ValueError("proto_pool: one image per call (PA-ATF runs batch 1 per domain)")
        feat = feat.contiguous()
        rois = gt_rois.detach().contiguous().float()
        mask = mask.detach().contiguous().view(-1)
        perm = perm.contiguous().to(torch.int32)
        _, C, H, W = feat.shape
        G = rois.shape[0]
        if mask.numel() != C or perm.numel() != G or rois.shape[1] != 5:
            raise ValueError("proto_pool: mask (C), perm (G) and gt_rois (G, 5)")
        same = torch.empty((G, 2 * C, 7, 7), dtype=torch.float32, device=feat.device)
        diff = torch.empty_like(same)
        argmax = torch.empty((G, C, 7, 7), dtype=torch.int32, device=feat.device)
        _lib.check(_lib.lib().tlod_pa_proto_pool_fwd_f32(
            _lib.ptr(feat), C, H, W, _lib.ptr(rois), G, float(scale), _lib.ptr(mask),
            _lib.ptr(perm), _lib.ptr(same), _lib.ptr(diff), _lib.ptr(argmax),
            _lib.stream_of(feat)), "pa_proto_pool_fwd")
        ctx.meta = (C, H, W, G, float(scale), float(alpha))
        ctx.save_for_backward(rois, mask, perm, argmax)
        ctx.mark_non_differentiable(argmax)
        return same, diff, argmax

    @staticmethod
    def backward(ctx, d_same, d_diff, _dargmax=None):
        rois, mask, perm, argmax = ctx.saved_tensors
        C, H, W, G, scale, alpha = ctx.meta
        d_same, d_diff = d_same.contiguous(), d_diff.contiguous()
        dfeat = torch.empty((1, C, H, W), dtype=torch.float32, device=d_same.device)
        _lib.check(_lib.lib().tlod_pa_proto_pool_bwd_f32(
            _lib.ptr(d_same), _lib.ptr(d_diff), _lib.ptr(mask), _lib.ptr(perm), _lib.ptr(argmax),
            _lib.ptr(rois), G, scale, C, H, W, alpha, _lib.ptr(dfeat),
            _lib.stream_of(d_same)), "pa_proto_pool_bwd")
        return dfeat, None, None, None, None, None


def proto_pool(feat, gt_rois, scale, mask, perm, alpha=0.1):
    """CLUB's inputs for one level: feat (1, C, H, W), gt_rois (G, 5), the level's channel
    mask (C values, detached here as in the reference) and CLUB's shuffle perm (G) ->
    (same, diff), each (G, 2C, 7, 7); the gradient to feat is reversed with alpha."""
    if not fused_pa_atf():
        return proto_pool_torch(feat, gt_rois, scale, mask, perm, alpha)
    same, diff, _ = _ProtoPool.apply(feat, gt_rois, scale, mask, perm, alpha)
    return same, diff


# ------------------------------------------------------------------ modules
class _ImageDA(nn.Module):
    """lib/PA_ATF/faster_rcnn.py:68-103; returns the domain logit map (N, 1, H, W), the channel
    mask (N, C, 1, 1) and the mask's argument (N, C) — the loss is taken by ``losses``."""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim
        self.Conv1 = Conv2d(dim, dim // 2, 1, bias=False, relu=True)
        self.Conv2 = Conv2d(dim // 2, 1, 1, bias=False)       # the small-1x1 kernels
        self.Convm1 = StridedConv2d(dim, dim, 5, stride=3, relu=True)
        self.Convm2 = StridedConv2d(dim, dim, 3, stride=2)

    def forward(self, x, alpha=0.1, arg=None):
        """arg (tests): gate arguments (N, C) to take the planes' values at instead of their
        own maxima — a second run of the same step follows the first run's routing."""
        xx = grad_reverse(x, alpha)
        z = self.Convm2(F.max_pool2d(self.Convm1(xx), 2, 2))
        if arg is None:
            mask, arg = gate(z)
        else:
            N, C = z.shape[:2]
            mask = torch.sigmoid(z.reshape(N, C, -1).gather(2, arg.long().view(N, C, 1))
                                 ).view(N, C, 1, 1)
        return self.Conv2(self.Conv1(xx * mask)), mask, arg


class _InstanceDA(_DAFInstanceDA):
    """lib/PA_ATF/faster_rcnn.py:43-66: DAF's layers; the logits (R, 1) are returned, the
    sigmoid and the (R, R)-broadcast L1 are taken by ``losses``."""

    def logit(self, x, alpha=0.1):
        x = grad_reverse(x, alpha)
        x = relu_dropout(self.dc_ip1(x), self.dc_drop1, getattr(self.dc_ip1, "act_tap", None))
        x = relu_dropout(self.dc_ip2(x), self.dc_drop2, getattr(self.dc_ip2, "act_tap", None))
        return self.clssifer(x)


class CLUB(nn.Module):
    """lib/PA_ATF/faster_rcnn.py:105-147 behind ``proto_pool`` (which applies the two gradient
    reversals and the shuffle): out_score = conv 2 dim -> dim 3x3 stride 2, ReLU, conv dim -> 128
    1x1, ReLU (the ReLUs are fused into the convs; indices 1 and 3 stay as placeholders so the
    keys are out_score.0 / out_score.2), fc = Linear(3 * 3 * 128, 2).  ``same`` and ``diff`` are
    scored as one batch of 2 G rows."""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim
        self.out_score = nn.Sequential(StridedConv2d(2 * dim, dim, 3, stride=2, relu=True),
                                       nn.Identity(),
                                       Conv2d(dim, 128, 1, relu=True),
                                       nn.Identity())
        self.fc = nn.Linear(3 * 3 * 128, 2)

    def forward(self, same, diff):
        G = same.shape[0]
        x = self.out_score[0](torch.cat((same, diff), 0)).contiguous()
        x = self.out_score[2](x)
        z = self.fc(x.reshape(2 * G, -1))
        return z[:G], z[G:]

    def forward_torch(self, same, diff):
        """The same scores as the reference composes them, one input at a time on plain
        F.conv2d / F.linear over this module's parameters (the statement the tests compare
        with; it also runs without a GPU)."""
        c0, c2 = self.out_score[0], self.out_score[2]

        def score(x):
            x = F.relu(F.conv2d(x, c0.weight, c0.bias, stride=2))
            x = F.relu(F.conv2d(x, c2.weight, c2.bias))
            return F.linear(x.reshape(x.size(0), -1), self.fc.weight, self.fc.bias)
        return score(same), score(diff)


# 14 unweighted terms -> DA_img, tgt_DA_img, DA_ins, tgt_DA_ins, pm_loss (term order of forward)
_GROUPS = ((0, 1, 2), (3, 4, 5), (6,), (7,), (8, 9, 10, 11, 12, 13))
_GROUP_M = {}


def _group_matrix(device):
    m = _GROUP_M.get(str(device))
    if m is None:
        m = torch.zeros(len(_GROUPS), 14)
        for i, g in enumerate(_GROUPS):
            m[i, list(g)] = 1.0
        m = _GROUP_M[str(device)] = m.to(device)
    return m


class _fasterRCNN(_atf._fasterRCNN):
    """lib/PA_ATF/faster_rcnn.py:149-409."""

    def __init__(self, classes, class_agnostic):
        super().__init__(classes, class_agnostic)
        del self.RCNN_rpn_t  # ATF's unused second RPN: PA-ATF's reference does not build it
        self.RCNN_imageDA_3 = _ImageDA(256)
        self.RCNN_imageDA_4 = _ImageDA(512)
        self.RCNN_imageDA = _ImageDA(self.dout_base_model)
        self.RCNN_instanceDA = _InstanceDA(self.instance_dim)
        self.club3 = CLUB(256)
        self.club4 = CLUB(512)
        self.club5 = CLUB(self.dout_base_model)
        self.align1 = _RoIPooling(7, 7, 1.0 / 4.0)   # parameter-free; proto_pool does their work
        self.align2 = _RoIPooling(7, 7, 1.0 / 8.0)
        self.align3 = _RoIPooling(7, 7, 1.0 / 16.0)
        self.force_args = None  # tests: three (N, C) gate-argument tensors (see _ImageDA)

    # ---------------------------------------------------------------- eval (4 arguments)
    def _detect(self, im_data, im_info):
        batch_size = im_data.size(0)
        base = self.RCNN_base(im_data)
        _, _, prob, bbox = self.RCNN_rpn.head(base)
        rois = self.RCNN_rpn.RPN_proposal((prob.detach(), bbox.detach(), im_info.detach(),
                                           "TEST"))
        feat = self._head_to_tail(self._pool(base, rois.view(-1, 5)))
        cls_prob = F.softmax(self.RCNN_cls_score(feat), 1).view(batch_size, rois.size(1), -1)
        bbox_pred = self.RCNN_bbox_pred(feat).view(batch_size, rois.size(1), -1)
        return rois, cls_prob, bbox_pred, 0, 0, 0, 0, None

    # ---------------------------------------------------------------- target proposals
    def _proposal_job(self, inp):
        """The side streams' layer: TRAIN proposals, the target's survivors (two-phase: replayed
        draws and captures pick later, on the main stream) or the chained subsample."""
        prob, deltas, info, key = inp
        layer = self.RCNN_rpn.RPN_proposal
        if key == "TRAIN":
            return layer(inp)
        c = cfg.TEST
        if key == "KEEP":
            kept, counts = proposal_keep(prob, deltas, info, layer._anchors, layer._feat_stride,
                                         c.RPN_PRE_NMS_TOP_N, c.RPN_NMS_THRESH)
            return torch.cat((kept.view(-1), counts.float()))  # one tensor for join()
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # the CPU generator: no device sync
        return proposal_subsample(prob, deltas, info, layer._anchors, layer._feat_stride,
                                  c.RPN_PRE_NMS_TOP_N, int(cfg.TRAIN.BATCH_SIZE),
                                  c.RPN_NMS_THRESH, seed)

    def _pick(self, packed, post):
        """Phase 2 of the target's proposals on the main stream (replay / capture)."""
        kept = packed[:-1].view(1, -1, 4)
        counts = packed[-1:].to(torch.int32)
        if self.replay_rng is not None:
            n_rest = max(int(counts[0]) - subsample_head(post), 0)
            k = min(n_rest, post - subsample_head(post))
            pick = [self.replay_rng.permutation(n_rest)[:k] if n_rest else []]
            rois = proposal_pick(kept, counts, post, pick=pick)
        else:
            rois = proposal_pick(kept, counts, post,
                                 seed=int(torch.randint(0, 2 ** 62, (1,)).item()))
        if self.capture is not None:
            self.capture.update(t_kept=kept.detach().clone(), t_count=counts.clone())
        return rois

    # ---------------------------------------------------------------- forward
    def forward(self, im_data, im_info, gt_boxes, num_boxes, need_backprop=None,
                tgt_im_data=None, tgt_im_info=None, tgt_gt_boxes=None, tgt_num_boxes=None,
                tgt_need_backprop=None, weight=0.1):
        if not self.training:
            return self._detect(im_data, im_info)
        if tgt_im_data is None:
            raise RuntimeError("PA-ATF trains through the 10-argument forward; the 4-argument "
                               "form is the eval-mode detector")
        batch_size = im_data.size(0)
        if batch_size != 1 or tgt_im_data.size(0) != 1:
            raise ValueError("PA-ATF runs one image per domain (gt_boxes.squeeze()[:num_boxes])")
        im_info = im_info.detach()
        gt_boxes = gt_boxes.detach()
        same = im_data.shape == tgt_im_data.shape
        rpn = self.RCNN_rpn
        early = early_rpn(self, same)

        # ---- backbones: the frozen conv1 / conv2 prefix is shared by both branches
        if same:
            z = self._shared(torch.cat([im_data, tgt_im_data], 0))
            c3s, c4s, bs = self._branch(self.RCNN_base, z)
            c3_t, c4_t, base_t = self._branch(self.RCNN_base_t, z[:1])
            base_feat, tgt_base_feat = bs[:1], bs[1:]
            tgt_c3, tgt_c4 = c3s[1:], c4s[1:]
            rpn_in = torch.cat([base_feat, base_t, tgt_base_feat], 0)
            if early:
                rpn_in = rpn_in.detach().requires_grad_(True)
            heads = rpn.head(rpn_in)
            hs = [tuple(h[i:i + 1] for h in heads) for i in range(3)]
        else:
            z = self._shared(im_data)
            _, _, base_feat = self._branch(self.RCNN_base, z)
            c3_t, c4_t, base_t = self._branch(self.RCNN_base_t, z)
            tgt_c3, tgt_c4, tgt_base_feat = self._branch(self.RCNN_base,
                                                         self._shared(tgt_im_data))
            hs = [rpn.head(f) for f in (base_feat, base_t, tgt_base_feat)]

        # ---- RPN: train mode on the source through both branches; the target's eval-mode
        # proposals with post-NMS top-N := the RCNN batch (rois.size(1), :312).  The reference
        # writes that count into the global cfg.TEST.RPN_POST_NMS_TOP_N and leaves it there; it
        # evaluates in another process, so its detector still proposes 300 RoIs.  Here the
        # count is passed to the target's job and the global stays what it was, so an
        # evaluation in the training process sees the configured 300 as well.
        post = int(cfg.TRAIN.BATCH_SIZE)
        two_phase = self.replay_rng is not None or self.capture is not None
        pending = proposals_on_side_streams(self._proposal_job, [
            (hs[0][2].detach(), hs[0][3].detach(), im_info, "TRAIN"),
            (hs[1][2].detach(), hs[1][3].detach(), im_info, "TRAIN"),
            (hs[2][2].detach(), hs[2][3].detach(), tgt_im_info.detach(),
             "KEEP" if two_phase else "SUBSAMPLE")])
        l_cls1, l_box1, _ = rpn.losses(hs[0][0], hs[0][1], hs[0][3], gt_boxes, im_info, num_boxes,
                                       rng=self.replay_rng)
        l_cls2, l_box2, _ = rpn.losses(hs[1][0], hs[1][1], hs[1][3], gt_boxes, im_info, num_boxes,
                                       rng=self.replay_rng)
        rpn_loss_cls = l_cls1 + l_cls2
        rpn_loss_bbox = l_box1 + l_box2
        if early:  # rpn_in rows: source (RCNN_base), source (RCNN_base_t), target (RCNN_base)
            rpn_loss_cls, rpn_loss_bbox = early_rpn_backward(
                rpn_loss_cls, rpn_loss_bbox, rpn_in,
                [(bs, lambda g: torch.cat([g[0:1], g[2:3]], 0)), (base_t, lambda g: g[1:2])])
        rois_domain, rois_domain_t, tgt_rois = pending.join()

        rois, rois_label, rois_target, rois_inside_ws, rois_outside_ws = \
            self._sampled(rois_domain, gt_boxes, num_boxes)
        rois_t, rois_label_t, rois_target_t, rois_inside_ws_t, rois_outside_ws_t = \
            self._sampled(rois_domain_t, gt_boxes, num_boxes)
        if two_phase:
            tgt_rois = self._pick(tgt_rois, post)
        if self.capture is not None:
            self.capture.update(s_rois=rois_domain.detach().clone(),
                                st_rois=rois_domain_t.detach().clone(),
                                t_rois=tgt_rois.detach().clone())

        # ---- one RoIAlign + fc6 / fc7 pass over the three 256-row RoI sets
        sets = (rois, rois_t, tgt_rois)
        n = [r.size(1) for r in sets]
        if same:
            feats = torch.cat([base_feat, tgt_base_feat, base_t], 0)
            rr = []
            for r, i in zip(sets, (0, 2, 1)):
                r = r.view(-1, 5).clone()
                r[:, 0] = float(i)
                rr.append(r)
            fc7 = self._head_to_tail(self._pool(feats, torch.cat(rr, 0)))
        else:
            fc7 = torch.cat([self._head_to_tail(self._pool(f, r.view(-1, 5)))
                             for f, r in zip((base_feat, base_t, tgt_base_feat), sets)], 0)
        n_det = n[0] + n[1]
        det = fc7[:n_det]  # s-branch and t-branch sampled RoIs

        bbox_all = self.RCNN_bbox_pred(det)
        labels = torch.cat([rois_label, rois_label_t])
        if not self.class_agnostic:
            view = bbox_all.view(bbox_all.size(0), int(bbox_all.size(1) / 4), 4)
            bbox_all = torch.gather(view, 1, labels.view(-1, 1, 1).expand(-1, 1, 4)).squeeze(1)
        cls_all = self.RCNN_cls_score(det)
        RCNN_loss_cls = (F.cross_entropy(cls_all[:n[0]], rois_label)
                         + F.cross_entropy(cls_all[n[0]:], rois_label_t))
        RCNN_loss_bbox = (smooth_l1_loss(bbox_all[:n[0]], rois_target, rois_inside_ws,
                                         rois_outside_ws)
                          + smooth_l1_loss(bbox_all[n[0]:], rois_target_t, rois_inside_ws_t,
                                           rois_outside_ws_t))
        cls_prob = F.softmax(cls_all[:n[0]], 1).view(batch_size, rois_t.size(1), -1)
        bbox_pred = bbox_all[:n[0]].view(batch_size, rois_t.size(1), -1)

        # ---- gated image heads: source through the t branch, target through the s branch
        da_heads = (self.RCNN_imageDA_3, self.RCNN_imageDA_4, self.RCNN_imageDA)
        pairs = ((c3_t, tgt_c3), (c4_t, tgt_c4), (base_t, tgt_base_feat))
        s_logit, t_logit, cw, args = [], [], [], []
        forced = self.force_args or (None, None, None)
        for h, (fs, ft), fa in zip(da_heads, pairs, forced):
            if same:
                logit, mask, arg = h(torch.cat((fs, ft), 0), weight, fa)
                s_logit.append(logit[:1])
                t_logit.append(logit[1:])
            else:
                ls, mask, arg = h(fs, weight, None if fa is None else fa[:1])
                lt, _, arg_t = h(ft, weight, None if fa is None else fa[1:])
                s_logit.append(ls)
                t_logit.append(lt)
                arg = torch.cat((arg, arg_t), 0)
            cw.append(mask[0].detach().reshape(-1))
            args.append(arg)  # (2, C): the source's row, then the target's

        # ---- instance head: the t branch's sampled RoIs and the target's RoIs (fc7 rows)
        ins = self.RCNN_instanceDA.logit(fc7[n[0]:])
        ins_s, ins_t = ins[:n[1]], ins[n[1]:]

        # ---- prototype loss over the source gt boxes (one host read: the gt count)
        G = int(num_boxes.view(-1)[0])
        club = []
        if G > 0:
            gt_rois = torch.cat((gt_boxes.new_zeros(G, 1), gt_boxes[0, :G, :4]), 1)
            perms = []
            for feat, scale, mask, mod in zip((c3_t, c4_t, base_t), (1 / 4, 1 / 8, 1 / 16), cw,
                                              (self.club3, self.club4, self.club5)):
                if self.replay_rng is not None:
                    perm = torch.from_numpy(np.asarray(self.replay_rng.permutation(G)))
                else:
                    perm = torch.randperm(G)
                perm = perm.to(torch.int32).to(feat.device, non_blocking=True)
                perms.append(perm)
                if self.capture is not None and fused_pa_atf():
                    sd, df, am = _ProtoPool.apply(feat, gt_rois, scale, mask, perm, 0.1)
                    self.capture.setdefault("pp_argmax", []).append(am.clone())
                    club.extend(mod(sd, df))
                else:
                    club.extend(mod(*proto_pool(feat, gt_rois, scale, mask, perm, 0.1)))
            if self.capture is not None:
                self.capture.update(perms=[p.clone() for p in perms])
        else:  # no box, no prototype: six zero terms without a gradient
            club = [gt_boxes.new_zeros(1, 2) for _ in range(6)]
        if self.capture is not None:
            self.capture.update(args=[a.clone() for a in args])

        terms = losses(s_logit + t_logit, (1, 1, 1, 0, 0, 0), (ins_s, ins_t), (n[1], 0), club,
                       (1, 0, 1, 0, 1, 0))
        if G == 0:
            terms = terms * terms.new_tensor([1.0] * 8 + [0.0] * 6)
        DA_img, tgt_DA_img, DA_ins, tgt_DA_ins, pm_loss = torch.mv(
            _group_matrix(terms.device), terms).unbind(0)
        return (rois_t, cls_prob, bbox_pred, rpn_loss_cls, rpn_loss_bbox, RCNN_loss_cls,
                RCNN_loss_bbox, rois_label_t, DA_img, tgt_DA_img, DA_ins, tgt_DA_ins, pm_loss)

    @staticmethod
    def total_loss(out, lamda=0.1, beta=0.1):
        """methods/PA_ATF/PA_ATF_train.py:405-408: det + lamda (DA_img + DA_ins + tgt_DA_img +
        tgt_DA_ins) + beta pm_loss."""
        (_, _, _, rpn_loss_cls, rpn_loss_box, RCNN_loss_cls, RCNN_loss_bbox, _, DA_img,
         tgt_DA_img, DA_ins, tgt_DA_ins, pm_loss) = out
        return weighted_loss_sum(
            (rpn_loss_cls, rpn_loss_box, RCNN_loss_cls, RCNN_loss_bbox, DA_img, DA_ins, tgt_DA_img,
             tgt_DA_ins, pm_loss), (1, 1, 1, 1, lamda, lamda, lamda, lamda, beta))


class vgg16(_fasterRCNN):
    """lib/PA_ATF/vgg16.py:20-79."""

    FUSE_POOLS = _atf.vgg16.FUSE_POOLS
    splits = _atf.vgg16.splits

    def __init__(self, classes, pretrained=False, class_agnostic=False):
        self.dout_base_model = 512
        self.instance_dim = 4096
        self.pretrained = pretrained
        self.class_agnostic = class_agnostic
        _fasterRCNN.__init__(self, classes, class_agnostic)

    def _init_modules(self):
        _atf.vgg16._init_modules(self)
        # the conv3 / conv34 / conv45 views as the reference builds them (vgg16.py:52-59):
        # fresh Sequentials, so their keys count from 0 (conv34_s.1.weight is conv4_1) and a
        # reference checkpoint's view keys name the same tensors here
        _, e3, e4 = self.splits
        for tag, base in (("s", self.RCNN_base), ("t", self.RCNN_base_t)):
            layers = list(base)
            setattr(self, "conv3_" + tag, nn.Sequential(*layers[:e3]))
            setattr(self, "conv34_" + tag, nn.Sequential(*layers[e3:e4]))
            setattr(self, "conv45_" + tag, nn.Sequential(*layers[e4:]))

    _head_to_tail = _atf.vgg16._head_to_tail
