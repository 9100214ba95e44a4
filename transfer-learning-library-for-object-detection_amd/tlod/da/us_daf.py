"""US-DAF (DAF with a one-channel image head and a scale-aware multi-label instance head) on
the tlod kernels — lib/US_DAF/{DA,faster_rcnn,vgg16,resnet}.py and the loss sum of
methods/US_DAF/US_DAF_train.py:428-438.

``resnet(classes).create_architecture()`` (or ``vgg16``) then ``model(im_data, im_info,
gt_boxes, num_boxes, tgt_im_data, tgt_im_info, tgt_gt_boxes, tgt_num_boxes)`` returns the
reference's 12-tuple (faster_rcnn.py:285-286).  The project's 10-tuple batch (with the two
need_backprop entries, which US-DAF fixes at 1 / 0, faster_rcnn.py:64-68) is accepted too, so
train_step, smoke_step and the gradient reducer drive it like every other method.

Beyond the detector, per image (source label 1, target label 0):
  * the image head's sigmoid map against the constant domain label under nn.BCELoss;
  * the instance head's four sigmoid outputs [domain, small, middle, large] against
    [domain label, scale labels of the RoI] under BCEloss_margin (faster_rcnn.py:25-33): the
    domain column of a row counts only where its own element loss exceeds 0.5.
The reference's four Python loops over the RoIs (about 1,100 device scalar reads per step) are
gone: the scale labels, both sigmoids, the gates and the four losses are one forward and one
backward launch (tlod_us_daf_loss_f32 / _bwd_f32); nothing in the forward synchronises with
the host.

Deviations from the reference, documented:
  * _InstanceDA is Linear(2048, ...) there (DA.py:72), so its VGG16 variant crashes on the
    4096-d head features; here the head takes ``instance_dim`` (the policy of tlod.da.daf's
    ResNet101 fix);
  * _init_weights touches RCNN_cls_score_img (faster_rcnn.py:306), which the reference's
    vgg16.py never defines; here both backbones define it;
  * label_img / image_softmax (faster_rcnn.py:152-177, 243-262) are computed and never used
    there: not built.  RCNN_imageDA_class and RCNN_cls_score_img are constructed and never
    called there: kept as frozen parameter-only modules, so reference checkpoints load with
    strict=True and, as in the reference (no gradient ever reaches them, so torch's SGD skips
    them), training never changes them.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from ..conv import Conv2d
from ..detector.losses import _grad_pair, fused_losses, weighted_loss_sum
from ..linear import Linear, relu_dropout
from ..rpn.proposal import proposals_on_side_streams
from . import daf
from .daf import early_rpn, early_rpn_backward, grad_reverse

NEAR_0 = 1e-10


# ------------------------------------------------------------------------------ device ops
def roi_scale_labels(rois):
    """rois (..., 5) -> (R, 3) 0 / 1 floats [small, middle, large] by faster_rcnn.py:108-119:
    area = (x2 - x1) * (y2 - y1) in fp32, <= 400 / between / >= 10000."""
    r = rois.detach().reshape(-1, 5)
    if not fused_losses():
        area = (r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2])
        return torch.stack([area <= 400, (area > 400) & (area < 10000), area >= 10000], 1).float()
    _lib.require_cuda(r)
    r = r.contiguous().float()
    lab = torch.empty((r.shape[0], 3), dtype=torch.float32, device=r.device)
    _lib.check(_lib.lib().tlod_roi_scale_labels_f32(_lib.ptr(r), r.shape[0], _lib.ptr(lab),
                                                    _lib.stream_of(r)), "roi_scale_labels")
    return lab


def bce_margin(s, label, gate=None):
    """BCEloss_margin (faster_rcnn.py:25-33) in torch; gate (n): the column-0 weights to use
    instead of the loss's own.  Returns (loss, gate)."""
    e = -(label * torch.log(s + NEAR_0) + (1 - label) * torch.log(1 - s + NEAR_0))
    a = (e[:, 0] > 0.5).float() if gate is None else gate.detach().to(e).view(-1)
    w = torch.cat([a.view(-1, 1), torch.ones((e.shape[0], 3), dtype=e.dtype, device=e.device)], 1)
    return (e * w).mean(), a


def _off(t, elems):
    return _lib.c_void_p(t.data_ptr() + 4 * elems)


class _USDAFLoss(torch.autograd.Function):
    """tlod_us_daf_loss_f32 / _bwd_f32 over one image-logit buffer and one instance-logit
    buffer holding the source part first: z_img (Bs + Bt images when the maps have one shape,
    else two tensors), z_ins (n_s + n_t, 4), rois (n_s + n_t, 5).  Each buffer gets one gradient
    tensor, so no slice enters the autograd graph.  Returns the four losses, then s_img, s_ins
    and the gates as non-differentiable outputs."""

    @staticmethod
    def forward(ctx, z_img_s, z_img_t, z_ins, rois, gate_in, Bs, n_s):
        packed = z_img_t is None
        _lib.require_cuda(z_img_s, z_img_t, z_ins, rois, gate_in)
        zi = z_img_s.detach().contiguous().float()
        zt = zi if packed else z_img_t.detach().contiguous().float()
        zn = z_ins.detach().contiguous().float()
        r = rois.detach().reshape(-1, 5).contiguous().float()
        n_t = zn.shape[0] - n_s
        assert zi.dim() == 4 and zi.shape[1] == 1 and zt.shape[1] == 1, (zi.shape, zt.shape)
        assert zn.dim() == 2 and zn.shape[1] == 4 and r.shape[0] == zn.shape[0] and n_t >= 0
        if packed:
            Bt = zi.shape[0] - Bs
            Hs, Ws = Ht, Wt = zi.shape[2:]
            t_off = Bs * Hs * Ws
        else:
            assert Bs == zi.shape[0]
            Bt, (Hs, Ws), (Ht, Wt), t_off = zt.shape[0], zi.shape[2:], zt.shape[2:], 0
        assert Bs > 0 and Bt > 0
        s_i, s_t = torch.empty_like(zi), (None if packed else torch.empty_like(zt))
        s_n = torch.empty_like(zn)
        gate = torch.empty(zn.shape[0], dtype=torch.float32, device=zn.device)
        loss = torch.empty(4, dtype=torch.float32, device=zn.device)
        g_in = None
        if gate_in is not None:
            g_in = gate_in.detach().contiguous().float().view(-1)
            assert g_in.numel() == zn.shape[0]
        _lib.check(_lib.lib().tlod_us_daf_loss_f32(
            _lib.ptr(zi), _off(zt, t_off), _lib.ptr(zn), _off(zn, 4 * n_s), _lib.ptr(r),
            _off(r, 5 * n_s), _lib.ptr(g_in), None if g_in is None else _off(g_in, n_s),
            Bs, Bt, Hs, Ws, Ht, Wt, n_s, n_t, _lib.ptr(s_i),
            _off(s_i if packed else s_t, t_off), _lib.ptr(s_n), _off(s_n, 4 * n_s),
            _lib.ptr(gate), _off(gate, n_s), _lib.ptr(loss), _lib.stream_of(zn)), "us_daf_loss")
        ctx.dims = (packed, Bs, Bt, Hs, Ws, Ht, Wt, n_s, n_t, t_off)
        ctx.shapes = (z_img_s.shape, None if packed else z_img_t.shape, z_ins.shape)
        saved = [s_i, s_n, r, gate] + ([] if packed else [s_t])
        ctx.save_for_backward(*saved)
        aux = (s_i, s_n, gate) if packed else (s_i, s_n, gate, s_t)
        ctx.mark_non_differentiable(*aux)
        ctx.set_materialize_grads(False)
        return (loss[0], loss[1], loss[2], loss[3]) + aux

    @staticmethod
    def backward(ctx, g0, g1, g2, g3, *_):
        packed, Bs, Bt, Hs, Ws, Ht, Wt, n_s, n_t, t_off = ctx.dims
        s_i, s_n, r, gate, *rest = ctx.saved_tensors
        s_t = s_i if packed else rest[0]
        if g0 is None and g1 is None and g2 is None and g3 is None:
            return (None,) * 7
        g = _grad_pair(g0, g1, g2, g3)
        d_i, d_n = torch.empty_like(s_i), torch.empty_like(s_n)
        d_t = d_i if packed else torch.empty_like(s_t)
        _lib.check(_lib.lib().tlod_us_daf_loss_bwd_f32(
            _lib.ptr(s_i), _off(s_t, t_off), _lib.ptr(s_n), _off(s_n, 4 * n_s), _lib.ptr(r),
            _off(r, 5 * n_s), _lib.ptr(gate), _off(gate, n_s), Bs, Bt, Hs, Ws, Ht, Wt, n_s, n_t,
            _lib.ptr(g), _lib.ptr(d_i), _off(d_t, t_off), _lib.ptr(d_n), _off(d_n, 4 * n_s),
            _lib.stream_of(s_n)), "us_daf_loss_bwd")
        sh = ctx.shapes
        return (d_i.view(sh[0]), None if packed else d_t.view(sh[1]), d_n.view(sh[2]), None,
                None, None, None)


def _cat_gate(gate_override):
    if gate_override is None:
        return None
    return torch.cat([g.detach().float().view(-1) for g in gate_override])


def _torch_losses(z_img_s, z_img_t, z_ins_s, z_ins_t, rois_s, rois_t, gate_override):
    """The same formulas as a torch composition (TLOD_FUSED_LOSSES=0)."""
    out, s_img, s_ins, gates = [], [], [], []
    for k, (zi, zn, r, y) in enumerate(((z_img_s, z_ins_s, rois_s, 1.0),
                                        (z_img_t, z_ins_t, rois_t, 0.0))):
        p = torch.sigmoid(zi)
        out.append(F.binary_cross_entropy(p.view(-1, 1), torch.full_like(p, y).view(-1, 1)))
        s = torch.sigmoid(zn)
        lab = torch.cat([torch.full((s.shape[0], 1), y, dtype=s.dtype, device=s.device),
                         roi_scale_labels(r).to(s)], 1)
        loss, gate = bce_margin(s, lab, None if gate_override is None else gate_override[k])
        out.append(loss)
        s_img.append(p.detach())
        s_ins.append(s.detach())
        gates.append(gate)
    return tuple(out), (s_img[0], s_img[1], s_ins[0], s_ins[1]), tuple(gates)


def us_daf_da_losses(z_img_s, z_img_t, z_ins_s, z_ins_t, rois_s, rois_t, gate_override=None):
    """Image logits (B, 1, H, W) and instance logits (n, 4) of the two domains, their RoIs
    (n, 5) -> ((DA_img, DA_ins, tgt_DA_img, tgt_DA_ins), (s_img_s, s_img_t, s_ins_s, s_ins_t),
    (gate_s, gate_t)); s and the gates carry no gradient.  gate_override = (gate_s, gate_t):
    the column-0 weights to use instead of the losses' own (tests)."""
    if not fused_losses():
        return _torch_losses(z_img_s, z_img_t, z_ins_s, z_ins_t, rois_s, rois_t, gate_override)
    n_s = z_ins_s.shape[0]
    # the instance rows and RoIs of the two domains as one buffer each (a per-row layout; the
    # two image maps may differ in shape and stay separate)
    z_ins = torch.cat([z_ins_s, z_ins_t], 0)
    rois = torch.cat([rois_s.detach().reshape(-1, 5), rois_t.detach().reshape(-1, 5)], 0)
    l0, l1, l2, l3, s_i, s_n, gate, s_t = _USDAFLoss.apply(
        z_img_s, z_img_t, z_ins, rois, _cat_gate(gate_override), z_img_s.shape[0], n_s)
    return (l0, l1, l2, l3), (s_i, s_t, s_n[:n_s], s_n[n_s:]), (gate[:n_s], gate[n_s:])


def us_daf_da_losses_packed(z_img2, z_ins2, rois2, Bs, n_s, gate_override=None):
    """us_daf_da_losses for the layout of the batched source + target pass: z_img2
    (Bs + Bt, 1, H, W), z_ins2 (n_s + n_t, 4) and rois2 (n_s + n_t, 5), source part first."""
    if not fused_losses():
        return _torch_losses(z_img2[:Bs], z_img2[Bs:], z_ins2[:n_s], z_ins2[n_s:], rois2[:n_s],
                             rois2[n_s:], gate_override)
    l0, l1, l2, l3, s_i, s_n, gate = _USDAFLoss.apply(
        z_img2, None, z_ins2, rois2, _cat_gate(gate_override), int(Bs), int(n_s))
    return ((l0, l1, l2, l3), (s_i[:Bs], s_i[Bs:], s_n[:n_s], s_n[n_s:]),
            (gate[:n_s], gate[n_s:]))


# ------------------------------------------------------------------------------ modules
class _ImageDA(nn.Module):
    """lib/US_DAF/DA.py:36-51: GRL(0.1) -> 1x1 dim->512 -> ReLU -> 1x1 512->1 -> sigmoid (no
    biases)."""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim
        self.Conv1 = Conv2d(dim, 512, 1, bias=False, relu=True)
        self.Conv2 = Conv2d(512, 1, 1, bias=False)

    def score(self, x):
        """The domain logits (the fused loss applies the sigmoid)."""
        return self.Conv2(self.Conv1(grad_reverse(x)))

    def forward(self, x):
        return torch.sigmoid(self.score(x))


class class_ImageDA(nn.Module):
    """lib/US_DAF/DA.py:54-67: constructed by the reference and never called.  Parameters
    only (frozen), so a reference checkpoint loads with strict=True."""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim
        self.Conv1 = nn.Conv2d(dim, 512, kernel_size=1, stride=1, bias=False)
        self.Conv2 = nn.Conv2d(512, 1, kernel_size=1, stride=1, bias=False)


class _InstanceDA(nn.Module):
    """lib/US_DAF/DA.py:69-89: GRL(0.1) -> fc 1024 -> ReLU -> Dropout -> fc 1024 -> ReLU ->
    Dropout -> fc 4 -> sigmoid; outputs [domain, small, middle, large].

    ``in_dim`` is 2048 for ResNet101 and 4096 for VGG16 (the reference hard-codes 2048, which
    breaks its VGG16 variant, DA.py:72)."""

    def __init__(self, in_dim=2048):
        super().__init__()
        self.dc_ip1 = Linear(in_dim, 1024)
        self.dc_relu1 = nn.ReLU()
        self.dc_drop1 = nn.Dropout(p=0.5)
        self.dc_ip2 = Linear(1024, 1024)
        self.dc_relu2 = nn.ReLU()
        self.dc_drop2 = nn.Dropout(p=0.5)
        self.clssifer = nn.Linear(1024, 4)

    def score(self, x):
        """The four logits (the fused loss applies the sigmoid)."""
        x = grad_reverse(x)
        x = relu_dropout(self.dc_ip1(x), self.dc_drop1, getattr(self.dc_ip1, "act_tap", None))
        x = relu_dropout(self.dc_ip2(x), self.dc_drop2, getattr(self.dc_ip2, "act_tap", None))
        return self.clssifer(x)

    def forward(self, x):
        return torch.sigmoid(self.score(x))


def _freeze(module):
    for p in module.parameters():
        p.requires_grad = False


class _fasterRCNN(daf._fasterRCNN):
    """lib/US_DAF/faster_rcnn.py:36-309 on DAF's detector plumbing."""

    def __init__(self, classes, class_agnostic):
        super().__init__(classes, class_agnostic)
        del self.consistency_loss
        self.RCNN_imageDA = _ImageDA(self.dout_base_model)
        self.RCNN_imageDA_class = class_ImageDA(self.dout_base_model)
        self.RCNN_instanceDA = _InstanceDA(self.instance_dim)
        _freeze(self.RCNN_imageDA_class)

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

    # ---------------------------------------------------------------- forward
    def forward(self, *args, gate_override=None):
        """The reference's 8 arguments (faster_rcnn.py:62-63), or the project's 10-tuple
        batch, whose entries 4 and 9 (the need_backprop pair) are ignored: US-DAF fixes the
        domain labels at 1 / 0 (:64-68); in eval mode the detector's 4 arguments.
        gate_override = (gate_s, gate_t): tests."""
        if len(args) == 4:
            if self.training:
                raise RuntimeError("US-DAF trains on a source and a target image: the "
                                   "4-argument forward is the eval-mode detector")
            return self._detect(*args)
        if len(args) == 10:
            args = args[:4] + args[5:9]
        if len(args) != 8:
            raise TypeError(f"US-DAF forward takes 8 (or 10, or in eval mode 4) tensors, "
                            f"got {len(args)}")
        (im_data, im_info, gt_boxes, num_boxes, tgt_im_data, tgt_im_info, _tgt_gt_boxes,
         _tgt_num_boxes) = args
        batch_size = im_data.size(0)
        im_info = im_info.detach()
        gt_boxes = gt_boxes.detach()
        same = (im_data.shape == tgt_im_data.shape) and batch_size == 1
        early = early_rpn(self, same)
        if same:
            base2 = self.RCNN_base(torch.cat([im_data, tgt_im_data], 0))
            base_feat, tgt_base_feat = base2[:1], base2[1:]
            rpn_in = base2.detach().requires_grad_(True) if early else base2
            score2, score_r2, prob2, bbox2 = self.RCNN_rpn.head(rpn_in)
            s_score, s_score_r, s_prob, s_bbox = score2[:1], score_r2[:1], prob2[:1], bbox2[:1]
            t_prob, t_bbox = prob2[1:], bbox2[1:]
        else:
            base_feat = self.RCNN_base(im_data)
            tgt_base_feat = self.RCNN_base(tgt_im_data)
            s_score, s_score_r, s_prob, s_bbox = self.RCNN_rpn.head(base_feat)
            _, _, t_prob, t_bbox = self.RCNN_rpn.head(tgt_base_feat)

        # source RPN in train mode (faster_rcnn.py:80-82), target RPN in eval mode (:202-204:
        # TEST proposals, no losses), both on side streams while this stream does the anchor
        # target, the RPN losses and the image-level DA head (independent of the proposals)
        rpn = self.RCNN_rpn
        pending = proposals_on_side_streams(rpn.RPN_proposal, [
            (s_prob.detach(), s_bbox.detach(), im_info, "TRAIN"),
            (t_prob.detach(), t_bbox.detach(), tgt_im_info.detach(), "TEST")])
        if same:
            rpn_loss_cls, rpn_loss_bbox, _ = rpn.losses(score2, score_r2, bbox2, gt_boxes, im_info,
                                                        num_boxes, rng=self.replay_rng, n_images=1)
        else:
            rpn_loss_cls, rpn_loss_bbox, _ = rpn.losses(s_score, s_score_r, s_bbox, gt_boxes,
                                                        im_info, num_boxes, rng=self.replay_rng)
        if early:
            rpn_loss_cls, rpn_loss_bbox = early_rpn_backward(
                rpn_loss_cls, rpn_loss_bbox, rpn_in, [(base2, lambda g: g)])
        if same:
            z_img2 = self.RCNN_imageDA.score(base2)
        rois, tgt_rois = pending.join()
        props = (rois.detach().clone(), tgt_rois.detach().clone()) if self.capture is not None \
            else None

        rois, rois_label, rois_target, rois_inside_ws, rois_outside_ws = \
            self.RCNN_proposal_target(rois, gt_boxes, num_boxes, rng=self.replay_rng)
        rois_label = rois_label.view(-1).long()
        rois_target = rois_target.view(-1, rois_target.size(2))
        rois_inside_ws = rois_inside_ws.view(-1, rois_inside_ws.size(2))
        rois_outside_ws = rois_outside_ws.view(-1, rois_outside_ws.size(2))

        n_s = rois.size(1)
        if same:
            t_rois = tgt_rois.view(-1, 5).clone()
            t_rois[:, 0] = 1.0  # target image is batch entry 1 of base2
            rois2 = torch.cat([rois.view(-1, 5), t_rois], 0)
            feat2 = self._head_to_tail(self._pool(base2, rois2))
        else:
            pooled_feat = self._head_to_tail(self._pool(base_feat, rois.view(-1, 5)))
            tgt_pooled_feat = self._head_to_tail(self._pool(tgt_base_feat, tgt_rois.view(-1, 5)))

        cls_prob, bbox_pred, RCNN_loss_cls, RCNN_loss_bbox = self._rcnn_losses(
            feat2 if same else pooled_feat, rois_label, rois_target, rois_inside_ws,
            rois_outside_ws)
        cls_prob = cls_prob.view(batch_size, n_s, -1)
        bbox_pred = bbox_pred.view(batch_size, n_s, -1)

        # DA heads (faster_rcnn.py:264-282): the scale labels come from the sampled source
        # RoIs and the 300 TEST proposals of the target, zero-padded rows included
        if same:
            z_ins2 = self.RCNN_instanceDA.score(feat2)
            da, _, gate = us_daf_da_losses_packed(z_img2, z_ins2, rois2, 1, n_s, gate_override)
        else:
            da, _, gate = us_daf_da_losses(
                self.RCNN_imageDA.score(base_feat), self.RCNN_imageDA.score(tgt_base_feat),
                self.RCNN_instanceDA.score(pooled_feat),
                self.RCNN_instanceDA.score(tgt_pooled_feat), rois, tgt_rois, gate_override)
        if self.capture is not None:
            self.capture.update(s_rois=props[0], t_rois=props[1],
                                gate=tuple(g.detach().clone() for g in gate))
        DA_img_loss_cls, DA_ins_loss_cls, tgt_DA_img_loss_cls, tgt_DA_ins_loss_cls = da
        return (rois, cls_prob, bbox_pred, rpn_loss_cls, rpn_loss_bbox, RCNN_loss_cls,
                RCNN_loss_bbox, rois_label, DA_img_loss_cls, DA_ins_loss_cls, tgt_DA_img_loss_cls,
                tgt_DA_ins_loss_cls)

    @staticmethod
    def total_loss(out, lamda=0.1):
        """methods/US_DAF/US_DAF_train.py:428-431."""
        return weighted_loss_sum(tuple(out[3:7]) + tuple(out[8:12]), (1, 1, 1, 1) + (lamda,) * 4)

    def _init_weights(self):
        """faster_rcnn.py:288-306 (normal_init, truncated=False)."""
        super()._init_weights()
        self.RCNN_cls_score_img.weight.data.normal_(0, 0.01)
        self.RCNN_cls_score_img.bias.data.zero_()


class vgg16(_fasterRCNN):
    """lib/US_DAF/vgg16.py (random init: the pretrained caffe weights are external).  Defines
    RCNN_cls_score_img, which the reference's _init_weights needs and its vgg16.py lacks."""

    FUSE_POOLS = daf.vgg16.FUSE_POOLS

    def __init__(self, classes, pretrained=False, class_agnostic=False):
        self.dout_base_model = 512
        self.instance_dim = 4096
        self.pretrained = pretrained
        self.class_agnostic = class_agnostic
        _fasterRCNN.__init__(self, classes, class_agnostic)

    def _init_modules(self):
        daf.vgg16._init_modules(self)
        self.RCNN_cls_score_img = nn.Linear(1, self.n_classes)
        _freeze(self.RCNN_cls_score_img)

    def _head_to_tail(self, pool5):
        return self.RCNN_top(pool5.view(pool5.size(0), -1))


class resnet(_fasterRCNN):
    """lib/US_DAF/resnet.py:220-290 (ResNet101; random init — the caffe weights are
    external).  RCNN_cls_score_img (resnet.py:249) is never called: frozen parameters."""

    def __init__(self, classes, num_layers=101, pretrained=False, class_agnostic=False):
        if num_layers != 101:
            raise NotImplementedError("only ResNet101")
        self.dout_base_model = 1024
        self.instance_dim = 2048
        self.pretrained = pretrained
        self.class_agnostic = class_agnostic
        _fasterRCNN.__init__(self, classes, class_agnostic)

    def _init_modules(self):
        daf.resnet._init_modules(self)
        self.RCNN_cls_score_img = nn.Linear(1, self.n_classes)
        _freeze(self.RCNN_cls_score_img)

    train = daf.resnet.train
    _pool = daf.resnet._pool
    _head_to_tail = daf.resnet._head_to_tail
