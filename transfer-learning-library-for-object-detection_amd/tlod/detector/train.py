"""The DAF training step (methods/DAF/DAF_train.py:353-408) on the tlod path, plus the
synthetic Cityscapes->Foggy batch source used by bench.py / smoke().

Per step (one source + one target image): forward -> loss sum with lamda * DA terms
(:397-400) -> backward -> clip_gradient(10) for VGG16 (:406-407, here device-side with
no .item()) -> SGD(momentum 0.9; biases 2x lr, no weight decay; weights lr, wd 5e-4)
(:311-325), or Adam over the same groups (``--o adam``, :320-325).  Optional gradient all-reduce hook (tlod.dist) runs inside backward.
"""
import math

import numpy as np
import torch

from ..config import cfg, setup_training_cfg

from ..data.imdb import CITYSCAPE_CLASSES as CITYSCAPES_CLASSES  # cityscape.py:51-54


METHODS = ("faster_rcnn", "daf", "maf", "atf", "pt_maf", "us_daf", "idf", "pa_atf")


def build_model(method, device, net="vgg16", classes=CITYSCAPES_CLASSES, seed=0,
                dataset="cityscape"):
    """<method>.<net>(classes).create_architecture() (methods/<M>/<M>_train.py), random
    init (the pretrained caffe weights are external downloads).  method "faster_rcnn" is
    the source-only detector (lib/model/faster_rcnn, methods/faster_rcnn); it is also
    PT-MAF's teacher (put it in eval mode)."""
    if method not in METHODS:
        raise ValueError(f"unknown method {method!r} (have {METHODS})")
    if net not in ("vgg16", "res101"):
        raise ValueError(f"unknown backbone {net!r}")
    import importlib
    mod = importlib.import_module(".faster_rcnn" if method == "faster_rcnn" else f"..da.{method}",
                                  __package__)
    if net == "res101" and not hasattr(mod, "resnet"):
        raise NotImplementedError(f"{method} with ResNet101")
    setup_training_cfg(net, dataset)
    torch.manual_seed(seed)
    if net == "vgg16":
        m = mod.vgg16(classes, pretrained=False, class_agnostic=False)
    else:
        m = mod.resnet(classes, 101, pretrained=False, class_agnostic=False)
    m.create_architecture()
    m.net = net
    return m.to(device).train()


def build_daf_vgg16(device, classes=CITYSCAPES_CLASSES, seed=0):
    return build_model("daf", device, "vgg16", classes, seed)


def make_optimizer(model, lr, momentum=None, weight_decay=None, double_bias=None, bias_decay=None,
                   fused=True, clip=None, optimizer="sgd", betas=None, eps=None):
    """DAF_train.py:311-325 param groups (collapsed to two groups — same update).
    optimizer: "sgd" or "adam" (the reference's --o; Adam with torch's defaults unless betas /
    eps are given).  fused=True: libtlod's fused clip_gradient(clip) + update
    (tlod.optim.FusedSGDClip / FusedAdamClip); fused=False: the torch optimizer.
    clip None: 10 for VGG16, none for ResNet101 (DAF_train.py:406-407)."""
    if optimizer not in ("sgd", "adam"):
        raise ValueError(f"unknown optimizer {optimizer!r} (have 'sgd', 'adam')")
    if clip is None:
        clip = default_clip(model)
    momentum = cfg.TRAIN.MOMENTUM if momentum is None else momentum
    wd = cfg.TRAIN.WEIGHT_DECAY if weight_decay is None else weight_decay
    double_bias = cfg.TRAIN.DOUBLE_BIAS if double_bias is None else double_bias
    bias_decay = cfg.TRAIN.BIAS_DECAY if bias_decay is None else bias_decay
    biases, weights = [], []
    for k, v in model.named_parameters():
        if v.requires_grad:
            (biases if "bias" in k else weights).append(v)
    groups = [{"params": weights, "lr": lr, "weight_decay": wd},
              {"params": biases, "lr": lr * (double_bias + 1),
               "weight_decay": wd if bias_decay else 0.0}]
    if optimizer == "adam":
        kw = {}
        if betas is not None:
            kw["betas"] = tuple(betas)
        if eps is not None:
            kw["eps"] = eps
        if fused:
            from ..optim import FusedAdamClip
            return FusedAdamClip(groups, clip_norm=clip, **kw)
        return torch.optim.Adam(groups, lr=lr, **kw)
    if fused:
        from ..optim import FusedSGDClip
        return FusedSGDClip(groups, momentum=momentum, clip_norm=clip)
    return torch.optim.SGD(groups, lr=lr, momentum=momentum, foreach=True)


@torch.no_grad()
def clip_gradient_(params, clip_norm):
    """net_utils.py:38-49 without the host sync: total = sqrt(sum ||g||^2);
    g *= clip / max(total, clip)."""
    grads = [p.grad for p in params if p.requires_grad and p.grad is not None]
    if not grads:
        return None
    norms = torch._foreach_norm(grads)
    total = torch.linalg.vector_norm(torch.stack(norms))
    scale = clip_norm / torch.clamp(total, min=clip_norm)
    torch._foreach_mul_(grads, scale)
    return total


class SyntheticCityscapes:
    """Synthetic batches of the reference's input tensors:
    BGR uint8 uniform[0,255] at 600x1200 minus PIXEL_MEANS (NCHW fp32); source gt = 8
    boxes (x1 in [0,W-64), size 32..400, clipped, class 1..8) padded to 50;
    target gt = [1,1,1,1,1] (roibatchLoader.py:217-226), or with tgt_G > 0 that many
    source-style boxes (IDF's pseudo labels).  A small pool of batches is made resident on the
    device up front so the timed loop reads HBM only."""

    def __init__(self, device, H=600, W=1200, G=8, max_gt=50, pool=4, seed=1000, n_classes=8,
                 tgt_G=0):
        self.device = torch.device(device)
        rng = np.random.default_rng(seed)
        means = torch.tensor(cfg.PIXEL_MEANS.reshape(3), dtype=torch.float32)
        self.batches = []
        for _ in range(pool):
            def img():
                u8 = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
                return (u8.float() - means).permute(2, 0, 1).contiguous()[None]
            def boxes(n):
                gt = np.zeros((1, max_gt, 5), np.float32)
                x1 = rng.uniform(0, W - 64, n)
                y1 = rng.uniform(0, H - 64, n)
                w = rng.uniform(32, 400, n)
                h = rng.uniform(32, 400, n)
                gt[0, :n, 0] = x1
                gt[0, :n, 1] = y1
                gt[0, :n, 2] = np.minimum(x1 + w, W - 1)
                gt[0, :n, 3] = np.minimum(y1 + h, H - 1)
                gt[0, :n, 4] = rng.integers(1, n_classes + 1, n)
                return torch.from_numpy(gt)
            gt = boxes(G)
            info = torch.tensor([[H, W, 600.0 / 1024.0]], dtype=torch.float32)
            d = self.device
            src = (img().to(d), info.to(d), gt.to(d),
                   torch.tensor([G], dtype=torch.int64, device=d), torch.ones(1, device=d))
            tgt_img = img().to(d)
            if tgt_G > 0:  # drawn after everything the default batch draws
                tgt_gt = boxes(tgt_G).to(d)
                tgt_num = torch.tensor([tgt_G], dtype=torch.int64, device=d)
            else:
                tgt_gt = torch.ones((1, 5), device=d)
                tgt_num = torch.zeros(1, dtype=torch.int64, device=d)
            self.batches.append(src + (tgt_img, info.clone().to(d), tgt_gt, tgt_num,
                                       torch.zeros(1, device=d)))
        self.i = 0

    def next(self):
        b = self.batches[self.i % len(self.batches)]
        self.i += 1
        return b


def daf_loss(out, lamda=0.1):
    from ..da.daf import _fasterRCNN
    return _fasterRCNN.total_loss(out, lamda)


def default_clip(model):
    """clip_gradient's norm: 10 for VGG16, none for ResNet101 (DAF_train.py:406-407); a model
    with its own ``clip_norm`` (IDF: 0, its training script never clips) says so."""
    own = getattr(model, "clip_norm", None)
    if own is not None:
        return float(own)
    return 10.0 if getattr(model, "net", "vgg16") == "vgg16" else 0.0


def train_step(model, optimizer, batch, lamda=0.1, clip=None, reducer=None):
    """One DAF/MAF/ATF iteration (the method's own loss sum, model.total_loss); returns the
    loss as a device tensor (no host sync)."""
    from ..optim import FusedClipOptimizer
    fused = isinstance(optimizer, FusedClipOptimizer)
    if reducer is not None:
        reducer.zero_grad()  # grads are views into the arena the reducer all-reduces
    else:
        optimizer.zero_grad(set_to_none=True)
    out = model(*batch)
    loss = model.total_loss(out, lamda)
    loss.backward()
    scale = 1.0
    if reducer is not None:
        reducer.finish(scale=not fused)  # SUM all-reduce; the fused step applies 1/world
        scale = reducer.grad_scale
    if fused:
        optimizer.step(grad_scale=scale)  # clip_gradient + SGD / Adam fused
    else:
        clip = default_clip(model) if clip is None else clip
        if clip:
            clip_gradient_([p for p in model.parameters()], clip)
        optimizer.step()
    return loss.detach()


def pt_maf_train_step(model, teacher, optimizer, batch, lamda=0.1, T=3.0, high=0.7, low=0.1,
                       alpha=1.0, beta=1.0, gamma=1.0, reducer=None):
    """One PT-MAF iteration (methods/PT_MAF/PT_MAF_train.py:434-464): the student's forward,
    the frozen teacher (a tlod.detector.faster_rcnn.vgg16 in eval mode, under no_grad and
    unknown to the optimizer) on the source image and the student's sampled RoIs, the loss
    sum with the KD term, backward, then as train_step.  Returns the loss as a device tensor
    (no host sync)."""
    from ..da.pt_maf import kd_loss, kd_teacher
    from ..optim import FusedClipOptimizer
    fused = isinstance(optimizer, FusedClipOptimizer)
    if reducer is not None:
        reducer.zero_grad()
    else:
        optimizer.zero_grad(set_to_none=True)
    out = model(*batch, T=T, high=high, low=low, alpha=alpha, beta=beta, gamma=gamma)
    teacher_out = kd_teacher(teacher, batch[0], batch[1], batch[2], batch[3], out[0], T)
    loss = model.total_loss(out, lamda, kd_loss(model, teacher_out, out[7], T))
    loss.backward()
    scale = 1.0
    if reducer is not None:
        reducer.finish(scale=not fused)
        scale = reducer.grad_scale
    if fused:
        optimizer.step(grad_scale=scale)
    else:
        clip = default_clip(model)
        if clip:
            clip_gradient_([p for p in model.parameters()], clip)
        optimizer.step()
    return loss.detach()


def idf_forward(model, batch, separation=True, eta=1.0):
    """The two calls of an IDF iteration over the project's 10-tuple batch: the source image
    with its ground truth (IDF_train.py:228), then the target image with ``target=True``, the
    batch's target gt_boxes / num_boxes as the pseudo boxes and the reference's single all-zero
    box for the main stack (:277-286).  Returns (out_s, out_t), the model's 20-tuples."""
    im, info, gt, num, _, t_im, t_info, t_gt, t_num, _ = batch
    out_s = model(im, info, gt, num, gt, num, separation, False, eta)
    out_t = model(t_im, t_info, t_gt.new_zeros((1, 1, 5)), t_num.new_zeros(1),
                  t_gt.view(1, -1, 5), t_num, separation, True, eta)
    return out_s, out_t


def _idf_step(model, optimizer, batch, separation, gamma, eta, reducer, ef, target_gate=None):
    """zero_grad, the two calls, the loss sum, backward, update (no gradient clipping)."""
    from ..optim import FusedClipOptimizer
    fused = isinstance(optimizer, FusedClipOptimizer)
    if reducer is not None:
        reducer.zero_grad()
    else:
        optimizer.zero_grad(set_to_none=True)
    out_s, out_t = idf_forward(model, batch, separation, eta)
    if ef or target_gate is not None:
        loss = model.total_loss(out_s, out_t, separation, gamma, ef, target_gate)
    else:
        loss = model.total_loss(out_s, out_t, separation, gamma)
    loss.backward()
    scale = 1.0
    if reducer is not None:
        reducer.finish(scale=not fused)
        scale = reducer.grad_scale
    if fused:
        optimizer.step(grad_scale=scale)
    else:
        clip = default_clip(model)
        if clip:
            clip_gradient_([p for p in model.parameters()], clip)
        optimizer.step()
    return loss.detach()


def idf_train_step(model, optimizer, batch, separation=True, gamma=3.0, eta=1.0, reducer=None,
                   ef=False):
    """One IDF iteration (methods/IDF/IDF_train.py:223-339) over the project's 10-tuple batch:
    the source call on the ground truth, the target call (``target=True``) with the batch's
    target gt_boxes / num_boxes as the pseudo boxes and the reference's single all-zero box
    for the main stack (:277-280), the loss sum (model.total_loss; ``ef``: EFocalLoss on the
    instance rows, :162-165), backward, update.  No gradient clipping.  Returns the loss as a
    device tensor (no host sync)."""
    return _idf_step(model, optimizer, batch, separation, gamma, eta, reducer, ef)


SELFTRAIN_SEED_OFFSET = 104729  # keeps the labels' draws apart from the sampling layers' seeds


def idf_selftrain_step(model, labeler, optimizer, batch, thresh=0.5, seed=None, ef=False,
                       separation=True, gamma=3.0, eta=1.0, reducer=None, class_agnostic=False,
                       max_gt=None, im_info_host=None):
    """One IDF iteration whose pseudo boxes are made inside the step (online self-training):
    ``labeler`` — a frozen eval-mode detector, e.g. ``build_model("faster_rcnn", ...).eval()`` —
    labels the batch's target image (tlod.eval.pseudo.label_image: its forward, tlod_detect_f32
    at ``thresh``, tlod_pseudo_gt_f32), and idf_train_step's body runs with those boxes in place
    of ``batch[7:9]``.

    A target image that gets no label contributes its domain and separation terms only: the
    target call's four detection losses are multiplied by ``num_boxes_p > 0`` on the device.
    (The reference labels offline and its roidb filter drops such an image from the target set
    altogether; inside a step there is nothing to skip to without a host sync.)

    seed: the base of the labels' random cap (None: cfg.RNG_SEED); the per-step seed is derived
    from it and a call counter kept on ``model``, as the sampling layers derive theirs.
    im_info_host: (height, width, scale) of the target blob as host numbers; without it
    ``batch[6]`` is read back, which is the step's one host sync.
    Returns (loss, num_boxes_p), device tensors."""
    from ..eval.pseudo import label_image
    if im_info_host is None:
        im_info_host = batch[6].reshape(-1, 3)[0].tolist()
    calls = getattr(model, "_selftrain_calls", 0) + 1
    model._selftrain_calls = calls
    base = int(cfg.RNG_SEED if seed is None else seed) + SELFTRAIN_SEED_OFFSET
    gt_p, num_p = label_image(labeler, batch[5], im_info_host, thresh, class_agnostic, max_gt,
                              seed=(base * 1000003 + calls) & 0xFFFFFFFFFFFFFFFF)
    batch = tuple(batch[:7]) + (gt_p, num_p) + tuple(batch[9:])
    loss = _idf_step(model, optimizer, batch, separation, gamma, eta, reducer, ef,
                     target_gate=num_p > 0)
    return loss, num_p


def smoke_step(device, method="daf", net="vgg16"):
    """One tiny <method>-<net> forward+backward+update on `device` (used by smoke())."""
    model = build_model(method, device, net)
    opt = make_optimizer(model, 2e-3)
    data = SyntheticCityscapes(device, H=192, W=320, G=4, pool=1, seed=7)
    loss = train_step(model, opt, data.next())
    torch.cuda.synchronize()
    v = float(loss)
    assert math.isfinite(v), f"non-finite {method} loss {v}"
    return v
