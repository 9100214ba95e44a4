"""US-DAF (tlod.da.us_daf) on the device against the CPU restatement (tests/ref_us_daf.py) with
the same weights, replayed draws, the device's proposals (rois_override) and the device's
BCEloss_margin gates (gate_override).

Bars: the eight losses within 1e-4 relative; sampled RoIs identical; gradients under
tests/helpers.pattern_grad_bar; the device's own gates against the oracle's own: at most 1 % of
the rows differ, each with its oracle column-0 element loss within 1e-3 * max(1, max|z0|) of
0.5 (the project's 1e-3 relative activation bar pushed through |dL/dz| <= 1).

A random-init instance head puts most rows of a domain on one side of the gate (VGG16 seed 0:
source 256 on / 0 off), so the set-up rescales row 0 of clssifer: z0 -> SCALE * z0 + SHIFT,
constants chosen per case with the CPU oracle so that both domains hold at least 16 gated-on
and 16 gated-off rows and no oracle row lies inside three times the band above.  Counts on /
off, source then target, of the CPU oracle on its own proposals (the device, on its own
proposals, gave the same but for seed 2's source in the training-mode run: 157 / 99):
    VGG16 192x320 seed 0     (3.81, 1.92):       173 / 83,  176 / 124
    VGG16 224x352 seed 2     (3.96, 1.84):       158 / 98,  176 / 124
    ResNet101 224x320 seed 0 (2.59e-5, -4.62):    63 / 65,  226 / 74
A random-init ResNet101 (no pretrained statistics behind its frozen BatchNorms) has activations
near 1e5: the RPN's box deltas overflow, every box clips to the image and NMS leaves 5 target
proposals plus 295 identical zero-padded rows — no 16 / 16 split exists.  The ResNet101 set-up
therefore also scales RPN_bbox_pred's weights by 1e-6 (300 distinct target proposals).
One case keeps the untouched init.
"""
import numpy as np
import pytest
import torch

from helpers import arm_taps, pattern_grad_bar, record_pattern
from ref_us_daf import LOSSES, OracleUSDAF, total_loss
from test_losses_gpu import close

pytestmark = pytest.mark.gpu
dev = "cuda"

IDX = [3, 4, 5, 6, 8, 9, 10, 11]
# (net, H, W, seed) -> (SCALE, SHIFT) of clssifer's row 0
RESHAPE = {("vgg16", 192, 320, 0): (3.81, 1.92),
           ("vgg16", 224, 352, 2): (3.96, 1.84),
           ("res101", 224, 320, 0): (2.59e-5, -4.62)}
CASES = list(RESHAPE)
R101_BBOX_SCALE = 1e-6


def _models(net, seed, reshape=None, **kw):
    from tlod.detector.train import build_model
    m = build_model("us_daf", dev, net, seed=seed, **kw)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    if reshape is not None:
        with torch.no_grad():
            c = m.RCNN_instanceDA.clssifer
            c.weight[0].mul_(reshape[0])
            c.bias[0].mul_(reshape[0]).add_(reshape[1])
            if net == "res101":
                m.RCNN_rpn.RPN_bbox_pred.weight.mul_(R101_BBOX_SCALE)
    o = OracleUSDAF(dropout=0.0, backbone=net).train()
    o.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
    return m, o


def _batch(H, W, seed, tgt_W=None):
    from oracle.daf_step import synthetic_batch
    b = synthetic_batch(H, W, seed=seed)
    if tgt_W is not None:
        b = b[:5] + synthetic_batch(H, tgt_W, seed=seed)[5:]
    return b


def _device_step(m, gpu_batch, backward=True, eight=False, **kw):
    m.replay_rng = np.random.RandomState(3)
    m.capture = {}
    args = gpu_batch[:4] + gpu_batch[5:9] if eight else gpu_batch
    out = m(*args, **kw)
    assert len(out) == 12
    if backward:
        m.total_loss(out, 0.1).backward()
    return out


def _overrides(m):
    ov = (m.capture["s_rois"].cpu().numpy(), m.capture["t_rois"].cpu().numpy())
    return ov, tuple(g.cpu() for g in m.capture["gate"])


def _assert_losses(out, ref):
    for name, i in zip(LOSSES, IDX):
        g, r = float(out[i].detach()), float(ref[name].detach())
        print(name, g, r)
        assert abs(g - r) <= 1e-4 * max(abs(r), 1e-3), (name, g, r)


def _counts(gates):
    return [(int(g.sum()), int(g.numel() - g.sum())) for g in gates]


def _assert_own_gates(gates, ref):
    """The device's gates against the oracle's own (ref carries them beside an override): at
    most 1 % of a domain's rows differ, each with its oracle column-0 loss inside the band; the
    oracle holds at most 1 % of its rows inside that band and 16 rows on either side."""
    for pre, g in zip(("", "t_"), gates):
        rg, col0, z0 = ref[pre + "gate"], ref[pre + "col0"], ref[pre + "z0"]
        band = 1e-3 * max(1.0, float(z0.abs().max()))
        inside = int(((col0 - 0.5).abs() <= band).sum())
        diff = g != rg
        print(pre, "device on", int(g.sum()), "oracle on", int(rg.sum()), "differ", int(diff.sum()),
              "oracle rows in band", inside, "band", band)
        assert inside <= 0.01 * g.numel(), (pre, inside)
        assert int(rg.sum()) >= 16 and int(rg.numel() - rg.sum()) >= 16
        assert int(diff.sum()) <= 0.01 * g.numel(), (pre, int(diff.sum()))
        assert ((col0 - 0.5).abs()[diff] <= band).all(), pre


@pytest.mark.parametrize("net,H,W,seed", CASES)
def test_us_daf_losses_and_grads_match_oracle(net, H, W, seed):
    m, o = _models(net, seed, RESHAPE[(net, H, W, seed)])
    cpu_batch = _batch(H, W, seed + 1)
    gpu_batch = tuple(t.to(dev) for t in cpu_batch)
    taps = arm_taps(m)
    out = _device_step(m, gpu_batch, eight=True)  # the reference's 8-argument signature
    ov, gates = _overrides(m)
    print("gates on / off", _counts(gates))
    for on, off in _counts(gates):
        assert on >= 16 and off >= 16, _counts(gates)
    assert gates[0].numel() == out[7].numel() and gates[1].numel() == 300
    box = {}

    def step(mod, b):
        box["ref"] = mod(b, np.random.RandomState(3), rois_override=ov, gate_override=gates)
        return total_loss(box["ref"], 0.1)

    own = record_pattern(o, lambda: step(o, cpu_batch).backward())
    ref = box["ref"]
    _assert_losses(out, ref)
    _assert_own_gates(gates, ref)  # the training-mode run's gates, too
    np.testing.assert_array_equal(out[0].cpu().numpy().reshape(-1, 5), ref["rois"].reshape(-1, 5))
    for k in ("RCNN_imageDA_class.Conv1.weight", "RCNN_cls_score_img.weight"):
        assert dict(m.named_parameters())[k].grad is None
    pattern_grad_bar(m, o, step, cpu_batch, taps, out[7].numel(), own)


def test_us_daf_untouched_init_matches_oracle():
    """The untouched random init (no gate reshape), through the 10-tuple batch."""
    m, o = _models("vgg16", 0)
    cpu_batch = _batch(192, 320, 1)
    out = _device_step(m, tuple(t.to(dev) for t in cpu_batch))
    ov, gates = _overrides(m)
    print("gates on / off", _counts(gates))
    with torch.no_grad():
        ref = o(cpu_batch, np.random.RandomState(3), rois_override=ov, gate_override=gates)
    _assert_losses(out, ref)
    np.testing.assert_array_equal(out[0].cpu().numpy().reshape(-1, 5), ref["rois"].reshape(-1, 5))
    for name, p in m.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all(), name


@pytest.mark.parametrize("net,H,W,seed", CASES)
def test_us_daf_own_gates_without_override(net, H, W, seed):
    """The device's gates from its own logits against the oracle's own."""
    m, o = _models(net, seed, RESHAPE[(net, H, W, seed)])
    cpu_batch = _batch(H, W, seed + 1)
    with torch.no_grad():
        _device_step(m, tuple(t.to(dev) for t in cpu_batch), backward=False)
        ov, gates = _overrides(m)
        ref = o(cpu_batch, np.random.RandomState(3), rois_override=ov)
    _assert_own_gates(gates, ref)


def test_us_daf_gate_override_reaches_the_loss():
    """gate_override replaces the device's own gates: all-on and all-off gates give different
    instance losses, each matching the oracle under the same override."""
    m, o = _models("vgg16", 0, RESHAPE[CASES[0]])
    cpu_batch = _batch(192, 320, 1)
    gpu_batch = tuple(t.to(dev) for t in cpu_batch)
    seen = []
    with torch.no_grad():
        for fill in (1.0, 0.0):
            gates = (torch.full((256,), fill), torch.full((300,), fill))
            out = _device_step(m, gpu_batch, backward=False,
                               gate_override=tuple(g.to(dev) for g in gates))
            ov, got = _overrides(m)
            assert torch.equal(got[0], gates[0]) and torch.equal(got[1], gates[1])
            _assert_losses(out, o(cpu_batch, np.random.RandomState(3), rois_override=ov,
                                  gate_override=gates))
            seen.append((float(out[9]), float(out[11])))
    assert seen[0][0] > seen[1][0] and seen[0][1] > seen[1][1]


def test_us_daf_fused_matches_unfused(monkeypatch):
    """TLOD_FUSED_LOSSES=0 (the torch compositions) in the same process: the same losses,
    identical gates."""
    m, _ = _models("vgg16", 0, RESHAPE[CASES[0]])
    gpu_batch = tuple(t.to(dev) for t in _batch(192, 320, 1))
    with torch.no_grad():
        out = _device_step(m, gpu_batch, backward=False)
        _, gates = _overrides(m)
        monkeypatch.setenv("TLOD_FUSED_LOSSES", "0")
        out0 = _device_step(m, gpu_batch, backward=False)
        _, gates0 = _overrides(m)
    assert torch.equal(out[0], out0[0])
    for i in IDX:
        close(out[i], out0[i])
    assert torch.equal(gates[0], gates0[0]) and torch.equal(gates[1], gates0[1])


def test_us_daf_two_pass_path_matches_oracle():
    """Differently sized source / target images (192x320, 192x336) take the two-pass path (one
    backbone / head pass per image, the separate-layout loss launch).  The oracle is per-image
    by construction, and the batched path is held to it above, so the two paths agree when
    this one meets the same 1e-4."""
    m, o = _models("vgg16", 5)
    cpu_batch = _batch(192, 320, 6, tgt_W=336)
    assert cpu_batch[0].shape != cpu_batch[5].shape
    with torch.no_grad():
        out = _device_step(m, tuple(t.to(dev) for t in cpu_batch), backward=False)
        ov, gates = _overrides(m)
        print("gates on / off", _counts(gates))
        ref = o(cpu_batch, np.random.RandomState(3), rois_override=ov, gate_override=gates)
    _assert_losses(out, ref)


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_us_daf_train_step_leaves_frozen_modules_alone(optimizer):
    from tlod.detector.train import SyntheticCityscapes, make_optimizer, train_step
    m, _ = _models("vgg16", 0)
    opt = make_optimizer(m, 1e-3, optimizer=optimizer)
    data = SyntheticCityscapes(dev, H=192, W=320, G=4, pool=1, seed=7)
    dead = {k: v.detach().clone() for k, v in m.named_parameters()
            if k.startswith(("RCNN_imageDA_class.", "RCNN_cls_score_img."))}
    assert len(dead) == 4
    before = {k: v.detach().clone() for k, v in m.named_parameters() if v.requires_grad}
    assert not set(dead) & set(before)
    loss = train_step(m, opt, data.next())
    assert torch.isfinite(loss)
    params = dict(m.named_parameters())
    for k, v in dead.items():
        assert params[k].grad is None and torch.equal(params[k].detach(), v), k
    changed = [k for k in before if not torch.equal(params[k].detach(), before[k])]
    assert len(changed) > 0.9 * len(before), (len(changed), len(before))


def test_us_daf_eval_path():
    """im_detect on a US-DAF model: the 4-argument eval-mode forward, per-class arrays."""
    from tlod.eval.detect import im_detect
    m, _ = _models("vgg16", 0)
    b = tuple(t.to(dev) for t in _batch(192, 320, 1))
    per_class = im_detect(m, b[0], b[1], b[2], b[3])
    assert len(per_class) == m.n_classes and m.training
    assert all(d.ndim == 2 and d.shape[1] == 5 for d in per_class)
    assert sum(len(d) for d in per_class[1:]) > 0


def test_us_daf_smoke_step_res101():
    from tlod.detector.train import smoke_step
    assert np.isfinite(smoke_step(dev, "us_daf", "res101"))


def test_us_daf_published_configuration():
    """PASCAL VOC -> Clipart with ResNet101 (the reference README's US-DAF result): 21 classes,
    9 anchors, 20 gt boxes; one finite training step at 192x320."""
    from tlod.data.imdb import VOC_CLASSES
    from tlod.detector.train import SyntheticCityscapes, build_model, make_optimizer, train_step
    m = build_model("us_daf", dev, "res101", VOC_CLASSES, dataset="VOC2clipart")
    assert m.n_classes == 21 and m.RCNN_rpn.nc_score_out == 18
    opt = make_optimizer(m, 1e-3)
    data = SyntheticCityscapes(dev, H=192, W=320, G=4, max_gt=20, pool=1, seed=7, n_classes=20)
    loss = train_step(m, opt, data.next())
    assert torch.isfinite(loss)
    assert all(torch.isfinite(p).all() for p in m.parameters())
