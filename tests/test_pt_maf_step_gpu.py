"""PT-MAF (tlod.da.pt_maf) on the device against the CPU restatement (tests/ref_pt_maf.py)
with the same weights, replayed draws, the device's proposals (rois_override) and the
device's foreground / background maps (maps_override).

Bars: the eight MAF-named losses and the KD loss within 1e-4 relative; sampled RoIs
identical; gradients under tests/helpers.pattern_grad_bar; the device's own maps against the
oracle's own: at most 1 % of cells differ, each within 1e-5 * m of its threshold.

A random-init RPN has no background cells (b is empty at low = 0.1), so the set-up scales
RPN_cls_score's weights by SCALE and lowers its object-side biases by SHIFT — chosen with the
CPU oracle so that f and b hold at least 4 cells on both images of every parametrised seed
(seed 0 at 192x320: f 22 / 17, b 160 / 149 cells; seed 2 at 224x352: f 19 / 24, b 169 / 165;
no cell within 1e-5 * m of a threshold).  One case keeps the untouched init (b empty).
"""
import numpy as np
import pytest
import torch

from helpers import arm_taps, pattern_grad_bar, record_pattern
from ref_pt_maf import LOSSES, OraclePTMAF, make_teacher, teacher_outputs, total_loss
from test_losses_gpu import close

pytestmark = pytest.mark.gpu
dev = "cuda"

IDX = [3, 4, 5, 6, 8, 9, 10, 11]
SCALE, SHIFT = 6.0, 16.0
HEADS = ("RCNN_imageDA_3_f", "RCNN_imageDA_3_b", "RCNN_imageDA_4_f", "RCNN_imageDA_4_b",
         "RCNN_imageDA_f", "RCNN_imageDA_b")


def _device_models(seed, reshape=True):
    from tlod.detector.train import build_model
    m = build_model("pt_maf", dev, seed=seed)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    if reshape:
        with torch.no_grad():
            cls = m.RCNN_rpn.RPN_cls_score
            cls.weight.mul_(SCALE)
            cls.bias[m.num_anchor:].sub_(SHIFT)
    teacher = build_model("faster_rcnn", dev, seed=seed + 100).eval()
    return m, teacher


def _oracles(m, teacher):
    o = OraclePTMAF(dropout=0.0).train()
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()
          if not k.startswith(("conv3.", "conv34.", "conv45."))}  # views of RCNN_base
    o.load_state_dict(sd, strict=True)
    ot = make_teacher()
    ot.load_state_dict({k: v.detach().cpu() for k, v in teacher.state_dict().items()},
                       strict=True)
    return o, ot.eval()


def _batch(H, W, seed, tgt_W=None):
    from oracle.daf_step import synthetic_batch
    b = synthetic_batch(H, W, seed=seed)
    if tgt_W is not None:
        b = b[:5] + synthetic_batch(H, tgt_W, seed=seed)[5:]
    return b


def _arm(m):
    """helpers.arm_taps stops at the RPN for a model without RCNN_imageDA: add the six heads'
    ReLU sites (ref_pt_maf's names) and the instance head's."""
    taps = arm_taps(m)

    def add(site, mod, kind):
        mod.act_tap = []
        taps[site] = (mod.act_tap, kind)
    for side in ("f", "b"):
        add(f"ida_{side}", getattr(m, f"RCNN_imageDA_{side}").Conv1, "map")
        for lvl in (3, 4):
            h = getattr(m, f"RCNN_imageDA_{lvl}_{side}")
            add(f"ida{lvl}_{side}", h.Conv1, "map")
            add(f"drm{lvl}_{side}", h.DRM.conv_low_dim, "map")
    add("ip1", m.RCNN_instanceDA.dc_ip1, "ins")
    add("ip2", m.RCNN_instanceDA.dc_ip2, "ins")
    return taps


def _device_step(m, teacher, gpu_batch, backward=True, **kw):
    """Forward (+ teacher, KD, backward) with replayed draws; returns (out, kd, teacher_out)."""
    from tlod.da.pt_maf import kd_loss, kd_teacher
    m.replay_rng = np.random.RandomState(3)
    m.capture = {}
    out = m(*gpu_batch, **kw)
    assert len(out) == 14
    tout = kd_teacher(teacher, *gpu_batch[:4], out[0], kw.get("T", 3.0))
    kd = kd_loss(m, tout, out[7], kw.get("T", 3.0))
    if backward:
        m.total_loss(out, 0.1, kd).backward()
    return out, kd, tout


def _overrides(m):
    ov = (m.capture["s_rois"].cpu().numpy(), m.capture["t_rois"].cpu().numpy())
    return ov, tuple(x.cpu() for x in m.capture["maps"])


def _assert_losses(out, kd, ref, ref_kd):
    for name, i in zip(LOSSES, IDX):
        g, r = float(out[i].detach()), float(ref[name].detach())
        print(name, g, r)
        assert abs(g - r) <= 1e-4 * max(abs(r), 1e-3), (name, g, r)
    g, r = float(kd.detach()), float(ref_kd.detach())
    print("kd", g, r)
    assert abs(g - r) <= 1e-4 * max(abs(r), 1e-3), ("kd", g, r)


@pytest.mark.parametrize("H,W,seed", [(192, 320, 0), (224, 352, 2)])
def test_pt_maf_losses_and_grads_match_oracle(H, W, seed):
    m, teacher = _device_models(seed)
    o, ot = _oracles(m, teacher)
    cpu_batch = _batch(H, W, seed + 1)
    gpu_batch = tuple(t.to(dev) for t in cpu_batch)
    taps = _arm(m)
    out, kd, _ = _device_step(m, teacher, gpu_batch)
    ov, mo = _overrides(m)
    for cells in mo:
        assert int(cells.sum()) >= 4, [int(c.sum()) for c in mo]
    assert out[12].shape == (1, 2, 12 * (H // 16), W // 16) and out[13].shape == (256, 9)
    box = {}

    def step(mod, b, tout):
        r = mod(b, np.random.RandomState(3), rois_override=ov, maps_override=mo)
        box["ref"], box["kd"] = r, mod.kd(r, tout)
        return total_loss(r, 0.1, box["kd"])

    tout = teacher_outputs(ot, cpu_batch, out[0].cpu().numpy())
    own = record_pattern(o, lambda: step(o, cpu_batch, tout).backward())
    ref, ref_kd = box["ref"], box["kd"]
    _assert_losses(out, kd, ref, ref_kd)
    np.testing.assert_array_equal(out[0].cpu().numpy().reshape(-1, 5), ref["rois"].reshape(-1, 5))
    np.testing.assert_array_equal((out[7] > 0).cpu().numpy(), ref["rois_label"].numpy() > 0)
    assert all(p.grad is None for p in teacher.parameters())
    pattern_grad_bar(m, o, lambda mod, b: step(mod, b, tout), cpu_batch, taps, out[7].numel(), own)


def test_pt_maf_untouched_init_has_empty_b_and_stays_finite():
    """Random init: b is empty on both images; every loss is finite and the three b heads get
    exactly zero gradient (empty-map rule: loss 0, gradient 0, no NaN)."""
    m, teacher = _device_models(0, reshape=False)
    gpu_batch = tuple(t.to(dev) for t in _batch(192, 320, 1))
    out, kd, _ = _device_step(m, teacher, gpu_batch)
    _, mo = _overrides(m)
    assert int(mo[1].sum()) == 0 and int(mo[3].sum()) == 0 and int(mo[0].sum()) >= 1
    for i in IDX:
        assert torch.isfinite(out[i]).all(), i
    assert torch.isfinite(kd)
    for name, p in m.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all(), name
        if name.startswith(("RCNN_imageDA_3_b", "RCNN_imageDA_4_b", "RCNN_imageDA_b")):
            assert p.grad is None or torch.count_nonzero(p.grad).item() == 0, name


def test_pt_maf_conv3_quirk():
    """faster_rcnn.py:298: the source conv3 b term reads conv3_score_f, so with the target
    terms off RCNN_imageDA_3_b gets no gradient — on the device (a direct sum of the source
    outputs) and in the oracle — and with them on it does."""
    m, teacher = _device_models(0)
    o, _ = _oracles(m, teacher)
    cpu_batch = _batch(192, 320, 1)
    gpu_batch = tuple(t.to(dev) for t in cpu_batch)
    out, kd, _ = _device_step(m, teacher, gpu_batch, backward=False)
    ov, mo = _overrides(m)
    assert int(mo[1].sum()) >= 4 and int(mo[3].sum()) >= 4
    src = out[3] + out[4] + out[5] + out[6] + 0.1 * (out[8] + out[9]) + kd
    src.backward(retain_graph=True)
    head = dict(m.RCNN_imageDA_3_b.named_parameters())
    for k, p in head.items():
        assert p.grad is None or torch.count_nonzero(p.grad).item() == 0, k
    assert torch.count_nonzero(m.RCNN_imageDA_4_b.Conv2.weight.grad).item() > 0
    (0.1 * (out[10] + out[11])).backward()
    for k, p in head.items():
        assert torch.count_nonzero(p.grad).item() > 0, k

    ref = o(cpu_batch, np.random.RandomState(3), rois_override=ov, maps_override=mo)
    total_loss(ref, 0.1, 0.0, tgt=0.0).backward(retain_graph=True)
    for k, p in o.RCNN_imageDA_3_b.named_parameters():
        assert p.grad is None or torch.count_nonzero(p.grad).item() == 0, k
    (0.1 * ref["tgt_DA_img_loss_cls"]).backward()
    for k, p in o.RCNN_imageDA_3_b.named_parameters():
        assert torch.count_nonzero(p.grad).item() > 0, k


@pytest.mark.parametrize("H,W,seed", [(192, 320, 0), (224, 352, 2)])
def test_pt_maf_own_maps_without_override(H, W, seed):
    """The device's f / b from its own RPN probabilities against the oracle's own: at most
    1 % of the cells differ, each within 1e-5 * m of its threshold."""
    m, teacher = _device_models(seed)
    o, _ = _oracles(m, teacher)
    cpu_batch = _batch(H, W, seed + 1)
    with torch.no_grad():
        _device_step(m, teacher, tuple(t.to(dev) for t in cpu_batch), backward=False)
        ov, mo = _overrides(m)
        ref = o(cpu_batch, np.random.RandomState(3), rois_override=ov)
    for n, (cells, rcells) in enumerate(zip(mo, ref["maps"])):
        t, mx = ref["t"][n // 2], ref["m"][n // 2]
        th = mx * (0.7 if n % 2 == 0 else 0.1)
        diff = cells != rcells
        print(n, int(cells.sum()), int(rcells.sum()), int(diff.sum()))
        assert int(cells.sum()) >= 4 and int(rcells.sum()) >= 4
        assert int(diff.sum()) <= 0.01 * diff.numel(), (n, int(diff.sum()))
        assert ((t - th).abs()[diff] <= 1e-5 * mx).all(), n


def test_pt_maf_fused_matches_unfused(monkeypatch):
    """TLOD_FUSED_LOSSES=0 (the torch compositions) in the same process: the same losses."""
    m, teacher = _device_models(0)
    gpu_batch = tuple(t.to(dev) for t in _batch(192, 320, 1))
    with torch.no_grad():
        out, kd, _ = _device_step(m, teacher, gpu_batch, backward=False)
        monkeypatch.setenv("TLOD_FUSED_LOSSES", "0")
        out0, kd0, _ = _device_step(m, teacher, gpu_batch, backward=False)
    assert torch.equal(out[0], out0[0])
    for i in IDX:
        close(out[i], out0[i])
    close(kd, kd0)


def test_pt_maf_two_pass_path_matches_oracle():
    """Differently sized source / target images (192x320, 192x336) take the two-pass path
    (one backbone / head pass per image, RCNN_imageDA_3_b skipped on the source).  The oracle
    is per-image by construction, and the batched path is held to it above, so the two paths
    agree when this one meets the same 1e-4."""
    m, teacher = _device_models(5)
    o, ot = _oracles(m, teacher)
    cpu_batch = _batch(192, 320, 6, tgt_W=336)
    assert cpu_batch[0].shape != cpu_batch[5].shape
    with torch.no_grad():
        out, kd, _ = _device_step(m, teacher, tuple(t.to(dev) for t in cpu_batch), backward=False)
        ov, mo = _overrides(m)
        assert mo[0].shape == (1, 12, 20) and mo[2].shape == (1, 12, 21)
        ref = o(cpu_batch, np.random.RandomState(3), rois_override=ov, maps_override=mo)
        ref_kd = o.kd(ref, teacher_outputs(ot, cpu_batch, out[0].cpu().numpy()))
    _assert_losses(out, kd, ref, ref_kd)


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_pt_maf_train_step(optimizer):
    from tlod.detector.train import SyntheticCityscapes, make_optimizer, pt_maf_train_step
    m, teacher = _device_models(0)
    opt = make_optimizer(m, 1e-3, optimizer=optimizer)
    data = SyntheticCityscapes(dev, H=192, W=320, G=4, pool=1, seed=7)
    before = {k: v.detach().clone() for k, v in m.named_parameters() if v.requires_grad}
    t_before = {k: v.detach().clone() for k, v in teacher.state_dict().items()}
    loss = pt_maf_train_step(m, teacher, opt, data.next())
    assert torch.isfinite(loss)
    changed = [k for k, v in m.named_parameters() if v.requires_grad
               and not torch.equal(v.detach(), before[k])]
    assert len(changed) > 0.9 * len(before), (len(changed), len(before))
    for k, v in teacher.state_dict().items():
        assert torch.equal(v, t_before[k]), k
    assert all(p.grad is None for p in teacher.parameters())


def test_pt_maf_eval_path():
    """im_detect on a PT-MAF model: the 4-argument eval-mode forward, per-class arrays."""
    from tlod.eval.detect import im_detect
    m, _ = _device_models(0)
    b = tuple(t.to(dev) for t in _batch(192, 320, 1))
    per_class = im_detect(m, b[0], b[1], b[2], b[3])
    assert len(per_class) == m.n_classes and m.training
    assert all(d.ndim == 2 and d.shape[1] == 5 for d in per_class)
    assert sum(len(d) for d in per_class[1:]) > 0
