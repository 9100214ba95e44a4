"""IDF (tlod.da.idf) on the device against the CPU restatement (tests/ref_idf.py): the full
source + target step with the same weights, dropout 0, replayed draws, the device's proposals
(rois_override) and the device's attention maps (att_override).

Bars: every loss term within 1e-4 relative; sampled RoIs identical; gradients under
tests/helpers.pattern_grad_bar; the device's own attention maps against the oracle's own: at
most 1 % of a map's cells differ, each with its avg within 1e-5 thr of the threshold.

Inputs: 192x320 with seed 0 and 224x352 with seed 2; the target's pseudo boxes are the
source-style boxes of a second synthetic batch.  With this project's init the CPU oracle alone
puts 47-58 % of the cells on and at most 4 cells of a map (0.3 %) inside the 1e-5 thr band
(smallest gap 4e-7 thr), so the 1 % cap leaves room for the device's own rounding."""
import types

import numpy as np
import pytest
import torch

from helpers import arm_taps, pattern_grad_bar, record_pattern
from ref_idf import DET, DOM, OracleIDF, total_loss

pytestmark = pytest.mark.gpu
dev = "cuda"

DISCS = ("netD_1", "netD_2", "netD_3", "netD_1_b", "netD_2_b", "netD_3_b")
N_ROWS = {"head": [256, 256], "head_t": [256], "ins": [256] * 4}
ZERO_GRAD = ("netD_da.fc1.bias", "netD_da.fc2.bias")


def _device_model(seed):
    from tlod.detector.train import build_model
    m = build_model("idf", dev, seed=seed)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if hasattr(mod, "drop_p"):
            mod.drop_p = 0.0
    return m


def _oracle(m):
    """The restatement with the device model's weights.  netD_da's fc1 / fc2 biases sit in
    front of a training-mode batch norm, whose mean subtraction makes their gradient exactly
    zero: what any fp32 run leaves there is rounding noise, and a relative error of noise
    against noise judges nothing, so the gradient bar leaves them out (the step test bounds
    them against their weights' gradients instead)."""
    o = OracleIDF(dropout=0.0).train()
    o.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
    for k in ZERO_GRAD:
        dict(o.named_parameters())[k].requires_grad_(False)
    return o


def _batch(H, W, seed):
    from oracle.daf_step import synthetic_batch
    b, p = synthetic_batch(H, W, seed=seed), synthetic_batch(H, W, seed=seed + 50)
    return b[:7] + (p[2], p[3], b[9])


def _arm(m):
    """helpers.arm_taps reads RCNN_base / RCNN_base_t / RCNN_top / RCNN_rpn: hand it a view of
    the two stacks under those names, then add the _t detector's sites and one site per
    discriminator (ref_idf's names)."""
    view = types.SimpleNamespace(
        RCNN_base=torch.nn.Sequential(*m.RCNN_base1, *m.RCNN_base2, *m.RCNN_base3),
        RCNN_base_t=torch.nn.Sequential(*m.RCNN_base1_b, *m.RCNN_base2_b, *m.RCNN_base3_b),
        RCNN_top=m.RCNN_top, RCNN_rpn=m.RCNN_rpn)
    taps = arm_taps(view)

    def add(site, mod, kind):
        mod.act_tap = []
        taps[site] = (mod.act_tap, kind)
    add("rpn_t", m.RCNN_rpn_t.RPN_Conv, "map")
    add("fc6_t", m.RCNN_top_t[0], "head_t")
    add("fc7_t", m.RCNN_top_t[3], "head_t")
    for name in DISCS:
        add(name, getattr(m, name), "map")
    add("netD_da", m.netD_da, "ins")
    return taps


def _device_step(m, gpu_batch, separation=True, backward=True):
    from tlod.detector.train import idf_forward
    m.replay_rng = np.random.RandomState(3)
    m.capture = {}
    out_s, out_t = idf_forward(m, gpu_batch, separation)
    assert len(out_s) == 20 and len(out_t) == 20
    loss = m.total_loss(out_s, out_t, separation, 3.0)
    if backward:
        loss.backward()
    return out_s, out_t, loss


def _overrides(m):
    c = m.capture
    rois = tuple(c[k].cpu().numpy() for k in ("s_rois", "t_rois", "t_rois_b"))
    return rois, tuple(a.cpu() for a in c["s_att"] + c["t_att"])


def _close(name, got, ref):
    g, r = float(got.detach()), float(ref.detach())
    print(name, g, r)
    assert abs(g - r) <= 1e-4 * max(abs(r), 1e-3), (name, g, r)


def _assert_terms(m, outs, refs):
    for tag, out, ref, label in (("s", outs[0], refs[0], 0), ("t", outs[1], refs[1], 1)):
        for i, k in enumerate(DET):
            _close(f"{tag}.{k}", out[3 + i], ref[k])
        dom = m.domain_terms(out, label, 3.0)
        for i, k in enumerate(DOM + ("ins",)):
            _close(f"{tag}.{k}", dom[i], ref["dom"][i])
        for i, k in ((15, "loss_se_2"), (16, "loss_se_3"), (17, "dist1"), (18, "dist2"),
                     (19, "dist3")):
            _close(f"{tag}.{k}", out[i], ref[k])
        for i, k in zip((8, 9, 10, 12, 13, 14), DOM):
            assert out[i].shape == (1, 2) and ref[k].shape == (1, 2)
        assert out[11].shape == (256, 2)


@pytest.mark.parametrize("H,W,seed", [(192, 320, 0), (224, 352, 2)])
def test_idf_losses_and_grads_match_oracle(H, W, seed):
    m = _device_model(seed)
    o = _oracle(m)
    cpu_batch = _batch(H, W, seed + 1)
    gpu_batch = tuple(t.to(dev) for t in cpu_batch)
    taps = _arm(m)
    out_s, out_t, loss = _device_step(m, gpu_batch)
    ro, ao = _overrides(m)
    box = {}

    def step(mod, b):
        box["ref"] = mod(b, np.random.RandomState(3), rois_override=ro, att_override=ao)
        return total_loss(*box["ref"])

    own = record_pattern(o, lambda: step(o, cpu_batch).backward())
    s, t = box["ref"]
    _assert_terms(m, (out_s, out_t), (s, t))
    _close("total", loss, total_loss(s, t))
    np.testing.assert_array_equal(out_s[0].cpu().numpy().reshape(-1, 5), s["rois"].reshape(-1, 5))
    np.testing.assert_array_equal(out_t[0].cpu().numpy().reshape(-1, 5), t["rois"].reshape(-1, 5))
    np.testing.assert_array_equal(out_s[7].cpu().numpy(), s["rois_label"].numpy())
    np.testing.assert_array_equal(out_t[7].cpu().numpy(), t["rois_label"].numpy())
    assert int((out_t[7] > 0).sum()) > 0  # the pseudo boxes do train the branch's head
    named = dict(m.named_parameters())
    for k, p in named.items():
        assert (p.grad is not None) == p.requires_grad, k
    for k in ZERO_GRAD:  # exactly zero behind the batch norm: noise, far below the weights'
        w = named[k.replace("bias", "weight")].grad
        assert float(named[k].grad.norm()) <= 1e-4 * float(w.norm()), k
    pattern_grad_bar(m, o, step, cpu_batch, taps, N_ROWS, own)


@pytest.mark.parametrize("H,W,seed", [(192, 320, 0), (224, 352, 2)])
def test_idf_own_attention_maps(H, W, seed):
    """The device's att maps against the oracle's own (fp64, from its own features): at most
    1 % of a map's cells differ, each within 1e-5 thr of the threshold.  The oracle's own maps
    are what dam gives on ITS features; its modulation uses the device's maps, so a level-2
    cell inside the band that lands on the other side is judged once, at level 2, and does not
    also move the conv5 features the level-3 maps are computed from."""
    m = _device_model(seed)
    o = _oracle(m).double()
    cpu_batch = _batch(H, W, seed + 1)
    with torch.no_grad():
        _device_step(m, tuple(t.to(dev) for t in cpu_batch), backward=False)
        ro, ao = _overrides(m)
        b64 = tuple(t.double() if t.is_floating_point() else t for t in cpu_batch)
        s, t = o(b64, np.random.RandomState(3), rois_override=ro, att_override=ao)
    own = s["att"] + t["att"]
    parts = s["att_parts"] + t["att_parts"]
    assert len(ao) == 8
    for n, (got, ref, (avg, thr)) in enumerate(zip(ao, own, parts)):
        diff = (got > 0) != (ref > 0)
        on = float((ref > 0).double().mean())
        print(n, diff.numel(), "on", round(on, 3), "differ", int(diff.sum()))
        assert 0.3 < on < 0.7
        assert int(diff.sum()) <= 0.01 * diff.numel(), (n, int(diff.sum()))
        assert (((avg - thr).abs() <= 1e-5 * thr)[:, 0][diff]).all(), n


def test_idf_separation_switch():
    """separation=False: the same outputs, and a total without the four loss_se terms."""
    m = _device_model(0)
    gpu_batch = tuple(t.to(dev) for t in _batch(192, 320, 1))
    with torch.no_grad():
        out_s, out_t, with_se = _device_step(m, gpu_batch, True, backward=False)
        out_s0, out_t0, without = _device_step(m, gpu_batch, False, backward=False)
    se = out_s[15] + out_s[16] + out_t[15] + out_t[16]
    assert float(se) > 0
    assert torch.equal(out_s[0], out_s0[0]) and torch.equal(out_t[0], out_t0[0])
    for a, b in zip(out_s[3:7] + out_s[15:20] + out_t[3:7] + out_t[15:20],
                    out_s0[3:7] + out_s0[15:20] + out_t0[3:7] + out_t0[15:20]):
        assert abs(float(a - b)) <= 1e-6 * abs(float(b))
    assert abs(float(with_se - without) - float(se)) <= 1e-5 * abs(float(with_se))


def test_idf_fused_matches_unfused(monkeypatch):
    """TLOD_FUSED_IDF=0 (the torch compositions) in the same process.  What lies in front of
    the first attention map (dist1, the level-1 and level-2 discriminators) agrees within the
    kernels' bars in any case; the two paths' att maps follow the 1 % rule; and where no cell
    of any map landed on the other side, so do the terms behind them that do not depend on
    the sampled RoIs (1e-4, the step's bar).
    A cell that did land on the other side changes its pixel by a third: the terms behind it
    are then not comparable, and the run says so."""
    m = _device_model(0)
    gpu_batch = tuple(t.to(dev) for t in _batch(192, 320, 1))
    with torch.no_grad():
        out_s, out_t, loss = _device_step(m, gpu_batch, backward=False)
        att = m.capture["s_att"] + m.capture["t_att"]
        dom = [m.domain_terms(o, l) for o, l in ((out_s, 0), (out_t, 1))]
        monkeypatch.setenv("TLOD_FUSED_IDF", "0")
        out_s0, out_t0, loss0 = _device_step(m, gpu_batch, backward=False)
        att0 = m.capture["s_att"] + m.capture["t_att"]
        dom0 = [m.domain_terms(o, l) for o, l in ((out_s0, 0), (out_t0, 1))]
    flips = [int(((a > 0) != (a0 > 0)).sum()) for a, a0 in zip(att, att0)]
    print("cells on the other side per map:", flips)
    for a, n in zip(att, flips):
        assert n <= 0.01 * a.numel()
    for o, o0, d, d0 in ((out_s, out_s0, dom[0], dom0[0]), (out_t, out_t0, dom[1], dom0[1])):
        assert abs(float(o[17] - o0[17])) <= 2e-6 * abs(float(o0[17]))
        for i in (0, 1, 3, 4):  # d1, d2, d1_b, d2_b
            assert abs(float(d[i] - d0[i])) <= 2e-5 * max(abs(float(d0[i])), 1e-3), i
    if not any(flips):
        # the RCNN losses and the instance term are left out: the two paths' maps differ in
        # ulps, which can reorder near-tied proposal scores and change the sampled RoI set
        for o, o0, d, d0 in ((out_s, out_s0, dom[0], dom0[0]), (out_t, out_t0, dom[1], dom0[1])):
            for i in (3, 4, 15, 16, 18, 19):
                assert abs(float(o[i] - o0[i])) <= 1e-4 * max(abs(float(o0[i])), 1e-3), i
            assert float((d[:6] - d0[:6]).abs().max()) <= 1e-4 * max(float(d0[:6].abs().max()), 1e-3)


def test_idf_train_step_at_600x1200_runs_finite():
    from tlod.detector.train import (SyntheticCityscapes, build_model, idf_train_step,
                                     make_optimizer)
    m = build_model("idf", dev)
    opt = make_optimizer(m, 1e-3)
    data = SyntheticCityscapes(dev, pool=1, seed=7, tgt_G=6)
    before = {k: v.detach().clone() for k, v in m.named_parameters() if v.requires_grad}
    dead = {k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith("fuse_3.")}
    loss = idf_train_step(m, opt, data.next())
    assert torch.isfinite(loss)
    changed = [k for k, v in m.named_parameters() if v.requires_grad
               and not torch.equal(v.detach(), before[k])]
    assert len(changed) > 0.9 * len(before), (len(changed), len(before))
    for k, v in m.state_dict().items():
        if k in dead:
            assert torch.equal(v, dead[k]), k
    loss = idf_train_step(m, opt, data.next(), separation=False)
    assert torch.isfinite(loss)


def test_idf_eval_path():
    """im_detect on an IDF model: the 4-argument eval-mode forward of the main stack."""
    from tlod.eval.detect import im_detect
    m = _device_model(0)
    b = tuple(t.to(dev) for t in _batch(192, 320, 1))
    per_class = im_detect(m, b[0], b[1], b[2], b[3])
    assert len(per_class) == m.n_classes and m.training
    assert all(d.ndim == 2 and d.shape[1] == 5 for d in per_class)
    assert sum(len(d) for d in per_class[1:]) > 0
