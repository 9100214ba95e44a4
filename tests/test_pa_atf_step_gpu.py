"""PA-ATF (tlod.da.pa_atf) on the device: the 13-output step against the CPU restatement
(tests/ref_pa_atf.py) with replayed draws, the fused ops against their torch compositions in
the same process (TLOD_FUSED_PA_ATF=0, TLOD_SCONV=0), one train_step at 600 x 1200, and the
eval path.

Image sizes: each side is at least 320, so the conv5 map has at least 20 cells per side and
Convm2 still sees a 3 x 3 input.  The target's NMS survivors must outnumber the 256 RoIs so
that the random part of the subsample is exercised: asserted, not assumed.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"

LOSSES = ["rpn_loss_cls", "rpn_loss_box", "RCNN_loss_cls", "RCNN_loss_bbox", "DA_img_loss_cls",
          "tgt_DA_img_loss_cls", "DA_ins_loss_cls", "tgt_DA_ins_loss_cls", "pm_loss"]
IDX = [3, 4, 5, 6, 8, 9, 10, 11, 12]
POST = 256
NRM, ELT = 1e-5, 1e-4  # tests/test_linear_gpu.py BARS["bf16x6"], the bars of the strided conv


def _model(seed):
    from tlod.detector.train import build_model
    m = build_model("pa_atf", dev, seed=seed)
    g = torch.Generator(device=dev).manual_seed(seed + 100)
    with torch.no_grad():  # make the two branches differ (tests/test_atf_step_gpu.py)
        for p in m.RCNN_base_t[m.splits[0]:].parameters():
            if p.requires_grad:
                p.mul_(1.0 + 0.05 * torch.randn(p.shape, generator=g, device=dev))
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m


def _batch(H, W, seed):
    from oracle.daf_step import synthetic_batch
    return synthetic_batch(H, W, seed=seed)


def _arm(m):
    """tests/helpers.arm_taps (backbones, RPN, fc6 / fc7, the three Conv1 ReLUs, ip1 / ip2) plus
    PA-ATF's own sites: the six mask-net ReLUs (Convm1, source and target) with the 2x2 max-pool
    that follows them (its argument is taken from the same activation, as the backbone's pool
    sites are), and CLUB's two ReLUs per level (rows: same, then diff)."""
    from helpers import arm_taps
    taps = arm_taps(m)
    for lvl, h, c in ((3, m.RCNN_imageDA_3, m.club3), (4, m.RCNN_imageDA_4, m.club4),
                      (5, m.RCNN_imageDA, m.club5)):
        h.Convm1.act_tap = []
        taps[f"m1_{lvl}"] = (h.Convm1.act_tap, "map")
        taps[f"mp{lvl}"] = (h.Convm1.act_tap, "pool")
        for tag, conv in (("a", c.out_score[0]), ("b", c.out_score[2])):
            conv.act_tap = []
            taps[f"club{lvl}{tag}"] = (conv.act_tap, "club")
    return taps


def _step(m, gpu_batch, backward=True, force_args=None):
    m.replay_rng = np.random.RandomState(3)
    m.capture = {}
    m.force_args = force_args
    m.zero_grad(set_to_none=True)
    out = m(*gpu_batch)
    assert len(out) == 13
    loss = m.total_loss(out)
    if backward:
        loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    return out, loss.detach(), grads, dict(m.capture)


def test_pa_atf_losses_match_the_restatement():
    """320 x 352, model seed 0, batch seed 1: every scalar term and the total within 1e-4 of
    tests/ref_pa_atf.py run on the device's proposals, kept / picked target RoIs, gate
    arguments and prototype-pooling argmax; the sampled RoIs and labels identical; every
    trainable parameter has a gradient, under tests/helpers.pattern_grad_bar (the fp64
    restatement in the device's activation pattern; bar: twice the fp32 restatements' own
    error, floor 2e-5 normwise)."""
    from helpers import pattern_grad_bar, record_pattern
    from ref_pa_atf import OraclePAATF, total_loss
    from tlod.config import cfg
    m = _model(0)
    taps = _arm(m)
    cpu_batch = _batch(320, 352, 1)
    out, loss, grads, cap = _step(m, tuple(t.to(dev) for t in cpu_batch))
    assert cfg.TEST.RPN_POST_NMS_TOP_N == 300        # the global cfg is left alone
    count = int(cap["t_count"][0])
    print("target NMS survivors:", count)
    assert count > 256
    o = OraclePAATF(dropout=0.0).train()
    o.load_from(m)
    ov = tuple(cap[k].cpu().numpy() for k in ("s_rois", "st_rois", "t_kept", "t_rois"))
    args = [a.cpu() for a in cap["args"]]
    pp = [a.cpu().numpy() for a in cap["pp_argmax"]]
    assert all(tuple(a.shape) == (2, c) for a, c in zip(args, (256, 512, 512))) and len(pp) == 3

    def run(mod, b, own_keep=False):
        box["ref"] = mod(b, np.random.RandomState(3), rois_override=ov, arg_override=args,
                         count=count, pp_override=pp, own_keep=own_keep)
        return total_loss(box["ref"])
    box = {}
    own = record_pattern(o, lambda: run(o, cpu_batch).backward())
    ref = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in box["ref"].items()}
    for name, i in zip(LOSSES, IDX):
        g, r = float(out[i].detach()), float(ref[name])
        print(f"{name}: device {g:.7f} restatement {r:.7f}")
        assert abs(g - r) <= 1e-4 * max(abs(r), 1e-3), (name, g, r)
    g, r = float(loss), float(total_loss(ref))
    assert abs(g - r) <= 1e-4 * abs(r), (g, r)
    np.testing.assert_array_equal(out[0].cpu().numpy().reshape(-1, 5), ref["rois"].reshape(-1, 5))
    np.testing.assert_array_equal(out[7].cpu().numpy(), ref["rois_label"])
    np.testing.assert_array_equal(cap["t_rois"].cpu().numpy(), ref["t_rois"])   # the replayed pick
    for k, p in m.named_parameters():
        if p.requires_grad:
            assert k in grads and torch.isfinite(grads[k]).all(), k
    assert len(grads) == sum(p.requires_grad for p in m.parameters())
    gp = dict(m.named_parameters())
    for k, p in o.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and gp[k].grad is not None, k
    G = int(cpu_batch[3].view(-1)[0])
    nb = out[7].numel()
    rows = {"head": [nb, nb, POST], "ins": [nb, POST], "club": [G, G]}
    pattern_grad_bar(m, o, run, cpu_batch, taps, rows, own)


def test_pa_atf_proposals_without_override():
    """336 x 400, model seed 2, batch seed 3, losses only: the s-branch and t-branch proposals
    and the target's NMS survivors come from each side's own RPN outputs and are compared as
    sets (tests/helpers.assert_proposal_sets_match); the terms that do not depend on the sampled
    RoIs — the RPN losses, the six gated image terms, pm_loss — within 1e-4."""
    from helpers import assert_proposal_sets_match
    from ref_pa_atf import OraclePAATF
    m = _model(2)
    cpu_batch = _batch(336, 400, 3)
    with torch.no_grad():
        out, _, _, cap = _step(m, tuple(t.to(dev) for t in cpu_batch), backward=False)
        count = int(cap["t_count"][0])
        print("target NMS survivors:", count)
        assert count > 256
        o = OraclePAATF(dropout=0.0).train()
        o.load_from(m)
        ov = (None, None, cap["t_kept"].cpu().numpy(), cap["t_rois"].cpu().numpy())
        ref = o(cpu_batch, np.random.RandomState(3), rois_override=ov,
                arg_override=[a.cpu() for a in cap["args"]], count=count,
                pp_override=[a.cpu().numpy() for a in cap["pp_argmax"]])
    for key, ref_key in (("s_rois", "props_s"), ("st_rois", "props_st")):
        assert_proposal_sets_match(cap[key].cpu().numpy(), ref[ref_key], key)
    pad = lambda b: np.concatenate([np.zeros((len(b), 1), np.float32), b], 1)
    assert_proposal_sets_match(pad(cap["t_kept"][0, :count].cpu().numpy()), pad(ref["t_kept"]),
                               "t_kept")
    for name in ("rpn_loss_cls", "rpn_loss_box", "DA_img_loss_cls", "tgt_DA_img_loss_cls",
                 "pm_loss"):
        g, r = float(out[IDX[LOSSES.index(name)]]), float(ref[name])
        print(f"{name}: device {g:.7f} restatement {r:.7f}")
        assert abs(g - r) <= 1e-4 * max(abs(r), 1e-3), (name, g, r)


@pytest.mark.parametrize("switch", ["TLOD_FUSED_PA_ATF", "TLOD_SCONV"])
def test_pa_atf_fused_matches_unfused(switch, monkeypatch):
    """The same step with the switch off, in the same process, with the same replayed draws and
    with the first run's gate arguments forced on the second (a near-tie between two cells of
    a mask-net plane would otherwise reroute that channel's gradient; the restatement's
    arg_override rule), so the gradients are always compared.  Losses within 1e-5.  Every
    parameter's gradient under the bf16x6 bars of tests/test_linear_gpu.py that the strided
    convolution's own tests use: 1e-5 normwise, 1e-4 elementwise against the largest entry."""
    m = _model(2)
    gpu_batch = tuple(t.to(dev) for t in _batch(336, 400, 3))
    out, loss, grads, cap = _step(m, gpu_batch)
    monkeypatch.setenv(switch, "0")
    out0, loss0, grads0, cap0 = _step(m, gpu_batch, force_args=cap["args"])
    assert int(cap["t_count"][0]) > 256
    # nothing in front of the proposal layers depends on the switch
    assert all(torch.equal(cap[k], cap0[k]) for k in ("s_rois", "st_rois", "t_rois"))
    assert all(torch.equal(a, b) for a, b in zip(cap["args"], cap0["args"]))
    for i in IDX:
        a, b = float(out[i].detach()), float(out0[i].detach())
        assert abs(a - b) <= 1e-5 * max(abs(b), 1e-3), (i, a, b)
    assert abs(float(loss - loss0)) <= 1e-5 * abs(float(loss0))
    assert set(grads) == set(grads0)
    worst_n, worst_e = (0.0, ""), (0.0, "")
    for k in grads:
        d, r = (grads[k] - grads0[k]).double(), grads0[k].double()
        worst_n = max(worst_n, (float(d.norm() / r.norm().clamp(min=1e-30)), k))
        worst_e = max(worst_e, (float(d.abs().max() / r.abs().max().clamp(min=1e-30)), k))
    print("worst parameter gradient: normwise", worst_n, "elementwise", worst_e)
    assert worst_n[0] <= NRM, worst_n
    assert worst_e[0] <= ELT, worst_e


def test_pa_atf_train_step_at_600x1200_runs_finite():
    from tlod.detector.train import (SyntheticCityscapes, build_model, default_clip,
                                     make_optimizer, train_step)
    m = build_model("pa_atf", dev)
    assert default_clip(m) == 10.0
    opt = make_optimizer(m, 1e-3)
    data = SyntheticCityscapes(dev, pool=1, seed=7)
    before = {k: v.detach().clone() for k, v in m.named_parameters() if v.requires_grad}
    loss = train_step(m, opt, data.next())
    assert torch.isfinite(loss)
    changed = [k for k, v in m.named_parameters() if v.requires_grad
               and not torch.equal(v.detach(), before[k])]
    # (a saturated instance discriminator — random init at this size — leaves its last bias,
    # which has no weight decay, where it was: the rule of tests/test_idf_step_gpu.py)
    assert len(changed) > 0.9 * len(before), sorted(set(before) - set(changed))
    for k in changed:
        assert torch.isfinite(dict(m.named_parameters())[k]).all(), k
    assert torch.isfinite(train_step(m, opt, data.next()))


def test_pa_atf_eval_path():
    """im_detect on a PA-ATF model: the 4-argument eval-mode forward of the s branch."""
    from tlod.eval.detect import im_detect
    m = _model(0)
    b = tuple(t.to(dev) for t in _batch(320, 352, 1))
    per_class = im_detect(m, b[0], b[1], b[2], b[3])
    assert len(per_class) == m.n_classes and m.training
    assert all(d.ndim == 2 and d.shape[1] == 5 for d in per_class)
    assert sum(len(d) for d in per_class[1:]) > 0
