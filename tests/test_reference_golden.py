"""tests/golden/reference_v1.npz: outputs of the reference's own Python layers, recorded by
tests/golden/make_reference_golden.py (which runs the reference on the CPU; see its docstring
for the run-time stand-ins).  Everything else in the suite is measured against oracle/ and
tests/ref_*.py, this project's restatements; these tests pin the restatements, and the HIP
layers behind them, to what the reference itself computed.

CPU: the oracle (oracle/rpn.py, oracle/boxes.py), tlod.rpn.proposal.subsample_rule, the torch
composition of smooth-L1 and tests/ref_roi_crop.py's theta / grid reproduce the fixture with the
recorded draws replayed; and, when the reference checkout is given in TLOD_REFERENCE_DIR, the
generator reproduces the committed file bit for bit (so it is neither hand-edited nor made from
the oracle).  GPU: the same fixture through the HIP layers.  The GPU tests read the .npz only.

Not pinned: NMS.  The reference's NMS is a CUDA extension, so the generator ran the proposal
layers with oracle.nms.nms in its place: the proposal cases pin decode, clip, sort, the
``pre_nms_topN < numel over the whole batch`` rule, the post-NMS / PA-ATF subsample rule,
padding and the batch column, on whatever the restated NMS kept.

Cases.  Anchor target (A = 12, stride 16; 12 x 15 unless noted): a no gt box; b B = 2, two
identical gts (argmax ties) and an empty image; c a gt covering the image, a one-pixel gt, an
inverted gt; d 40 large gts in 50 rows at 18 x 24 (145 fg and 833 bg candidates: both
permutations drawn); e B = 2, im_info[1] smaller than im_info[0]; f 20 x 30, B = 2, G = 3.
Proposal target (256 RoIs): a fg only; b no gt, bg only; c 305 fg + 100 bg candidates (c128:
the same with cfgs/res101.yml's 128); d B = 2, an ordinary and a bg-only image; e RoIs ending
in zero rows.  Proposal layer (B, H, W, pre, post, delta scale): (1, 10, 12, 1000, 200, 0),
(2, 6, 7, 700, 100, 0.3), (1, 6, 7, 300, 100, 3.0), (2, 10, 12, 1000, 300, 0.2).  PA-ATF's
proposal_layer1 with key 'TEST': survivors <= int(post * 0.25), between that and post, more
than post.  Box primitives on 50 boxes x 5 gts with zero-area boxes and gts; _smooth_l1_loss
in float64 (sigma 3 over [1, 2, 3], sigma 1 over [1], with differences at +-1 / sigma^2);
_affine_theta / _affine_grid_gen (3 RoIs, 37 x 62, grids 7 and 14); clip_gradient above and
below the norm of 10; MAF's DRM forward and US-DAF's _ImageDA forward / backward in float64.

Bars are the families' existing ones: labels, weights, sampled RoIs, counts and picks exact;
regression targets rtol 2e-6 / atol 2e-6 and decoded boxes rtol 2e-6 / atol 1e-4
(tests/test_rpn_gpu.py), delta-scale-0 proposals exact; losses and gradients ``close`` of
tests/test_losses_gpu.py; the clipped update rtol 1e-5 / atol 1e-6 (tests/test_optim_gpu.py);
conv outputs ``_close`` of tests/test_conv_gpu.py.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_roi_crop
from oracle import boxes as obox
from oracle import nms as onms
from oracle import rpn as orpn
from test_conv_gpu import _close as conv_close
from test_losses_gpu import close

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "reference_v1.npz"))
ENV = "TLOD_REFERENCE_DIR"
STRIDE = 16
AT_CASES = ["a", "b", "c", "d", "e", "f"]
PT_CASES = ["a", "b", "c", "c128", "d", "e"]
PL_CASES = [0, 1, 2, 3]
PA_CASES = [0, 1, 2]
TGT = dict(rtol=2e-6, atol=2e-6)
BOX = dict(rtol=2e-6, atol=1e-4)
dev = "cuda"


class Replay:
    """Replays a case's recorded draws (kind 0 permutation, 1 rand, 2 sample) in order."""

    def __init__(self, prefix):
        self.kinds, self.lens = G[prefix + "_draw_kinds"], G[prefix + "_draw_lens"]
        self.flat = G[prefix + "_draws"]
        self.i, self.off = 0, 0

    def _next(self, kind, n=None):
        assert self.i < len(self.kinds), "more draws than the reference made"
        assert self.kinds[self.i] == kind and (n is None or self.lens[self.i] == n), \
            (self.i, int(self.kinds[self.i]), kind, int(self.lens[self.i]), n)
        v = self.flat[self.off:self.off + self.lens[self.i]]
        self.off += self.lens[self.i]
        self.i += 1
        return v

    def permutation(self, n):
        return self._next(0, n).astype(np.int64)

    def rand(self, n):
        return self._next(1, n)

    def picks(self):
        return self._next(2).astype(np.int64)

    def done(self):
        return self.i == len(self.kinds)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def check_targets(prefix, names, got, exact):
    for k, v in zip(names, got):
        v = v.detach().cpu().numpy() if torch.is_tensor(v) else v
        if k == "targets" and not exact:
            np.testing.assert_allclose(v, G[f"{prefix}_{k}"], err_msg=f"{prefix}_{k}", **TGT)
        else:
            np.testing.assert_array_equal(v, G[f"{prefix}_{k}"], err_msg=f"{prefix}_{k}")


AT_NAMES = ("labels", "targets", "inside", "outside")
PT_NAMES = ("rois", "labels", "targets", "inside", "outside")


# ============================================================================ CPU: the oracle
def test_anchor_table():
    base = obox.generate_anchors(scales=np.array([4, 8, 16, 32]), ratios=np.array([0.5, 1, 2]))
    np.testing.assert_array_equal(base, G["anchors_base"])


@pytest.mark.parametrize("case", AT_CASES)
def test_oracle_anchor_target(case):
    p = "at_" + case
    H, W = (int(v) for v in G[p + "_hw"])
    rp = Replay(p)
    got = orpn.anchor_target(H, W, G[p + "_gt"], G[p + "_info"], G["anchors_base"], STRIDE, rp)
    assert rp.done()
    check_targets(p, AT_NAMES, got, exact=False)


def rcnn_cfg_of(p):
    batch, bg_lo, fg_frac, fg_thresh, bg_hi = G[p + "_cfg"]
    return dict(orpn.DEFAULT_RCNN, batch=int(batch), bg_lo=bg_lo, fg_frac=fg_frac,
                fg_thresh=fg_thresh, bg_hi=bg_hi)


@pytest.mark.parametrize("case", PT_CASES)
def test_oracle_proposal_target(case):
    p = "pt_" + case
    rp = Replay(p)
    got = orpn.proposal_target(G[p + "_rois_in"], G[p + "_gt"], rp, rcnn_cfg_of(p))
    assert rp.done()
    check_targets(p, PT_NAMES, got, exact=False)


def check_rois(p, got):
    """Delta scale 0 decodes exactly (exp(0) = 1): bit-exact; otherwise the decode bar."""
    want = G[p + "_rois"]
    if not G[p + "_deltas"].any():
        np.testing.assert_array_equal(got, want, err_msg=p)
    else:
        np.testing.assert_allclose(got, want, err_msg=p, **BOX)
    np.testing.assert_array_equal(got[:, :, 0], want[:, :, 0])        # the batch column
    pad = ~want[:, :, 1:].any(2)
    assert not got[pad][:, 1:].any()                                   # zero padding, exactly


@pytest.mark.parametrize("case", PL_CASES)
def test_oracle_proposal_layer(case):
    p = f"pl_{case}"
    pre, post, thr = G[p + "_cfg"]
    got = orpn.proposal_layer(G[p + "_prob"], G[p + "_deltas"], G[p + "_info"], G["anchors_base"],
                              STRIDE, int(pre), int(post), thr)
    check_rois(p, got)


@pytest.mark.parametrize("case", PA_CASES)
def test_subsample_rule_reproduces_pa_atf(case):
    """PA-ATF's proposal_layer1 ('TEST'): the oracle's decode / sort / NMS, then
    tlod.rpn.proposal.subsample_rule with the recorded random.sample picks."""
    from tlod.rpn.proposal import subsample_head, subsample_rule
    p = f"pa_{case}"
    pre, post, thr = G[p + "_cfg"]
    pre, post = int(pre), int(post)
    prob, deltas, info = G[p + "_prob"], G[p + "_deltas"], G[p + "_info"]
    scores, props = orpn.decode_clip(prob, deltas, info, G["anchors_base"], STRIDE)
    rp = Replay(p)
    B = prob.shape[0]
    got = np.zeros((B, post, 5), np.float32)
    for b in range(B):
        order = np.argsort(-scores[b], kind="stable")
        if 0 < pre < scores.size:
            order = order[:pre]
        box = props[b][order]
        keep = list(onms.nms(np.concatenate([box, scores[b][order, None]], 1), thr))
        assert len(keep) == G[p + "_survivors"][b]
        picks = rp.picks()
        rows, idx = subsample_rule(keep, post, lambda n: picks)
        assert idx == [int(i) for i in picks]                      # every recorded pick is used
        assert rows[:subsample_head(post)] == keep[:subsample_head(post)]
        got[b, :, 0] = b
        got[b, :len(rows), 1:] = box[rows]
    assert rp.done()
    check_rois(p, got)


def test_oracle_box_primitives():
    anchors, gt, rois = G["box_anchors"], G["box_gt"], G["box_rois"]
    B = gt.shape[0]
    for b in range(B):
        np.testing.assert_array_equal(obox.bbox_overlaps(anchors, gt[b]), G["box_ov2"][b])
        np.testing.assert_array_equal(obox.bbox_overlaps(rois[b, :, 1:5], gt[b]), G["box_ov3"][b])
        np.testing.assert_allclose(obox.bbox_transform(anchors, G["box_gt_rois"][b]),
                                   G["box_tf2"][b], **TGT)
        np.testing.assert_allclose(obox.bbox_transform(rois[b, :, 1:5], G["box_gt_rois"][b]),
                                   G["box_tf3"][b], **TGT)
        inv = obox.bbox_transform_inv(G["box_boxes"][b], G["box_deltas"][b])
        np.testing.assert_allclose(inv, G["box_inv"][b], **BOX)
        info = G["box_info"][b]
        np.testing.assert_allclose(obox.clip_boxes(inv, info[0], info[1]), G["box_clip"][b], **BOX)
        # the clamp itself, on the reference's own decoded boxes: exact
        np.testing.assert_array_equal(obox.clip_boxes(G["box_inv"][b], info[0], info[1]),
                                      G["box_clip"][b])
    # the masks were reached: a zero-area gt column is 0, a zero-area box row is -1
    assert (G["box_ov2"][0][:, 3] == 0).sum() >= 48 and (G["box_ov2"][:, 7] == -1).all()
    assert (G["box_ov3"][1, 12] == -1).all()


SL1 = [("sl1_rpn", (1, 2, 3)), ("sl1_rcnn", (1,))]


@pytest.mark.parametrize("p,dim", SL1)
def test_smooth_l1_composition(p, dim):
    from tlod.detector.losses import smooth_l1_loss
    pred = torch.from_numpy(G[p + "_pred"]).requires_grad_(True)
    loss = smooth_l1_loss(pred, *(torch.from_numpy(G[f"{p}_{k}"]) for k in
                                  ("tgt", "inside", "outside")),
                          sigma=float(G[p + "_sigma"][0]), dim=dim)
    loss.backward()
    close(loss.reshape(1), torch.from_numpy(G[p + "_loss"]))
    close(pred.grad, torch.from_numpy(G[p + "_grad"]))


def test_ref_roi_crop_theta_and_grid():
    """ref_roi_crop.theta is _affine_grid_gen's (x row first); _affine_theta holds the same
    entries with the y row first.  Both are a few float32 divisions in the same order: exact.
    The grid is theta[.., 0] * base + theta[.., 2] with base = linspace(-1, 1, G): three
    roundings on each side (base, product, sum; torch multiplies a (G*G, 3) base grid by
    theta), so at most 4 ulp of the largest term."""
    rois = G["aff_rois"]
    H, W = (int(v) for v in G["aff_hw"])
    th = ref_roi_crop.theta(rois, H, W)
    want = G["aff_theta"]
    np.testing.assert_array_equal(th[:, 1, 1], want[:, 0, 0])
    np.testing.assert_array_equal(th[:, 1, 2], want[:, 0, 2])
    np.testing.assert_array_equal(th[:, 0, 0], want[:, 1, 1])
    np.testing.assert_array_equal(th[:, 0, 2], want[:, 1, 2])
    assert not want[:, 0, 1].any() and not want[:, 1, 0].any()
    atol = 4 * 2.0 ** -23 * 2 * float(np.abs(th).max())           # |a * base + b| <= 2 max|theta|
    for g in (7, 14):
        grid_yx = ref_roi_crop.affine_grid_yx(rois, H, W, g)
        ref = G[f"aff_grid{g}"]                                    # (R, g, g, 2) in (x, y)
        err = float(np.abs(grid_yx[..., ::-1] - ref).max())
        print(f"grid {g}: max |restatement - reference| = {err:.3e} (bar {atol:.3e})")
        assert err <= atol


def test_second_tier_restatements():
    """MAF's DRM (float64): conv 1x1 -> ReLU -> oracle.maf_step.drm_chunks, exactly; US-DAF's
    _ImageDA: GRL(0.1) -> 1x1 -> ReLU -> 1x1 -> sigmoid in float64, value and input gradient."""
    from oracle.maf_step import drm_chunks
    x, w = torch.from_numpy(G["drm_x"]).double(), torch.from_numpy(G["drm_w"]).double()
    for s in (2, 4):
        y = drm_chunks(F.relu(F.conv2d(x, w)), s)
        assert torch.equal(y, torch.from_numpy(G[f"drm_y{s}"]))
    x = torch.from_numpy(G["ida_x"]).double().requires_grad_(True)
    w1, w2 = (torch.from_numpy(G[k]).double() for k in ("ida_w1", "ida_w2"))
    y = torch.sigmoid(F.conv2d(F.relu(F.conv2d(x, w1)), w2))
    y.backward(torch.from_numpy(G["ida_gy"]).double())
    close(y, torch.from_numpy(G["ida_y"]))
    close(-0.1 * x.grad, torch.from_numpy(G["ida_gx"]))


def test_generator_reproduces_the_fixture():
    """With the reference checkout in TLOD_REFERENCE_DIR: rerun the generator in memory; every
    array of the committed file comes out again, bit for bit, and nothing else does."""
    ref = os.environ.get(ENV)
    if not ref:
        pytest.skip(f"{ENV} is not set: no reference checkout to regenerate the fixture from")
    spec = importlib.util.spec_from_file_location(
        "make_reference_golden", os.path.join(HERE, "golden", "make_reference_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    out = gen.generate(ref)
    assert sorted(out) == sorted(G.files)
    for k in G.files:
        a, b = np.asarray(out[k]), G[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert a.tobytes() == b.tobytes(), k


# ============================================================================ GPU: the HIP path
@pytest.mark.gpu
@pytest.mark.parametrize("case", AT_CASES)
def test_hip_anchor_target(case):
    from tlod.config import setup_training_cfg
    from tlod.rpn.anchor_target import anchor_target, rpn_cfg_struct
    setup_training_cfg("vgg16")
    p = "at_" + case
    H, W = (int(v) for v in G[p + "_hw"])
    rp = Replay(p)
    got = anchor_target(t(G["anchors_base"]), H, W, STRIDE, t(G[p + "_gt"]), t(G[p + "_info"]),
                        rpn_cfg_struct(), rng=rp)
    assert rp.done()
    check_targets(p, AT_NAMES, got, exact=False)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PT_CASES)
def test_hip_proposal_target(case):
    from tlod.config import setup_training_cfg
    from tlod.rpn.proposal_target import proposal_target, rcnn_cfg_struct
    p = "pt_" + case
    want = rcnn_cfg_of(p)
    try:
        setup_training_cfg("res101" if want["batch"] == 128 else "vgg16")
        cs = rcnn_cfg_struct()
        assert (cs.batch_size, cs.bg_thresh_lo, cs.fg_fraction, cs.fg_thresh, cs.bg_thresh_hi) == \
            (want["batch"], want["bg_lo"], want["fg_frac"], want["fg_thresh"], want["bg_hi"])
        rp = Replay(p)
        got = proposal_target(t(G[p + "_rois_in"]), t(G[p + "_gt"]), cs, rng=rp)
    finally:
        setup_training_cfg("vgg16")
    assert rp.done()
    check_targets(p, PT_NAMES, got, exact=False)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PL_CASES)
def test_hip_proposal_layer(case):
    from tlod.rpn.proposal import proposal
    p = f"pl_{case}"
    pre, post, thr = G[p + "_cfg"]
    got = proposal(t(G[p + "_prob"]), t(G[p + "_deltas"]), t(G[p + "_info"]), t(G["anchors_base"]),
                   STRIDE, int(pre), int(post), float(thr))
    check_rois(p, got.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("case", PA_CASES)
def test_hip_proposal_keep_and_pick(case):
    from tlod.rpn.proposal import proposal_keep, proposal_pick
    p = f"pa_{case}"
    pre, post, thr = G[p + "_cfg"]
    kept, counts = proposal_keep(t(G[p + "_prob"]), t(G[p + "_deltas"]), t(G[p + "_info"]),
                                 t(G["anchors_base"]), STRIDE, int(pre), float(thr))
    np.testing.assert_array_equal(counts.cpu().numpy(), G[p + "_survivors"])
    rp = Replay(p)
    picks = [rp.picks() for _ in range(kept.shape[0])]
    assert rp.done()
    got = proposal_pick(kept, counts, int(post), pick=picks)
    check_rois(p, got.cpu().numpy())


@pytest.mark.gpu
def test_hip_rpn_box_loss():
    """rpn_losses' smooth-L1 half (sigma 3, summed over [1, 2, 3]) on the fixture's float64
    inputs rounded to float32; the class half gets seeded scores and labels of its own."""
    from tlod.detector.losses import rpn_losses
    p = "sl1_rpn"
    pred = t(G[p + "_pred"]).float().requires_grad_(True)
    tgt, inside, outside = (t(G[f"{p}_{k}"]).float() for k in ("tgt", "inside", "outside"))
    B, A4, H, W = pred.shape
    g = torch.Generator().manual_seed(0)
    score = torch.randn(B, A4 // 2, H, W, generator=g).to(dev)
    lab = torch.randint(-1, 2, (B, 1, (A4 // 4) * H, W), generator=g).float().to(dev)
    _, lb = rpn_losses(score, pred, lab, tgt, inside, outside, sigma=float(G[p + "_sigma"][0]))
    lb.backward()
    close(lb.reshape(1).cpu(), torch.from_numpy(G[p + "_loss"]))
    close(pred.grad.cpu(), torch.from_numpy(G[p + "_grad"]))


@pytest.mark.gpu
def test_hip_rcnn_box_loss():
    """rcnn_losses' smooth-L1 half (sigma 1, summed over [1]), class-agnostic boxes."""
    from tlod.detector.losses import rcnn_losses
    p = "sl1_rcnn"
    pred = t(G[p + "_pred"]).float().requires_grad_(True)
    tgt, inside, outside = (t(G[f"{p}_{k}"]).float() for k in ("tgt", "inside", "outside"))
    R = pred.shape[0]
    g = torch.Generator().manual_seed(1)
    cls = torch.randn(R, 9, generator=g).to(dev)
    lab = torch.randint(0, 9, (R,), generator=g).to(dev)
    _, _, _, lb = rcnn_losses(cls, pred, lab, tgt, inside, outside, agnostic=True,
                              sigma=float(G[p + "_sigma"][0]))
    lb.backward()
    close(lb.reshape(1).cpu(), torch.from_numpy(G[p + "_loss"]))
    close(pred.grad.cpu(), torch.from_numpy(G[p + "_grad"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["big", "small"])
def test_hip_clip_gradient(name):
    """FusedSGDClip(clip_norm=10) on three zero parameters with the recorded gradients, lr 1,
    no momentum, no weight decay: the update is minus the clipped gradient, so the parameters
    are minus clip_gradient's 'after'; norm_scale holds the norm and the factor."""
    from tlod.optim import FusedSGDClip
    before = [G[f"clipg_{name}_before_{k}"] for k in "abc"]
    after = [G[f"clipg_{name}_after_{k}"] for k in "abc"]
    params = [torch.nn.Parameter(torch.zeros(b.shape, device=dev)) for b in before]
    opt = FusedSGDClip([{"params": params, "lr": 1.0, "weight_decay": 0.0}], momentum=0.0,
                       clip_norm=10.0)
    opt.zero_grad()
    sum((p * t(b)).sum() for p, b in zip(params, before)).backward()
    opt.step()
    norm = float(np.sqrt(sum((b.astype(np.float64) ** 2).sum() for b in before)))
    want = torch.tensor([norm, 10.0 / max(norm, 10.0)])
    assert (want[1] < 1) == (name == "big")
    torch.testing.assert_close(opt.norm_scale.cpu(), want.float(), rtol=1e-5, atol=1e-6)
    for p, a in zip(params, after):
        torch.testing.assert_close(-p.detach().cpu(), torch.from_numpy(a), rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [2, 4])
def test_hip_drm_forward(scale):
    from tlod.da.maf import DRM
    m = DRM(8, 4, scale).to(dev)
    with torch.no_grad():
        m.conv_low_dim.weight.copy_(t(G["drm_w"]))
    y = m(t(G["drm_x"]))
    want = torch.from_numpy(G[f"drm_y{scale}"])
    assert tuple(y.shape) == tuple(want.shape)
    conv_close(y, want)


@pytest.mark.gpu
def test_hip_us_daf_image_head():
    from tlod.da.us_daf import _ImageDA
    m = _ImageDA(8).to(dev)
    with torch.no_grad():
        m.Conv1.weight.copy_(t(G["ida_w1"]))
        m.Conv2.weight.copy_(t(G["ida_w2"]))
    x = t(G["ida_x"]).requires_grad_(True)
    y = m(x)
    y.backward(t(G["ida_gy"]))
    conv_close(y, torch.from_numpy(G["ida_y"]))
    conv_close(x.grad, torch.from_numpy(G["ida_gx"]))
