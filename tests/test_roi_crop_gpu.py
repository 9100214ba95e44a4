"""RoI crop (POOLING_MODE 'crop') on the MI355X: the general grid sampler and the fused
crop + max-pool kernels, forward and backward, against the CPU restatement of the reference
(tests/ref_roi_crop.py), and the detectors running in 'crop' mode.

Shapes: B = 2 (image indexing), C in {5, 67} (channel tails: 67 = 64 + 3), a 7 x 9 map
(non-square: x / y swaps), P in {7, 3}, with and without the max-pool.  Six RoIs per image
(ref_roi_crop.edge_rois): inside, straddling two borders each way, entirely outside,
degenerate, and integer corners including xcoord == W - 1.

Tolerances: the sampler's four products of two weights in [0, 1] and three adds are a few ulp
of max|x|: 16 * 2^-24 * max|x| (bit-equality is expected and printed).  The fused forward
recomputes the affine grid (not torch's linspace rounding): 1e-5 * max|x|.  Backwards:
1e-5 * max|grad_in|, the project's RoI backward tolerance, against the fp64 autograd of the
restatement; two runs bit-identical.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_roi_crop as ref

pytestmark = pytest.mark.gpu
dev = "cuda"
B, H, W = 2, 7, 9
CASES = [(C, P, mp) for C in (5, 67) for P in (7, 3) for mp in (1, 0)]
SEED = 11


@functools.lru_cache(maxsize=None)
def inputs(C, B_=B):
    """(x, rois) of one channel count, shared (read-only) by every test."""
    x = ref.ramp_map(np.random.default_rng(SEED + C), B_, C, H, W)
    rois = ref.edge_rois(H, W, B_)
    x.setflags(write=False)
    rois.setflags(write=False)
    return x, rois


@functools.lru_cache(maxsize=None)
def samples(C, G):
    """The restated (R, C, G, G) samples and their (y, x) grid."""
    x, rois = inputs(C)
    grid = ref.affine_grid_yx(rois, H, W, G)
    return ref.sample(x, grid), grid


def t(a):
    return torch.from_numpy(np.array(a)).to(dev)  # (a copy: the shared inputs are read-only)


def grad_out_for(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def assert_unambiguous(v, scale):
    """The precondition of every max-pool comparison, on the CPU reference: in each 2x2
    window that is not all zero the winner leads by more than 1e-4 * max|x|."""
    gap, zero = ref.window_gap(v)
    worst = float(gap[~zero].min())
    print("smallest winner margin", worst, "bar", 1e-4 * scale)
    assert worst > 1e-4 * scale


# ---------------------------------------------------------------- 1. general sampler, forward
@pytest.mark.parametrize("C", [5, 67])
@pytest.mark.parametrize("G", [14, 7, 6, 3])
def test_sampler_forward(C, G):
    from tlod import _lib
    x, rois = inputs(C)
    want, grid = samples(C, G)
    xd, gd = t(x), t(grid)
    R = len(rois)
    out = torch.full((R, C, G, G), float("nan"), device=dev)
    _lib.check(_lib.lib().tlod_roi_crop_fwd_f32(_lib.ptr(xd), B, C, H, W, _lib.ptr(gd), R, G, G,
                                                _lib.ptr(out), _lib.stream_of(xd)), "fwd")
    got = out.cpu().numpy()
    assert not np.isnan(got).any(), "an output was left unwritten"
    assert np.all(got[3] == 0) and np.all(got[9] == 0)  # the RoIs entirely outside the map
    err = float(np.abs(got - want).max())
    print("sampler forward max |err| =", err, "bit-equal:", bool(np.array_equal(got, want)))
    assert err <= 16 * 2.0 ** -24 * float(np.abs(x).max())
    # the module form
    from tlod.roi_crop import _RoICrop
    np.testing.assert_array_equal(_RoICrop()(xd, gd).cpu().numpy(), got)


# ---------------------------------------------------------------- 2. fused forward
@pytest.mark.parametrize("C,P,mp", CASES)
def test_fused_forward(C, P, mp):
    from tlod.roi_crop import RoICropPool, _RoICrop, affine_grid_gen
    x, rois = inputs(C)
    G = 2 * P if mp else P
    v, _ = samples(C, G)
    scale = float(np.abs(x).max())
    if mp:
        assert_unambiguous(v, scale)
        want, want_idx = ref.max_pool_2x2(v)
    else:
        want = v
    xd, rd = t(x), t(rois)
    got = RoICropPool(P, 1 / 16, bool(mp))(xd, rd)
    err = float(np.abs(got.cpu().numpy() - want).max())
    print("fused forward max |err| =", err, "bar", 1e-5 * scale)
    assert err <= 1e-5 * scale
    # the unfused composition on the device: affine_grid_gen -> (y, x) swap -> _RoICrop -> max-pool
    gxy = affine_grid_gen(rd, (H, W), G)
    gyx = torch.stack([gxy[..., 1], gxy[..., 0]], 3).contiguous()
    comp = _RoICrop()(xd, gyx)
    if mp:
        comp = F.max_pool2d(comp, 2, 2)
    assert float((got - comp).abs().max()) <= 1e-5 * scale
    if mp:  # the argmax byte: the winner's place in its window
        from tlod import _lib
        out = torch.empty_like(got)
        am = torch.full(got.shape, 255, dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().tlod_roi_crop_pool_fwd_f32(
            _lib.ptr(xd), B, C, H, W, _lib.ptr(rd), len(rois), P, 1 / 16, 1, _lib.ptr(out),
            _lib.ptr(am), _lib.stream_of(xd)), "pool_fwd")
        np.testing.assert_array_equal(am.cpu().numpy(), want_idx)
        assert torch.equal(out, got)


# ---------------------------------------------------------------- 3. backwards
@pytest.mark.parametrize("C", [5, 67])
@pytest.mark.parametrize("G", [14, 7, 6, 3])
def test_sampler_backward(C, G):
    from tlod.roi_crop import _RoICrop
    x, rois = inputs(C)
    _, grid = samples(C, G)
    go = grad_out_for((len(rois), C, G, G), 5)
    x64 = torch.from_numpy(x).double().requires_grad_()
    ref.sample_t(x64, torch.from_numpy(grid)).backward(torch.from_numpy(go).double())
    want = x64.grad.numpy()
    runs = []
    for _ in range(2):
        xd = t(x).requires_grad_()
        gd = t(grid).requires_grad_()
        _RoICrop()(xd, gd).backward(t(go))
        assert gd.grad is not None and not gd.grad.any()  # the grid gradient: exactly zero
        runs.append(xd.grad.cpu().numpy())
    np.testing.assert_array_equal(runs[0], runs[1])
    err = float(np.abs(runs[0] - want).max())
    print("sampler backward max |err| =", err, "bar", 1e-5 * float(np.abs(want).max()))
    assert err <= 1e-5 * float(np.abs(want).max())


@pytest.mark.parametrize("C,P,mp", CASES)
def test_fused_backward(C, P, mp):
    from tlod.roi_crop import RoICropPool
    x, rois = inputs(C)
    if mp:
        assert_unambiguous(samples(C, 2 * P)[0], float(np.abs(x).max()))
    go = grad_out_for((len(rois), C, P, P), 6)
    x64 = torch.from_numpy(x).double().requires_grad_()
    ref.crop_pool_t(x64, rois, P, mp).backward(torch.from_numpy(go).double())
    want = x64.grad.numpy()
    runs = []
    for _ in range(2):
        xd = t(x).requires_grad_()
        RoICropPool(P, 1 / 16, bool(mp))(xd, t(rois)).backward(t(go))
        runs.append(xd.grad.cpu().numpy())
    np.testing.assert_array_equal(runs[0], runs[1])
    err = float(np.abs(runs[0] - want).max())
    print("fused backward max |err| =", err, "bar", 1e-5 * float(np.abs(want).max()))
    assert err <= 1e-5 * float(np.abs(want).max())


def test_backward_contention():
    """64 identical RoIs on one image, C = 3: every touched cell sums 64 RoIs' taps."""
    from tlod.roi_crop import RoICropPool, _RoICrop
    C, P, R = 3, 7, 64
    x = ref.ramp_map(np.random.default_rng(SEED), 1, C, H, W)
    rois = np.repeat(ref.edge_rois(H, W, 1)[:1], R, 0)
    grid = ref.affine_grid_yx(rois, H, W, 2 * P)
    assert_unambiguous(ref.sample(x, grid), float(np.abs(x).max()))
    for fused in (True, False):
        go = grad_out_for((R, C, P, P) if fused else (R, C, 2 * P, 2 * P), 7)
        x64 = torch.from_numpy(x).double().requires_grad_()
        y64 = ref.crop_pool_t(x64, rois, P, 1) if fused else ref.sample_t(x64, torch.from_numpy(grid))
        y64.backward(torch.from_numpy(go).double())
        want = x64.grad.numpy()
        runs = []
        for _ in range(2):
            xd = t(x).requires_grad_()
            y = RoICropPool(P, 1 / 16, True)(xd, t(rois)) if fused else _RoICrop()(xd, t(grid))
            y.backward(t(go))
            runs.append(xd.grad.cpu().numpy())
        np.testing.assert_array_equal(runs[0], runs[1])
        err = float(np.abs(runs[0] - want).max())
        print("contention", "fused" if fused else "sampler", "max |err| =", err, "bar",
              1e-5 * float(np.abs(want).max()))
        assert err <= 1e-5 * float(np.abs(want).max())


# ---------------------------------------------------------------- 4. unequal per-image counts
def test_fused_unequal_counts():
    """4 RoIs on image 0 and 7 on image 1 (the project batches source and target RoIs of
    different counts): the image is rois[:, 0]; compared with per-image reference calls.  A
    RoI naming no image ([0, B) is validated on the device) gives zeros and no gradient."""
    from tlod.roi_crop import RoICropPool
    C, P = 5, 7
    x, rois12 = inputs(C)
    rois = np.concatenate([rois12[[0, 1, 2, 5]], rois12[[6, 7, 8, 9, 10, 11, 6]]], 0)
    rois[-1, 1:] += 8.0
    n0 = 4
    parts = [(x[0:1], rois[:n0]), (x[1:2], rois[n0:])]
    for xi, ri in parts:
        assert_unambiguous(ref.sample(xi, ref.affine_grid_yx(ri, H, W, 2 * P)),
                           float(np.abs(x).max()))
    want = np.concatenate([ref.crop_pool(xi, ri, P, 1) for xi, ri in parts], 0)
    go = grad_out_for(want.shape, 8)
    gwant = []
    for (xi, ri), g in zip(parts, (go[:n0], go[n0:])):
        x64 = torch.from_numpy(xi).double().requires_grad_()
        ref.crop_pool_t(x64, ri, P, 1).backward(torch.from_numpy(g).double())
        gwant.append(x64.grad.numpy())
    gwant = np.concatenate(gwant, 0)
    xd = t(x).requires_grad_()
    got = RoICropPool(P, 1 / 16, True)(xd, t(rois))
    got.backward(t(go))
    assert float(np.abs(got.detach().cpu().numpy() - want).max()) <= 1e-5 * float(np.abs(x).max())
    assert float(np.abs(xd.grad.cpu().numpy() - gwant).max()) <= 1e-5 * float(np.abs(gwant).max())
    # image indices outside [0, B)
    bad = rois.copy()
    bad[0, 0], bad[5, 0] = 2.0, -1.0
    xd = t(x).requires_grad_()
    got = RoICropPool(P, 1 / 16, True)(xd, t(bad))
    got.backward(t(go))
    g = got.detach().cpu().numpy()
    assert not g[0].any() and not g[5].any()
    keep = [i for i in range(len(rois)) if i not in (0, 5)]
    np.testing.assert_array_equal(g[keep], want_dev(x, rois, P)[keep])
    go2 = go.copy()
    go2[[0, 5]] = 0
    xe = t(x).requires_grad_()
    RoICropPool(P, 1 / 16, True)(xe, t(rois)).backward(t(go2))
    np.testing.assert_array_equal(xd.grad.cpu().numpy(), xe.grad.cpu().numpy())


def want_dev(x, rois, P):
    from tlod.roi_crop import RoICropPool
    with torch.no_grad():
        return RoICropPool(P, 1 / 16, True)(t(x), t(rois)).cpu().numpy()


# ---------------------------------------------------------------- 5. detector level
def torch_crop_pool(feat, rois, P=7):
    """POOLING_MODE 'crop' from torch ops only (faster_rcnn.py:73-81 with today's
    align_corners=True spelled out): theta -> affine_grid -> grid_sample -> max_pool2d(2, 2).
    The image of a RoI is rois[:, 0].  Works in fp32 / fp64, on either device."""
    Hf, Wf = feat.shape[2:]
    r = rois.detach().to(feat.dtype)
    x1, y1, x2, y2 = (r[:, i:i + 1] / 16.0 for i in (1, 2, 3, 4))
    zero = torch.zeros_like(x1)
    theta = torch.cat([(x2 - x1) / (Wf - 1), zero, (x1 + x2 - Wf + 1) / (Wf - 1),
                       zero, (y2 - y1) / (Hf - 1), (y1 + y2 - Hf + 1) / (Hf - 1)], 1).view(-1, 2, 3)
    grid = F.affine_grid(theta, torch.Size((r.size(0), 1, 2 * P, 2 * P)), align_corners=True)
    v = F.grid_sample(feat[r[:, 0].long()], grid, mode="bilinear", padding_mode="zeros",
                      align_corners=True)
    return F.max_pool2d(v, 2, 2)


class _CropOracle:
    """Stands in for the oracle steps' RoI pooling function (they have no crop mode)."""

    @staticmethod
    def apply(feat, rois):
        return torch_crop_pool(feat, rois)


@pytest.fixture
def crop_cfg():
    """Switches a built model's cfg to the reference's 'crop' defaults; restores cfg after."""
    import copy
    from tlod.config import cfg
    saved = copy.deepcopy(cfg)

    def switch():
        cfg.POOLING_MODE = "crop"
        cfg.CROP_RESIZE_WITH_MAX_POOL = True
    yield switch
    cfg.clear()
    cfg.update(saved)


FR_LOSSES = (["rpn_loss_cls", "rpn_loss_box", "RCNN_loss_cls", "RCNN_loss_bbox"], [3, 4, 5, 6])
DAF_LOSSES = (FR_LOSSES[0] + ["DA_img_loss_cls", "DA_ins_loss_cls", "tgt_DA_img_loss_cls",
                              "tgt_DA_ins_loss_cls", "DA_cst_loss", "tgt_DA_cst_loss"],
              FR_LOSSES[1] + [8, 9, 10, 11, 12, 13])


@pytest.mark.parametrize("method,net", [("faster_rcnn", "vgg16"), ("daf", "vgg16"),
                                        ("daf", "res101")])
def test_detector_step_in_crop_mode(method, net, crop_cfg, monkeypatch):
    """One 192 x 320 training step with POOLING_MODE 'crop' (replayed draws): the losses equal
    those of the same model with _pool replaced by the torch composition within 1e-4; the
    gradient of the last trainable backbone conv weight passes the pattern-matched fp64 bar
    (helpers.pattern_grad_bar) against the oracle step pooling with that composition."""
    import oracle.daf_step as odaf
    import oracle.frcnn_step as ofr
    from helpers import arm_taps, pattern_grad_bar, record_pattern
    from tlod.detector.train import build_model
    m = build_model(method, dev, net, seed=2)
    crop_cfg()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    full = odaf.synthetic_batch(192, 320, seed=3)
    if method == "daf":
        o = odaf.OracleDAF(dropout=0.0, backbone=net).train()
        cpu_batch, (names, idx), o_total = full, DAF_LOSSES, odaf.total_loss
        dev_args = tuple(v.to(dev) for v in full)
    else:
        o = ofr.OracleFRCNN(m.n_classes, scales=(4, 8, 16, 32), dropout=0.0).train()
        cpu_batch, (names, idx), o_total = full[:3], FR_LOSSES, ofr.total_loss
        dev_args = tuple(v.to(dev) for v in full[:4])
    o.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)

    def step():
        m.zero_grad(set_to_none=True)
        m.replay_rng = np.random.RandomState(3)
        m.capture = {}
        out = m(*dev_args)
        m.total_loss(out).backward()
        torch.cuda.synchronize()
        return out

    # the same model, pooling with the torch composition
    with monkeypatch.context() as mp:
        mp.setattr(type(m), "_pool", lambda self, feat, rois: torch_crop_pool(feat, rois))
        want = [float(step()[i].detach()) for i in idx]
    taps = arm_taps(m)
    out = step()  # the crop kernels
    for name, i, w in zip(names, idx, want):
        g = float(out[i].detach())
        print(name, g, w)
        assert abs(g - w) <= 1e-4 * max(abs(w), 1e-3), (name, g, w)

    # gradient bar, on the last trainable backbone conv weight
    last = [k for k, p in o.named_parameters()
            if k.startswith("RCNN_base.") and p.ndim == 4 and p.requires_grad][-1]
    for k, p in o.named_parameters():
        p.requires_grad = k == last
    monkeypatch.setattr(odaf, "_RoIAlignAvgCPU", _CropOracle)
    monkeypatch.setattr(ofr, "_RoIAlignAvgCPU", _CropOracle)
    if method == "daf":
        ov = (m.capture["s_rois"].cpu().numpy(), m.capture["t_rois"].cpu().numpy())
        run = lambda mod, b: o_total(mod(b, np.random.RandomState(3), rois_override=ov))
        n_rows = out[7].numel()
    else:
        ov = m.capture["s_rois"].cpu().numpy()
        run = lambda mod, b: o_total(mod(*b, np.random.RandomState(3), rois_override=ov))
        n_rows = None
    own = record_pattern(o, lambda: run(o, cpu_batch).backward())
    errs = pattern_grad_bar(m, o, run, cpu_batch, taps, n_rows, own)
    assert list(errs) == [last]


def test_detector_eval_in_crop_mode(crop_cfg):
    """Eval mode: the 300 TEST RoIs through the crop kernels, finite class probabilities."""
    import oracle.daf_step as odaf
    from tlod.detector.train import build_model
    m = build_model("faster_rcnn", dev, "vgg16", seed=2).eval()
    crop_cfg()
    args = tuple(v.to(dev) for v in odaf.synthetic_batch(192, 320, seed=3)[:4])
    with torch.no_grad():
        rois, cls_prob, bbox_pred = m(*args)[:3]
    assert rois.shape == (1, 300, 5) and cls_prob.shape == (1, 300, m.n_classes)
    assert bool(torch.isfinite(cls_prob).all()) and bool(torch.isfinite(bbox_pred).all())
    torch.testing.assert_close(cls_prob.sum(-1), torch.ones(1, 300, device=dev))


@pytest.mark.parametrize("method", ["maf", "atf"])
def test_other_methods_train_in_crop_mode(method, crop_cfg):
    """MAF and ATF inherit the DAF detector's pooling: one tiny training step in 'crop' mode."""
    from tlod.detector.train import SyntheticCityscapes, build_model, make_optimizer, train_step
    m = build_model(method, dev, "vgg16")
    crop_cfg()
    data = SyntheticCityscapes(dev, H=192, W=320, G=4, pool=1, seed=7)
    v = float(train_step(m, make_optimizer(m, 2e-3), data.next()))
    torch.cuda.synchronize()
    assert np.isfinite(v)
