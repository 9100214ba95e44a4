"""The production (device-RNG) branch of every sampler, pinned exactly to tests/device_rng.py.

  proposal target   proposal_target(seed=s) == the HIP replay call fed pt_draws (torch.equal on
                    all five outputs) == oracle.rpn.proposal_target fed the same draws (exact,
                    regression targets at the family's rtol / atol 2e-6);
  anchor target     the labels == the candidates minus anchor_subset, per image and stream;
  proposal_pick     proposal_pick(seed=s) == proposal_pick(pick=pick_rows) == rows assembled
                    in numpy;
  dropout           out and grad bit for bit from dropout_keep and the float32 scale.

The inputs and the expected outputs are built without a GPU (the *_inputs / *_expected
functions and the case lists below); tests/test_device_rng_cpu.py imports them to show that
the builders hit the branches they name and that a defective rule changes some expectation.
"""
from collections import namedtuple

import numpy as np
import pytest
import torch

import device_rng as R
from helpers import gt_set, random_boxes
from oracle import rpn as orpn
from oracle.boxes import bbox_overlaps, generate_anchors

dev = "cuda"
gpu = pytest.mark.gpu
TGT = dict(rtol=2e-6, atol=2e-6)  # as tests/test_reference_golden.py
BASE = generate_anchors(scales=np.array([4, 8, 16, 32]), ratios=np.array([0.5, 1, 2]))
M64 = R.M64


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# =================================================================== proposal target
RCNN = {"vgg16": dict(orpn.DEFAULT_RCNN, batch=256), "res101": dict(orpn.DEFAULT_RCNN, batch=128)}
# imgs: the (nfg, nbg) each image is built to have; G gt rows per image; zeros: RoI rows that
# are neither (zero boxes overlap nothing: -1)
PtCase = namedtuple("PtCase", "name imgs G zeros net")
PT_CASES = [PtCase(f"nfg{n}", [(n, 300)], 1 if n == 1 else 8, 5, "vgg16")
            for n in (1, 63, 64, 65, 1024, 1025, 2049)]           # P = 1 .. 4096
PT_CASES += [
    PtCase("largest_sort_one_bg", [(4095, 1)], 8, 0, "vgg16"),    # R + G = 4096
    PtCase("few_fg", [(20, 300)], 8, 5, "vgg16"),                 # bg fills S - nfg
    PtCase("fg_only", [(308, 0)], 8, 0, "vgg16"),
    PtCase("bg_only", [(0, 500)], 4, 0, "vgg16"),
    PtCase("b2_ordinary_bgonly", [(100, 300), (0, 390)], 8, 7, "vgg16"),
    PtCase("b2_bgonly_ordinary", [(0, 390), (100, 300)], 8, 7, "vgg16"),
    PtCase("b2_both_ordinary", [(70, 200), (90, 150)], 8, 3, "vgg16"),
    PtCase("res101", [(200, 300)], 8, 5, "res101"),
    PtCase("seeds", [(200, 300)], 8, 5, "vgg16"),
]
PT_BY_NAME = {c.name: c for c in PT_CASES}
PT_SEEDS = (5, 2 ** 32 + 5, 2 ** 63 + 5)
PT_PARAMS = [(c.name, 5) for c in PT_CASES] + [("seeds", s) for s in PT_SEEDS[1:]] + \
            [("b2_ordinary_bgonly", 2 ** 32 + 5)]
LAYER_SEED = 3


def pt_layer_seed(k):
    """The seed of _ProposalTargetLayer(nclasses, seed=3)'s k-th call (k = 1, 2, ...)."""
    return ((LAYER_SEED + 7919) * 1000003 + k) & M64


def _pt_image(rng, nfg, nbg, R_rows, G):
    """One image's (rois (R, 5), gt (G, 5)) with exactly nfg fg and nbg bg candidates among
    the R RoIs and the G appended gts: fg = the gts and gts moved by up to 3 px per edge
    (IoU >= 0.55), bg = random boxes whose best IoU is below 0.45, the rest zero rows; all in
    a random row order, so the candidate lists are not contiguous."""
    if nfg == 0:
        gt = np.zeros((G, 5), np.float32)  # no object: every real box is background (IoU 0)
        fg = np.zeros((0, 4), np.float32)
        bg = random_boxes(rng, nbg)
    else:
        gt = gt_set(rng, G=G, pad=G)
        n = nfg - G
        assert n >= 0
        fg = gt[rng.integers(0, G, n), :4] + rng.integers(-3, 4, (n, 4)).astype(np.float32)
        pool = random_boxes(rng, 4 * nbg + 64)
        ov = bbox_overlaps(pool, gt).max(1)
        bg = pool[(ov >= 0) & (ov < 0.45)][:nbg]
        assert len(bg) == nbg
    rows = np.zeros((R_rows, 4), np.float32)
    rows[:len(fg)] = fg
    rows[len(fg):len(fg) + nbg] = bg
    rois = np.zeros((R_rows, 5), np.float32)
    rois[:, 1:] = rows[rng.permutation(R_rows)]
    return rois, gt


_pt_cache = {}


def pt_inputs(name):
    """(rois (B, R, 5), gt (B, G, 5), counts [(nfg, nbg)] from the oracle's overlaps)."""
    if name in _pt_cache:
        return _pt_cache[name]
    c = PT_BY_NAME[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    R_rows = max(max(nfg - c.G, 0) + nbg for nfg, nbg in c.imgs) + c.zeros
    imgs = [_pt_image(rng, nfg, nbg, R_rows, c.G) for nfg, nbg in c.imgs]
    rois, gt = np.stack([i[0] for i in imgs]), np.stack([i[1] for i in imgs])
    cfg, counts = RCNN[c.net], []
    for b in range(len(imgs)):
        allr = np.concatenate([rois[b, :, 1:], gt[b, :, :4]])
        mo = bbox_overlaps(allr, gt[b]).max(1)
        fgm = mo >= np.float32(cfg["fg_thresh"])
        bgm = (mo < np.float32(cfg["bg_hi"])) & (mo >= np.float32(cfg["bg_lo"]))
        assert mo[fgm].min(initial=1.0) >= 0.55 and mo[bgm].max(initial=0.0) < 0.45  # no f32 edge
        counts.append((int(fgm.sum()), int(bgm.sum())))
    assert counts == [tuple(i) for i in c.imgs], (name, counts)
    _pt_cache[name] = (rois, gt, counts)
    return _pt_cache[name]


def pt_fg_per(cfg):
    return int(np.round(cfg["fg_frac"] * cfg["batch"])) or 1


def pt_replay(name, seed):
    cfg = RCNN[PT_BY_NAME[name].net]
    return R.Replay(pt_inputs(name)[2], cfg["batch"], pt_fg_per(cfg), seed)


def pt_expected(name, seed):
    """The oracle's five outputs under the restated draws."""
    rois, gt, _ = pt_inputs(name)
    rp = pt_replay(name, seed)
    out = orpn.proposal_target(rois, gt, rp, RCNN[PT_BY_NAME[name].net])
    assert rp.done()
    return out


def _pt_device(name, seed, layer=None):
    """(production outputs, HIP replay outputs, device counts) under the case's config."""
    from tlod import _lib
    from tlod.config import setup_training_cfg
    from tlod.rpn.proposal_target import proposal_target, rcnn_cfg_struct
    c = PT_BY_NAME[name]
    rois, gt, counts = pt_inputs(name)
    want = RCNN[c.net]
    try:
        setup_training_cfg(c.net)
        cs = rcnn_cfg_struct()
        assert (cs.batch_size, cs.bg_thresh_lo, cs.fg_fraction, cs.fg_thresh, cs.bg_thresh_hi) == \
            (want["batch"], want["bg_lo"], want["fg_frac"], want["fg_thresh"], want["bg_hi"])
        r, g = t(rois), t(gt)
        B, Rr, G = r.shape[0], r.shape[1], g.shape[1]
        L = _lib.lib()
        ws = _lib.workspace(L.tlod_proposal_target_workspace_bytes(B, Rr, G), r.device,
                            "proposal_target")
        cnt = torch.empty(2 * B, dtype=torch.int32, device=dev)
        _lib.check(L.tlod_proposal_target_count_f32(_lib.ptr(r), B, Rr, _lib.ptr(g), G, cs,
                                                    _lib.ptr(cnt), _lib.ptr(ws), ws.numel(),
                                                    _lib.stream_of(r)), "proposal_target_count")
        assert cnt.cpu().numpy().reshape(B, 2).tolist() == [list(x) for x in counts]
        if layer is not None:
            return [layer(r, g, None) for _ in range(2)]
        prod = proposal_target(r, g, cs, seed=seed)
        rp = pt_replay(name, seed)
        hip = proposal_target(r, g, cs, rng=rp)
        assert rp.done()
    finally:
        setup_training_cfg("vgg16")
    return prod, hip


PT_NAMES = ("rois", "labels", "targets", "inside", "outside")


def _check_pt(got, ref):
    for k, g, r in zip(PT_NAMES, got, ref):
        g = g.cpu().numpy()
        if k == "targets":
            np.testing.assert_allclose(g, r, err_msg=k, **TGT)
        else:
            np.testing.assert_array_equal(g, r, err_msg=k)


@gpu
@pytest.mark.parametrize("name,seed", PT_PARAMS)
def test_proposal_target_production_exact(name, seed):
    """The production call draws what pt_draws restates: the LDS sort over (key32, position)
    at every P, the with-replacement draws of all three branches, the streams of image b."""
    prod, hip = _pt_device(name, seed)
    for k, a, b in zip(PT_NAMES, prod, hip):
        assert torch.equal(a, b), k
    _check_pt(prod, pt_expected(name, seed))


@gpu
def test_proposal_target_seeds_differ():
    """Seeds 5, 2^32 + 5 and 2^63 + 5 each match the restatement (above) and give three
    different samples: no half of the seed is lost on the way to the kernel."""
    outs = [_pt_device("seeds", s)[0][0].cpu().numpy() for s in PT_SEEDS]
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], outs[2]) and \
        not np.array_equal(outs[1], outs[2])


@gpu
def test_proposal_target_layer_seed_derivation():
    from tlod.rpn.proposal_target import _ProposalTargetLayer
    layer = _ProposalTargetLayer(9, seed=LAYER_SEED)
    calls = _pt_device("b2_both_ordinary", None, layer=layer)
    for k, got in enumerate(calls, start=1):
        s = pt_layer_seed(k)
        assert s > 2 ** 32
        direct = _pt_device("b2_both_ordinary", s)[0]
        for n, a, b in zip(PT_NAMES, got, direct):
            assert torch.equal(a, b), (k, n)
        _check_pt(got, pt_expected("b2_both_ordinary", s))
    assert not torch.equal(calls[0][0], calls[1][0])


# =================================================================== anchor target
AtCase = namedtuple("AtCase", "name H W B kind")
AT_CASES = [
    AtCase("b2_lds", 37, 75, 2, "big"),       # N = 33300: at_sample_lds_kernel; image 1: streams 2, 3
    AtCase("b2_list", 50, 100, 2, "big"),     # N = 60000: at_sample_kernel / block_random_subset
    AtCase("few_fg", 37, 75, 1, "small"),     # nfg < 128: only bg is subsampled
    AtCase("few_fg_list", 50, 100, 1, "small"),
    AtCase("tiny_map", 5, 6, 1, "tiny"),      # nfg + nbg <= 256: nothing dropped
    AtCase("seeds", 37, 75, 1, "big"),
]
AT_BY_NAME = {c.name: c for c in AT_CASES}
AT_SEEDS = (5, 2 ** 32 + 5)
AT_PARAMS = [(c.name, 5) for c in AT_CASES] + [("seeds", 2 ** 32 + 5), ("b2_list", 2 ** 62 - 1)]


def at_layer_seed(k):
    return (LAYER_SEED * 1000003 + k) & M64


_at_cache = {}


def at_inputs(name):
    """(gts (B, 50, 5), im_info (B, 3), candidate labels (B, A H W) in output order)."""
    if name in _at_cache:
        return _at_cache[name]
    c = AT_BY_NAME[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    imw, imh = c.W * 16, c.H * 16
    gts = []
    for _ in range(c.B):
        if c.kind == "big":      # many fg candidates (as test_anchor_target_device_rng_exact_subset)
            g = gt_set(rng, G=50, W=imw, H=imh)
            g[:, 2:4] = np.maximum(g[:, 2:4], g[:, 0:2] + 200)
            g[:, 2] = np.minimum(g[:, 2], imw - 1)
            g[:, 3] = np.minimum(g[:, 3], imh - 1)
        elif c.kind == "small":  # one 48 x 40 object
            g = np.zeros((50, 5), np.float32)
            g[0] = [301, 203, 348, 242, 3]
        else:
            g = gt_set(rng, G=2, W=imw, H=imh)
        gts.append(g)
    gts = np.stack(gts)
    info = np.array([[imh, imw, 1.0]] * c.B, np.float32)
    ident = type("N", (), {"permutation": lambda self, n: np.arange(n)})()
    cfg = dict(orpn.DEFAULT_RPN)
    cfg["batch"] = 10 ** 9  # no subsampling: the candidates
    cand = orpn.anchor_target(c.H, c.W, gts, info, BASE, 16, ident, cfg)[0].reshape(c.B, -1)
    _at_cache[name] = (gts, info, cand)
    return _at_cache[name]


def at_counts(name):
    cand = at_inputs(name)[2]
    return [(int((l == 1).sum()), int((l == 0).sum())) for l in cand]


def at_expected(name, seed, batch=256, num_fg=128):
    """Labels (B, A H W) after subsampling: per image and kind, the m smallest
    (key32, anchor index) candidates are dropped."""
    c = AT_BY_NAME[name]
    cand = at_inputs(name)[2]
    A, HW = BASE.shape[0], c.H * c.W
    p = np.arange(A * HW)
    idx = (p % HW) * A + p // HW  # output (a, h, w) -> the kernels' anchor index (h, w, a)
    exp = cand.copy()
    for b in range(c.B):
        st_fg, st_bg = R.anchor_streams(b)
        fg = np.nonzero(cand[b] == 1)[0]
        exp[b, fg[R.anchor_subset(idx[fg], len(fg) - num_fg, seed, st_fg)]] = -1
        bg = np.nonzero(cand[b] == 0)[0]
        m_bg = len(bg) - (batch - min(len(fg), num_fg))
        exp[b, bg[R.anchor_subset(idx[bg], m_bg, seed, st_bg)]] = -1
    return exp


def _at_device(name, seed):
    from tlod.config import setup_training_cfg
    from tlod.rpn.anchor_target import anchor_target, rpn_cfg_struct
    setup_training_cfg("vgg16")
    c = AT_BY_NAME[name]
    gts, info, _ = at_inputs(name)
    return anchor_target(t(BASE.astype(np.float32)), c.H, c.W, 16, t(gts), t(info),
                         rpn_cfg_struct(), seed=seed)[0].reshape(c.B, -1).cpu().numpy()


@gpu
@pytest.mark.parametrize("name,seed", AT_PARAMS)
def test_anchor_target_production_exact(name, seed):
    exp = at_expected(name, seed)
    for nfg, nbg in [((l == 1).sum(), (l == 0).sum()) for l in exp]:
        assert nfg <= 128 and nfg + nbg <= 256
    np.testing.assert_array_equal(_at_device(name, seed), exp)


@gpu
def test_anchor_target_seeds_differ():
    a, b = (_at_device("seeds", s) for s in AT_SEEDS)
    assert not np.array_equal(a, b)


@gpu
def test_anchor_target_layer_seed_derivation():
    from tlod.config import setup_training_cfg
    from tlod.rpn.anchor_target import _AnchorTargetLayer
    setup_training_cfg("vgg16")
    c = AT_BY_NAME["b2_lds"]
    gts, info, _ = at_inputs(c.name)
    layer = _AnchorTargetLayer(16, [4, 8, 16, 32], [0.5, 1, 2], seed=LAYER_SEED).to(dev)
    score = torch.empty(c.B, 2 * BASE.shape[0], c.H, c.W, device=dev)
    calls = [layer((score, t(gts), t(info), None))[0].reshape(c.B, -1).cpu().numpy()
             for _ in range(2)]
    for k, got in enumerate(calls, start=1):
        np.testing.assert_array_equal(got, at_expected(c.name, at_layer_seed(k)))
    assert not np.array_equal(calls[0], calls[1])


# =================================================================== proposal_pick
#            counts          cap    post  head (None: post // 4)
PICK_CASES = [
    ((3, 10), 64, 16, None), ((40, 16), 64, 16, None),         # the four of
    ((5000, 300), 6000, 256, None), ((64, 65), 300, 256, None),  # test_pa_atf_ops_gpu
    ((16384, 2049), 16384, 256, None),   # n = 16320: eight key tiles; n = 1985
    ((16384, 2049), 16384, 256, 0),      # n = kPickMaxRows exactly; n just past one key tile
    ((321, 64 + 63), 400, 256, None),    # n = 257 and 63: a multiple of neither 64 nor 256
    ((64, 400), 512, 256, None),         # k = 0 (count == head) beside k = 192
    ((300, 50), 512, 64, 0),             # no head: every row is drawn
    ((300, 50), 512, 64, 64),            # head == post: nothing is drawn
]
PICK_SEEDS = (11, 2 ** 32 + 11, 2 ** 62 - 1)


def pick_kept(counts, cap):
    """Hand-made survivor lists: distinct boxes, zeros after each image's count."""
    g = torch.Generator().manual_seed(sum(counts) + cap)
    kept = torch.zeros(len(counts), cap, 4)
    for b, n in enumerate(counts):
        kept[b, :n] = torch.rand(n, 4, generator=g) * 100 + 1 + b
    return kept, torch.tensor(counts, dtype=torch.int32)


def pick_head(post, head):
    return int(post * 0.25) if head is None else head


def pick_expected(counts, cap, post, head, seed):
    """(rows (B, post, 5) assembled in numpy, [pick_rows per image])."""
    kept = pick_kept(counts, cap)[0].numpy()
    head = pick_head(post, head)
    want = np.zeros((len(counts), post, 5), np.float32)
    picks = []
    for b, n in enumerate(counts):
        nh, rest = min(n, head), max(n - head, 0)
        rows = R.pick_rows(rest, min(rest, post - head), seed, b)
        want[b, :, 0] = b
        want[b, :nh, 1:] = kept[b, :nh]
        want[b, nh:nh + len(rows), 1:] = kept[b, head + rows]
        picks.append(rows)
    return want, picks


@gpu
@pytest.mark.parametrize("counts,cap,post,head", PICK_CASES,
                         ids=["-".join(map(str, c[0] + c[1:])) for c in PICK_CASES])
def test_proposal_pick_production_exact(counts, cap, post, head):
    from tlod.rpn.proposal import proposal_pick
    kept, cnt = pick_kept(counts, cap)
    kd, cd = kept.to(dev), cnt.to(dev)
    outs = []
    for seed in PICK_SEEDS:
        want, picks = pick_expected(counts, cap, post, head, seed)
        got = proposal_pick(kd, cd, post, head=head, seed=seed)
        replay = proposal_pick(kd, cd, post, head=head, pick=picks)
        assert torch.equal(got, replay), seed
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=str(seed))
        outs.append(want)
    h = pick_head(post, head)
    if any(n - h > post - h > 0 for n in counts):  # a real choice somewhere
        assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], outs[2])


# =================================================================== ReLU + dropout
DROP_SHAPES = [(1,), (3,), (255,), (257,), (8192 * 256 + 259,), (556, 4096)]
DROP_PS = (0.5, 0.1, 0.9)
DROP_SEEDS = (123, 2 ** 32 + 123, 2 ** 62 - 1)
# every shape with every p, the seeds taken in turn; every seed with every p at n = 257
DROP_PARAMS = [(sh, p, DROP_SEEDS[(i + j) % 3]) for i, sh in enumerate(DROP_SHAPES)
               for j, p in enumerate(DROP_PS)]
DROP_PARAMS += [((257,), p, s) for p in DROP_PS for s in DROP_SEEDS
                if ((257,), p, s) not in DROP_PARAMS]
EDGE_IDX = 100  # where the hand-placed draw of the threshold cases sits


def drop_edge_seed(p, below=0):
    """A seed whose draw at EDGE_IDX equals float64(float32(p)) exactly (below = 1: one unit
    of 2^-53 under it).  float32(p) has 24 significant bits, so thr * 2^53 is an integer."""
    thr = float(np.float32(p)) * 2.0 ** 53
    assert thr == int(thr)
    return R.seed_for(R.DROPOUT_STREAM, EDGE_IDX, ((int(thr) - below) << 11) | 0x2a5)


DROP_EDGE = [(p, below) for p in DROP_PS for below in (0, 1)]


def drop_input(shape):
    g = torch.Generator().manual_seed(int(np.prod(shape)))
    y = torch.randn(shape, generator=g)
    f = y.view(-1)
    f[5::7][:5] = 0.0
    f[3::11][:5] = -0.0
    return y


def drop_scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))  # 1.f / (1.f - p)


def drop_expected(y, p, seed):
    """relu_dropout_kernel's output for y (a CPU tensor): kept positives times the scale."""
    keep = torch.from_numpy(R.dropout_keep(y.numel(), p, seed)).view(y.shape)
    scale = torch.tensor(float(drop_scale(p)), dtype=torch.float32)
    return torch.where(keep & (y > 0), y * scale, torch.zeros_like(y))


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


def _check_dropout(y, p, seed):
    from tlod.linear import ReluDropoutFunction
    want = drop_expected(y, p, seed)
    yr = y.to(dev).requires_grad_(True)
    out = ReluDropoutFunction.apply(yr, p, seed)
    assert torch.equal(_bits(out).cpu(), _bits(want))
    dout = torch.randn(y.shape, generator=torch.Generator().manual_seed(1))
    out.backward(dout.to(dev))
    scale = torch.tensor(float(drop_scale(p)), dtype=torch.float32)
    assert torch.equal(_bits(yr.grad).cpu(),
                       _bits(torch.where(want > 0, dout * scale, torch.zeros_like(dout))))
    return out.detach()


@gpu
@pytest.mark.parametrize("shape,p,seed", DROP_PARAMS,
                         ids=["x".join(map(str, sh)) + f"-p{p}-s{s}" for sh, p, s in DROP_PARAMS])
def test_relu_dropout_mask_exact(shape, p, seed):
    _check_dropout(drop_input(shape), p, seed)


@gpu
@pytest.mark.parametrize("p,below", DROP_EDGE)
def test_relu_dropout_threshold_is_inclusive(p, below):
    """A draw exactly on float64(float32(p)) keeps the element; one unit below drops it."""
    y = drop_input((257,)).abs() + 0.5
    seed = drop_edge_seed(p, below)
    out = _check_dropout(y, p, seed)
    assert bool(out[EDGE_IDX] > 0) == (below == 0)


@gpu
def test_relu_dropout_seeds_differ():
    y = drop_input((257,)).abs() + 0.5
    outs = [_check_dropout(y, 0.5, s) for s in DROP_SEEDS]
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])


@gpu
def test_relu_dropout_module_seed_draw():
    """relu_dropout takes its seed from torch's CPU generator: one randint(0, 2^62) per call."""
    from tlod.linear import ReluDropoutFunction, relu_dropout
    y = drop_input((255,))
    yd, drop = y.to(dev), torch.nn.Dropout(0.5)
    torch.manual_seed(7)
    got = [relu_dropout(yd, drop) for _ in range(2)]
    torch.manual_seed(7)
    seeds = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(2)]
    assert seeds[0] != seeds[1] and max(seeds) > 2 ** 32
    for o, s in zip(got, seeds):
        assert torch.equal(o, ReluDropoutFunction.apply(yd, 0.5, s))
        assert torch.equal(_bits(o).cpu(), _bits(drop_expected(y, 0.5, s)))
    assert not torch.equal(got[0], got[1])
