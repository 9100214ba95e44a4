"""The PA-ATF device ops (include/tlod_pa_atf.h) at the smallest shapes that can still go wrong.

Strided convolution (tlod.conv.StridedConv2d) against fp64 F.conv2d and its autograd under
tests/test_linear_gpu.py's bf16x6 bars (1e-5 normwise, 1e-4 elementwise against max|ref|);
im2col bit for bit against F.unfold; col2im's exact zeros where no window reaches.  The channel
gate against a numpy statement of adaptive_max_pool2d's scan (arg exact, mask within one fp32
ulp of the fp64 sigmoid) and its backward bit for bit against torch's sigmoid backward routed
to arg.  The prototype pooling bit for bit against the torch composition over
tlod.roi_pool._RoIPooling, its backward within 1e-6 of an fp64 scatter through the same
argmax, and twice the same bits.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
dev = "cuda"
NRM, ELT = 1e-5, 1e-4  # tests/test_linear_gpu.py BARS["bf16x6"]


def _close(got, ref, what=""):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nrm = float((got - ref).norm() / max(float(ref.norm()), 1e-30))
    elt = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
    print(f"{what}: normwise {nrm:.3e} elementwise {elt:.3e}")
    assert nrm <= NRM, f"{what}: normwise rel err {nrm:.3e}"
    assert elt <= ELT, f"{what}: elementwise err {elt:.3e}"


# ------------------------------------------------------------------ strided convolution
#          N   C   H   W  KS  s  p  Cout
SHAPES = [(1, 8, 20, 22, 5, 3, 0, 8),        # the smallest map the mask net accepts
          (2, 24, 23, 31, 5, 3, 0, 40),      # ragged everywhere, trailing columns uncovered
          (1, 16, 7, 9, 3, 2, 0, 16),
          (1, 8, 3, 3, 3, 2, 0, 4),          # a 1 x 1 output
          (1, 16, 9, 11, 3, 2, 1, 16),       # IDF's form
          (8, 32, 7, 7, 3, 2, 0, 16),        # CLUB's form
          (1, 256, 20, 22, 5, 3, 0, 256)]    # K = 6400, split-K
_REF = {}


def _conv_case(shape, relu):
    """Inputs and the fp64 reference of one case, computed once."""
    key = (shape, relu)
    if key not in _REF:
        N, C, H, W, KS, s, p, Cout = shape
        g = torch.Generator().manual_seed(sum(shape) + 17 * relu)
        x = torch.randn(N, C, H, W, generator=g)
        w = torch.randn(Cout, C, KS, KS, generator=g) / (C * KS * KS) ** 0.5
        b = torch.randn(Cout, generator=g)
        xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
        y = F.conv2d(xd, wd, bd, s, p)
        y = F.relu(y) if relu else y
        gy = torch.randn(y.shape, generator=g)
        (y * gy.double()).sum().backward()
        _REF[key] = (x, w, b, gy, y.detach(), xd.grad, wd.grad, bd.grad)
    return _REF[key]


def _run_conv(shape, relu):
    from tlod.conv import StridedConv2d
    N, C, H, W, KS, s, p, Cout = shape
    x, w, b, gy, y_ref, dx_ref, dw_ref, db_ref = _conv_case(shape, relu)
    m = StridedConv2d(C, Cout, KS, stride=s, padding=p, relu=relu).to(dev)
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    m.act_tap = []
    xg = x.to(dev).requires_grad_(True)
    y = m(xg)
    assert tuple(y.shape) == tuple(y_ref.shape)
    assert len(m.act_tap) == 1 and torch.equal(m.act_tap[0], y.detach())
    (y * gy.to(dev)).sum().backward()
    tag = f"{shape} relu={relu}"
    _close(y, y_ref, tag + " y")
    _close(xg.grad, dx_ref, tag + " dx")
    _close(m.weight.grad, dw_ref, tag + " dw")
    _close(m.bias.grad, db_ref, tag + " db")
    return y


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_strided_conv_against_fp64(shape, relu):
    y = _run_conv(shape, relu)
    # logically NCHW, channels-last in memory (the GEMM's rows)
    assert y.permute(0, 2, 3, 1).is_contiguous()


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4]])
def test_strided_conv_switch_off_is_f_conv2d(shape, monkeypatch):
    monkeypatch.setenv("TLOD_SCONV", "0")
    from tlod import conv
    assert not conv.sconv_on()
    called = []
    monkeypatch.setattr(conv, "im2col", lambda *a, **k: called.append(1))
    _run_conv(shape, True)
    assert not called


def test_strided_conv_without_input_or_bias_gradient():
    """A frozen input (no dgrad) and a bias-free conv: only the weight gradient runs."""
    from tlod.conv import StridedConv2d
    shape = SHAPES[2]
    N, C, H, W, KS, s, p, Cout = shape
    x, w, _, gy, _, _, _, _ = _conv_case(shape, False)
    m = StridedConv2d(C, Cout, KS, stride=s, padding=p, bias=False).to(dev)
    with torch.no_grad():
        m.weight.copy_(w)
    y = m(x.to(dev))
    (y * gy.to(dev)).sum().backward()
    wd = w.double().requires_grad_(True)
    (F.conv2d(x.double(), wd, None, s, p) * gy.double()).sum().backward()
    _close(m.weight.grad, wd.grad, "dw, no dgrad, no bias")


@pytest.mark.parametrize("shape", SHAPES[:6] + [(1, 3, 24, 31, 5, 3, 0, 1), (1, 3, 6, 5, 3, 1, 2, 1),
                                                (2, 5, 9, 8, 1, 2, 0, 1)])
def test_im2col_is_unfold_and_col2im_its_adjoint(shape):
    from tlod.conv import col2im, conv_out_size, im2col
    N, C, H, W, KS, s, p, _ = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(N, C, H, W, generator=g).to(dev)
    col = im2col(x, KS, s, p)
    Ho, Wo = conv_out_size(H, W, KS, s, p)
    want = F.unfold(x, KS, padding=p, stride=s).transpose(1, 2).reshape(N * Ho * Wo, C * KS * KS)
    assert torch.equal(col, want)
    dcol = (torch.rand(col.shape, generator=g) + 0.5).to(dev)  # positive: a covered cell is > 0
    dx = col2im(dcol, (N, C, H, W), KS, s, p)
    fold = F.fold(dcol.double().view(N, Ho * Wo, -1).transpose(1, 2), (H, W), KS, padding=p,
                  stride=s)
    assert float((dx.double() - fold).abs().max()) <= 1e-6 * float(fold.abs().max())
    covered = F.fold(torch.ones_like(dcol).view(N, Ho * Wo, -1).transpose(1, 2), (H, W), KS,
                     padding=p, stride=s) > 0
    assert torch.equal(dx != 0, covered)          # exact zeros where no window reaches
    if p == 0 and s <= KS:  # the windows tile a leading block without gaps
        hc, wc = (Ho - 1) * s + KS, (Wo - 1) * s + KS
        assert int((~covered).sum()) == N * C * (H * W - hc * wc)


def test_col2im_leaves_trailing_rows_and_columns_zero():
    from tlod.conv import col2im
    # (24 - 5) % 3 = 1 and (31 - 5) % 3 = 2: row 23 and columns 29, 30 are outside every window
    dcol = torch.ones(7 * 9, 3 * 25, device=dev)
    dx = col2im(dcol, (1, 3, 24, 31), 5, 3, 0)
    assert torch.count_nonzero(dx[:, :, 23:]).item() == 0
    assert torch.count_nonzero(dx[:, :, :, 29:]).item() == 0
    assert bool((dx[:, :, :23, :29] >= 1).all()) and float(dx.max()) == 4.0


# ------------------------------------------------------------------ channel gate
def _gate_input(shape, seed):
    N, C, h, w = shape
    z = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    if C >= 5 and h * w > 1:
        z[0, 0] = 1.5                       # a constant plane: arg 0
        z[0, 1] = -z[0, 1].abs() - 1        # all negative
        z[0, 2, -1, -1] = 100.0             # the maximum is the last cell
        z[0, 3].view(-1)[h * w // 2] = float("nan")
        z[0, 4].view(-1)[1] = z[0, 4].max() # the maximum twice: the first one counts
    return z


def _gate_ref(z):
    """adaptive_max_pool2d's scan: val > max or isnan(val) takes over."""
    zz = z.numpy().reshape(z.shape[0] * z.shape[1], -1)
    arg = np.zeros(zz.shape[0], np.int32)
    for i, row in enumerate(zz):
        nan = np.flatnonzero(np.isnan(row))
        arg[i] = nan[-1] if nan.size else int(np.argmax(row))
    mx = zz[np.arange(zz.shape[0]), arg].astype(np.float64)
    with np.errstate(over="ignore"):
        return arg.reshape(z.shape[:2]), (1.0 / (1.0 + np.exp(-mx))).reshape(z.shape[:2])


@pytest.mark.parametrize("shape", [(1, 5, 1, 1), (2, 70, 3, 6), (1, 256, 11, 24)])
def test_gate_forward_and_backward(shape):
    from tlod.da import pa_atf
    N, C, h, w = shape
    z = _gate_input(shape, 3)
    arg_ref, m_ref = _gate_ref(z)
    zg = z.to(dev).requires_grad_(True)
    mask, arg = pa_atf.gate(zg)
    assert tuple(mask.shape) == (N, C, 1, 1) and arg.dtype == torch.int32
    np.testing.assert_array_equal(arg.cpu().numpy(), arg_ref)
    if C >= 5 and h * w > 1:
        assert arg_ref[0, 0] == 0 and arg_ref[0, 2] == h * w - 1 and arg_ref[0, 3] == h * w // 2
        assert arg_ref[0, 4] <= 1
    got = mask.detach().cpu().numpy().reshape(N, C)
    m32 = m_ref.astype(np.float32)
    ok = np.isfinite(m_ref)
    assert np.isnan(got[~ok]).all() and int((~ok).sum()) == (1 if C >= 5 and h * w > 1 else 0)
    assert (np.abs(got[ok].astype(np.float64) - m_ref[ok]) <= np.spacing(m32[ok])).all()
    # against the torch composition on the same device: same arg wherever there is no NaN
    m_t, arg_t = pa_atf.gate_torch(z.to(dev))
    assert torch.equal(arg_t, arg)
    # the backward, bit for bit: torch's sigmoid backward from this mask, routed to arg
    dmask = torch.randn(N, C, 1, 1, generator=torch.Generator().manual_seed(4)).to(dev)
    (mask * dmask).sum().backward()
    want = torch.zeros(N * C, h * w, device=dev)
    g = torch.ops.aten.sigmoid_backward(dmask, mask.detach()).view(-1)
    want[torch.arange(N * C, device=dev), arg.view(-1).long()] = g
    assert torch.equal(zg.grad.view(N * C, -1)[ok.reshape(-1)], want[ok.reshape(-1)])
    assert torch.count_nonzero(zg.grad.view(N * C, -1)[ok.reshape(-1)]).item() <= int(ok.sum())


def test_gate_switch_off_is_the_torch_composition(monkeypatch):
    from tlod.da import pa_atf
    z = _gate_input((2, 70, 3, 6), 5)
    z[0, 3] = torch.nan_to_num(z[0, 3])
    m1, a1 = pa_atf.gate(z.to(dev))
    monkeypatch.setenv("TLOD_FUSED_PA_ATF", "0")
    assert not pa_atf.fused_pa_atf()
    m0, a0 = pa_atf.gate(z.to(dev))
    assert torch.equal(a0, a1) and torch.allclose(m0, m1, rtol=3e-7, atol=0)


# ------------------------------------------------------------------ the 14 loss terms
def _loss_case(map_shape, G, seed):
    g = torch.Generator().manual_seed(seed)
    img = [torch.randn(map_shape, generator=g) * 3 for _ in range(6)]
    img[0].view(-1)[0], img[0].view(-1)[1] = 200.0, -200.0     # BCELoss's clamp, label 1
    img[3].view(-1)[2], img[3].view(-1)[4] = 200.0, -200.0     # and label 0
    ins = [torch.randn(256, 1, generator=g) * 2 for _ in range(2)]
    club = [torch.randn(G, 2, generator=g) * 2 for _ in range(6)]
    return img, [1, 1, 1, 0, 0, 0], ins, [256, 0], club, [1, 0, 1, 0, 1, 0]


@pytest.mark.parametrize("map_shape,G", [((1, 1, 3, 5), 1), ((2, 1, 20, 22), 8)])
def test_losses_against_the_fp64_composition(map_shape, G):
    from tlod.da import pa_atf
    img, il, ins, io, club, cl = _loss_case(map_shape, G, 11 + G)
    w = torch.randn(14, generator=torch.Generator().manual_seed(12)).double()
    ref_in = [t.double().requires_grad_(True) for t in img + ins + club]
    ref = pa_atf.losses_torch(ref_in[:6], il, ref_in[6:8], io, ref_in[8:], cl)
    (ref * w).sum().backward()
    dev_in = [t.to(dev).requires_grad_(True) for t in img + ins + club]
    got = pa_atf.losses(dev_in[:6], il, dev_in[6:8], io, dev_in[8:], cl)
    assert tuple(got.shape) == (14,) and got.dtype == torch.float32
    (got * w.float().to(dev)).sum().backward()
    rel = (got.detach().cpu().double() - ref.detach()).abs() / ref.detach().abs()
    print("loss terms", ref.detach().numpy().round(4), "rel err", float(rel.max()))
    assert float(rel.max()) <= 2e-5
    for t, (a, b) in enumerate(zip(dev_in, ref_in)):
        top = float(b.grad.abs().max())
        err = float((a.grad.cpu().double() - b.grad).abs().max())
        assert err <= 2e-5 * top, (t, err, top)
    assert float(dev_in[0].grad.view(-1)[1]) == 0.0 and float(dev_in[3].grad.view(-1)[2]) == 0.0
    # the broadcast instance term is the plain mean when the label is constant
    x = torch.sigmoid(ins[0].double())
    assert abs(float(ref[6].detach()) - float((1 - x).mean())) < 1e-12
    # twice the same bits
    again = pa_atf.losses([t.detach() for t in dev_in[:6]], il, [t.detach() for t in dev_in[6:8]],
                          io, [t.detach() for t in dev_in[8:]], cl)
    assert torch.equal(again, got.detach())


def test_losses_mixed_instance_labels_and_switch_off(monkeypatch):
    """R = 300 rows with 256 ones and 44 zeros: the (R, R) broadcast is not the plain mean."""
    from tlod.da import pa_atf
    img, il, ins, io, club, cl = _loss_case((1, 1, 3, 5), 3, 21)
    ins = [torch.randn(300, 1, generator=torch.Generator().manual_seed(22)) for _ in range(2)]
    io = [256, 44]
    args = ([t.to(dev) for t in img], il, [t.to(dev) for t in ins], io, [t.to(dev) for t in club], cl)
    got = pa_atf.losses(*args)
    ref = pa_atf.losses_torch([t.double() for t in img], il, [t.double() for t in ins], io,
                              [t.double() for t in club], cl)
    assert float(((got.cpu().double() - ref).abs() / ref.abs()).max()) <= 2e-5
    x = torch.sigmoid(ins[0].double())
    plain = torch.cat(((1 - x[:256]), x[256:])).mean()
    assert abs(float(ref[6]) - float(plain)) > 1e-3
    monkeypatch.setenv("TLOD_FUSED_PA_ATF", "0")
    off = pa_atf.losses(*args)
    # the fp32 composition saturates its sigmoid at |z| = 200 as the fp64 one does; below that
    # its log(1 - p) carries 2^-24 / (1 - p) relative error (1e-2 on one cell at z = 12 of these
    # 15-cell maps), so it is only held to 1e-3 of the fp64 terms
    assert float(((off.cpu().double() - ref).abs() / ref.abs()).max()) <= 1e-3


# ------------------------------------------------------------------ prototype pooling
def _proto_case(name):
    g = torch.Generator().manual_seed(len(name))
    if name == "one":
        C, H, W, scale = 5, 12, 14, 1 / 4
        rois = torch.tensor([[0, 6.0, 4.0, 44.0, 39.0]])
        perm = torch.tensor([0])
    elif name == "overlap":
        C, H, W, scale = 70, 9, 13, 1 / 8
        rois = torch.tensor([[0, 8.0, 8.0, 70.0, 60.0],      # overlaps the next one
                             [0, 30.0, 20.0, 130.0, 90.0],   # partly outside the 104 x 72 image
                             [0, 41.0, 33.0, 41.0, 33.0]])   # one pixel
        perm = torch.tensor([2, 0, 1])
    else:
        C, H, W, scale = 64, 10, 12, 1 / 16
        xy = torch.rand(8, 2, generator=g) * torch.tensor([120.0, 100.0])
        wh = torch.rand(8, 2, generator=g) * 70 + 4
        rois = torch.cat((torch.zeros(8, 1), xy, xy + wh), 1)
        perm = torch.tensor([3, 1, 0, 2, 7, 6, 5, 4])          # 1 is a fixed point
    feat = torch.randn(1, C, H, W, generator=g)
    mask = torch.rand(C, generator=g)
    return feat, rois, scale, mask, perm.to(torch.int32)


@pytest.mark.parametrize("name", ["one", "overlap", "shuffle"])
def test_proto_pool(name):
    from tlod.da import pa_atf
    from tlod.da.pa_atf import _ProtoPool
    feat, rois, scale, mask, perm = _proto_case(name)
    _, C, H, W = feat.shape
    G = rois.shape[0]
    alpha = 0.1
    fg = feat.to(dev).requires_grad_(True)
    same, diff, argmax = _ProtoPool.apply(fg, rois.to(dev), scale, mask.to(dev), perm.to(dev), alpha)
    ft = feat.to(dev).requires_grad_(True)
    s_t, d_t = pa_atf.proto_pool_torch(ft, rois.to(dev), scale, mask.to(dev), perm.to(dev), alpha)
    assert torch.equal(same, s_t) and torch.equal(diff, d_t)       # bit for bit
    assert int((argmax >= 0).sum()) > 0.5 * argmax.numel()
    if name == "overlap":
        assert int((argmax < 0).sum()) > 0                           # empty bins off the map
    gen = torch.Generator().manual_seed(9)
    gs, gd = torch.randn(same.shape, generator=gen), torch.randn(same.shape, generator=gen)
    (same * gs.to(dev)).sum().backward(retain_graph=True)
    first = fg.grad.clone()
    fg.grad = None
    ((same * gs.to(dev)).sum() + (diff * gd.to(dev)).sum()).backward()
    ((s_t * gs.to(dev)).sum() + (d_t * gd.to(dev)).sum()).backward()
    # fp64 through the same argmax
    m = mask.double().view(1, C, 1, 1)
    gs, gd = gs.double(), gd.double()
    dp = m * (gs[:, :C] + gd[:, :C]) + (1 - mask).double().view(1, C, 1, 1) * gs[:, C:]
    for g2 in range(G):
        dp[int(perm[g2])] += (1 - mask).double().view(C, 1, 1) * gd[g2, C:]
    am = argmax.cpu().numpy().reshape(-1)
    ref = np.zeros(C * H * W)
    np.add.at(ref, am[am >= 0], (-alpha * dp).numpy().reshape(-1)[am >= 0])
    got = fg.grad.cpu().double().numpy().reshape(-1)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{name}: dfeat rel err {err:.3e}, cells hit {int((ref != 0).sum())} of {ref.size}")
    assert err <= 1e-6
    assert np.array_equal(got != 0, ref != 0)
    assert float((ft.grad - fg.grad).abs().max()) <= 1e-5 * float(fg.grad.abs().max())
    assert not torch.equal(first, fg.grad)
    # twice the same bits
    f2 = feat.to(dev).requires_grad_(True)
    s2, d2, a2 = _ProtoPool.apply(f2, rois.to(dev), scale, mask.to(dev), perm.to(dev), alpha)
    ((s2 * gs.float().to(dev)).sum() + (d2 * gd.float().to(dev)).sum()).backward()
    assert torch.equal(s2, same) and torch.equal(d2, diff) and torch.equal(a2, argmax)
    assert torch.equal(f2.grad, fg.grad)


def test_proto_pool_switch_off_is_the_torch_composition(monkeypatch):
    from tlod.da import pa_atf
    feat, rois, scale, mask, perm = _proto_case("shuffle")
    args = (feat.to(dev), rois.to(dev), scale, mask.to(dev), perm.to(dev))
    s1, d1 = pa_atf.proto_pool(*args)
    monkeypatch.setenv("TLOD_FUSED_PA_ATF", "0")
    s0, d0 = pa_atf.proto_pool(*args)
    assert torch.equal(s0, s1) and torch.equal(d0, d1)


# ------------------------------------------------------------------ proposal subsampling
def _kept(counts, cap, seed):
    """Hand-made survivor lists: distinct boxes, zeros after each image's count."""
    g = torch.Generator().manual_seed(seed)
    kept = torch.zeros(len(counts), cap, 4)
    for b, n in enumerate(counts):
        kept[b, :n] = torch.rand(n, 4, generator=g) * 100 + 1 + b
    return kept, torch.tensor(counts, dtype=torch.int32)


#                                          below head / between    above post / exactly post
@pytest.mark.parametrize("counts,cap,post", [((3, 10), 64, 16), ((40, 16), 64, 16),
                                             ((5000, 300), 6000, 256), ((64, 65), 300, 256)])
def test_subsample_explicit_picks_and_device_rng(counts, cap, post):
    from tlod.rpn.proposal import proposal_pick, subsample_head, subsample_rule
    B, head = 2, subsample_head(post)
    assert head == post // 4
    kept, cnt = _kept(counts, cap, sum(counts))
    kd, cd = kept.to(dev), cnt.to(dev)
    # explicit picks: the restatement, exactly
    rs = np.random.RandomState(7)
    want = np.zeros((B, post, 5), np.float32)
    picks = []
    for b, n in enumerate(counts):
        rows, idx = subsample_rule(list(range(n)), post, rs.permutation)
        assert len(rows) == min(n, head) + min(max(n - head, 0), post - head)
        want[b, :, 0] = b
        want[b, :len(rows), 1:] = kept[b, rows].numpy()
        picks.append(idx)
    got = proposal_pick(kd, cd, post, pick=picks).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    # device RNG
    r1 = proposal_pick(kd, cd, post, seed=5).cpu().numpy()
    r1b = proposal_pick(kd, cd, post, seed=5).cpu().numpy()
    r2 = proposal_pick(kd, cd, post, seed=6).cpu().numpy()
    np.testing.assert_array_equal(r1, r1b)
    for b, n in enumerate(counts):
        nh, k = min(n, head), min(max(n - head, 0), post - head)
        for r in (r1, r2):
            assert (r[b, :, 0] == b).all()
            np.testing.assert_array_equal(r[b, :nh, 1:], kept[b, :nh].numpy())     # the head, exact
            assert (r[b, nh + k:, 1:] == 0).all()                                   # zero padded
            rest = {tuple(v) for v in kept[b, head:n].tolist()}
            drawn = [tuple(v) for v in r[b, nh:nh + k, 1:].tolist()]
            assert len(set(drawn)) == k and set(drawn) <= rest                      # distinct subset
            rank = {tuple(v): i for i, v in enumerate(kept[b, head:n].tolist())}
            order = [rank[d] for d in drawn]
            assert order == sorted(order)                                           # ascending rank
        if n - head > post - head:   # a real choice: another seed draws another subset
            assert not np.array_equal(r1[b], r2[b])
        else:
            np.testing.assert_array_equal(r1[b], r2[b])


def test_subsample_draw_is_uniform_enough():
    """Every survivor of the rest is drawn at the rate k / n: 400 seeds, n = 24, k = 6 — each
    count is Binomial(400, 1/4), mean 100, sd 8.7; 6 sd on either side."""
    from tlod.rpn.proposal import proposal_pick
    kept, cnt = _kept((26,), 32, 1)
    hits = np.zeros(26)
    for seed in range(400):
        r = proposal_pick(kept.to(dev), cnt.to(dev), 8, seed=seed).cpu().numpy()[0, 2:, 1:]
        for v in r:
            hits[int(np.flatnonzero((kept[0].numpy() == v).all(1))[0])] += 1
    assert hits[:2].sum() == 0 and hits[2:].sum() == 400 * 6
    assert hits[2:].min() > 100 - 52 and hits[2:].max() < 100 + 52


def test_proposal_keep_and_the_chained_entry():
    from helpers import rpn_outputs
    from oracle import rpn as orpn
    from oracle.boxes import generate_anchors
    from oracle.nms import nms as onms
    from tlod.rpn.proposal import proposal_keep, proposal_pick, proposal_subsample
    base = generate_anchors(scales=np.array([4, 8, 16, 32]), ratios=np.array([0.5, 1, 2]))
    base = np.ascontiguousarray(base, np.float32)
    B, A, H, W, pre, thr = 2, base.shape[0], 20, 22, 3000, 0.7
    rng = np.random.default_rng(3)
    prob, deltas = rpn_outputs(rng, B, A, H, W, delta_scale=0.0)     # exp(0) = 1: decode exact
    im_info = np.array([[320, 352, 1.0], [300, 340, 1.0]], np.float32)
    t = lambda x: torch.from_numpy(x).to(dev)
    kept, counts = proposal_keep(t(prob), t(deltas), t(im_info), t(base), 16, pre, thr)
    assert tuple(kept.shape) == (B, pre, 4)
    ref = orpn.proposal_layer(prob, deltas, im_info, base, 16, pre, pre, thr)
    np.testing.assert_array_equal(kept.cpu().numpy(), ref[:, :, 1:])
    scores, props = orpn.decode_clip(prob, deltas, im_info, base, 16)
    for b in range(B):
        order = np.argsort(-scores[b], kind="stable")[:pre]
        keep = onms(np.concatenate([props[b][order], scores[b][order, None]], 1), thr)
        assert int(counts[b]) == len(keep) > 256          # the random part is exercised
    two = proposal_pick(kept, counts, 256, seed=11)
    one = proposal_subsample(t(prob), t(deltas), t(im_info), t(base), 16, pre, 256, thr, seed=11)
    assert torch.equal(one, two)
    assert int((one[:, :, 1:].abs().sum(2) > 0).sum()) == 2 * 256
