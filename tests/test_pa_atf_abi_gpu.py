"""Guard bands and poisoned outputs around the PA-ATF extension of the C ABI
(include/tlod_pa_atf.h), with tests/abi_guard.Call as it is: every output starts as poison and
must be fully written, every input must be bit-equal afterwards, no guard byte may change, and
a call with a bad shape is refused before anything is launched (pure poison left).  Values are
checked against torch on the CPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from abi_guard import Call

pytestmark = pytest.mark.gpu
f32, i32 = torch.float32, torch.int32
TLOD_EINVAL = -1


def lib():
    from tlod import _lib
    return _lib.lib()


def _ok(st, what=""):
    assert st == 0, (what, st, lib().tlod_last_error().decode(errors="replace"))


#                                    N  C   H   W  KS s  p
@pytest.mark.parametrize("shape", [(2, 24, 23, 31, 5, 3, 0), (1, 16, 9, 11, 3, 2, 1),
                                   (3, 5, 3, 3, 3, 2, 0), (1, 300, 7, 7, 3, 2, 0)])
def test_im2col_and_col2im(shape):
    L = lib()
    N, C, H, W, KS, s, p = shape
    Ho, Wo = (H + 2 * p - KS) // s + 1, (W + 2 * p - KS) // s + 1
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(N, C, H, W, generator=g)
    c = Call()
    col = c.out((N * Ho * Wo, C * KS * KS), f32, "col")
    _ok(c.run(L.tlod_im2col_f32, c.inp(x, "x"), N, C, H, W, KS, s, p, col))
    c.check()
    want = F.unfold(x, KS, padding=p, stride=s).transpose(1, 2).reshape(N * Ho * Wo, -1)
    assert torch.equal(col.payload.cpu(), want)

    dcol = torch.rand(N * Ho * Wo, C * KS * KS, generator=g) + 0.5
    c = Call()
    dx = c.out((N, C, H, W), f32, "dx")
    _ok(c.run(L.tlod_col2im_f32, c.inp(dcol, "dcol"), N, C, H, W, KS, s, p, dx))
    c.check()                                    # the uncovered cells are written too (0)
    fold = F.fold(dcol.double().view(N, Ho * Wo, -1).transpose(1, 2), (H, W), KS, padding=p,
                  stride=s)
    assert float((dx.payload.cpu().double() - fold).abs().max()) <= 1e-6 * float(fold.max())

    for bad in ((N, C, H, W, 0, s, p), (N, C, H, W, KS, 0, p), (N, C, KS - 1, W, KS, s, 0),
                (N, C, H, W, KS, s, -1)):
        c = Call()
        col = c.out((N * Ho * Wo, C * KS * KS), f32, "col")
        assert c.run(L.tlod_im2col_f32, c.inp(x, "x"), *bad, col) == TLOD_EINVAL
        c.check_rejected()
        c = Call()
        dx = c.out((N, C, H, W), f32, "dx")
        assert c.run(L.tlod_col2im_f32, c.inp(dcol, "dcol"), *bad, dx) == TLOD_EINVAL
        c.check_rejected()


@pytest.mark.parametrize("shape", [(1, 5, 1, 1), (2, 70, 3, 6), (1, 257, 11, 24)])
def test_gate_and_backward(shape):
    L = lib()
    N, C, h, w = shape
    g = torch.Generator().manual_seed(sum(shape))
    z = torch.randn(shape, generator=g)
    c = Call()
    mask, arg = c.out((N, C), f32, "mask"), c.out((N, C), i32, "arg")
    _ok(c.run(L.tlod_pa_gate_f32, c.inp(z, "z"), N, C, h, w, mask, arg))
    c.check()
    mx, am = F.adaptive_max_pool2d(z, 1, return_indices=True)
    assert torch.equal(arg.payload.cpu().long(), am.view(N, C))
    ref = torch.sigmoid(mx.double()).view(N, C)
    assert float((mask.payload.cpu().double() - ref).abs().max()) <= 2.0 ** -24

    dmask = torch.randn(N, C, generator=g)
    m = mask.payload.cpu().clone()
    c = Call()
    dz = c.out(shape, f32, "dz")
    _ok(c.run(L.tlod_pa_gate_bwd_f32, c.inp(dmask, "dmask"), c.inp(m, "mask"),
              c.inp(am.view(N, C).to(i32), "arg"), N, C, h, w, dz))
    c.check()
    want = torch.zeros(N * C, h * w)
    want[torch.arange(N * C), am.view(-1)] = torch.ops.aten.sigmoid_backward(dmask, m).view(-1)
    assert torch.equal(dz.payload.cpu().view(N * C, -1), want)

    c = Call()
    mask, arg = c.out((N, C), f32, "mask"), c.out((N, C), i32, "arg")
    assert c.run(L.tlod_pa_gate_f32, c.inp(z, "z"), N, C, 0, w, mask, arg) == TLOD_EINVAL
    c.check_rejected()
    c = Call()
    dz = c.out(shape, f32, "dz")
    assert c.run(L.tlod_pa_gate_bwd_f32, c.inp(dmask, "dmask"), c.inp(m, "mask"),
                 c.inp(am.view(N, C).to(i32), "arg"), N, 0, h, w, dz) == TLOD_EINVAL
    c.check_rejected()


@pytest.mark.parametrize("C,H,W,G,scale", [(5, 12, 14, 1, 0.25), (70, 9, 13, 3, 0.125),
                                           (64, 10, 12, 8, 0.0625)])
def test_proto_pool_and_backward(C, H, W, G, scale):
    from oracle import roi as oroi
    L = lib()
    g = torch.Generator().manual_seed(C + G)
    feat = torch.randn(1, C, H, W, generator=g)
    xy = torch.rand(G, 2, generator=g) * torch.tensor([W / scale * 0.8, H / scale * 0.8])
    wh = torch.rand(G, 2, generator=g) * torch.tensor([W / scale * 0.6, H / scale * 0.6])
    rois = torch.cat((torch.zeros(G, 1), xy, xy + wh), 1)
    mask = torch.rand(C, generator=g)
    perm = torch.randperm(G, generator=g).to(i32)
    c = Call()
    same, diff = c.out((G, 2 * C, 7, 7), f32, "same"), c.out((G, 2 * C, 7, 7), f32, "diff")
    argmax = c.out((G, C, 7, 7), i32, "argmax")
    _ok(c.run(L.tlod_pa_proto_pool_fwd_f32, c.inp(feat, "feat"), C, H, W, c.inp(rois, "rois"), G,
              scale, c.inp(mask, "mask"), c.inp(perm, "perm"), same, diff, argmax))
    c.check()
    p, am = oroi.roi_pool_fwd(feat.numpy(), rois.numpy(), 7, 7, scale)
    p, m = torch.from_numpy(p), mask.view(1, C, 1, 1)
    np.testing.assert_array_equal(argmax.payload.cpu().numpy(), am)
    assert torch.equal(same.payload.cpu(), torch.cat((p * m, p * (1 - m)), 1))
    assert torch.equal(diff.payload.cpu(), torch.cat((p * m, p[perm.long()] * (1 - m)), 1))

    gs, gd = torch.randn(G, 2 * C, 7, 7, generator=g), torch.randn(G, 2 * C, 7, 7, generator=g)
    c = Call()
    dfeat = c.out((1, C, H, W), f32, "dfeat")
    _ok(c.run(L.tlod_pa_proto_pool_bwd_f32, c.inp(gs, "d_same"), c.inp(gd, "d_diff"),
              c.inp(mask, "mask"), c.inp(perm, "perm"), c.inp(torch.from_numpy(am), "argmax"),
              c.inp(rois, "rois"), G, scale, C, H, W, 0.1, dfeat))
    c.check()
    md, cm = mask.double().view(1, C, 1, 1), (1 - mask).double().view(1, C, 1, 1)
    dp = md * (gs[:, :C].double() + gd[:, :C].double()) + cm * gs[:, C:].double()
    for g2 in range(G):
        dp[int(perm[g2])] += cm[0] * gd[g2, C:].double()
    ref = np.zeros(C * H * W)
    flat = am.reshape(-1)
    np.add.at(ref, flat[flat >= 0], (-0.1 * dp).numpy().reshape(-1)[flat >= 0])
    got = dfeat.payload.cpu().double().numpy().reshape(-1)
    assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max()

    c = Call()
    same, diff = c.out((G, 2 * C, 7, 7), f32, "same"), c.out((G, 2 * C, 7, 7), f32, "diff")
    argmax = c.out((G, C, 7, 7), i32, "argmax")
    st = c.run(L.tlod_pa_proto_pool_fwd_f32, c.inp(feat, "feat"), C, H, W, c.inp(rois, "rois"), 0,
               scale, c.inp(mask, "mask"), c.inp(perm, "perm"), same, diff, argmax)
    assert st == TLOD_EINVAL
    c.check_rejected()
    c = Call()
    dfeat = c.out((1, C, H, W), f32, "dfeat")
    st = c.run(L.tlod_pa_proto_pool_bwd_f32, c.inp(gs, "d_same"), c.inp(gd, "d_diff"),
               c.inp(mask, "mask"), c.inp(perm, "perm"), c.inp(torch.from_numpy(am), "argmax"),
               c.inp(rois, "rois"), G, scale, 0, H, W, 0.1, dfeat)
    assert st == TLOD_EINVAL
    c.check_rejected()


def _tables(bufs):
    import ctypes
    return (ctypes.c_void_p * len(bufs))(*[b.ptr.value for b in bufs])


@pytest.mark.parametrize("cells,R,G", [(15, 256, 1), (880, 300, 8)])
def test_losses_and_backward(cells, R, G):
    import ctypes
    from tlod.da import pa_atf
    L = lib()
    g = torch.Generator().manual_seed(cells + G)
    z = [torch.randn(cells, generator=g) * 3 for _ in range(6)]
    z[1][0], z[4][0] = -200.0, 200.0                     # BCELoss's clamp on both labels
    z += [torch.randn(R, generator=g) * 2 for _ in range(2)]
    z += [torch.randn(G, 2, generator=g) * 2 for _ in range(6)]
    n = [cells] * 6 + [R] * 2 + [G] * 6
    label = [1, 1, 1, 0, 0, 0, R, R - 256, 1, 0, 1, 0, 1, 0]
    nt, lt = (ctypes.c_int * 14)(*n), (ctypes.c_int * 14)(*label)
    zd = [t.double().requires_grad_(True) for t in z]
    ref = pa_atf.losses_torch(zd[:6], label[:6], zd[6:8], label[6:8], zd[8:], label[8:])
    g_loss = torch.randn(14, generator=g)
    (ref * g_loss.double()).sum().backward()

    c = Call()
    ins = [c.inp(t, f"z{i}") for i, t in enumerate(z)]
    loss = c.out((14,), f32, "loss")
    _ok(c.run(L.tlod_pa_atf_loss_f32, _tables(ins), nt, lt, loss))
    c.check()
    got = loss.payload.cpu().double()
    assert float(((got - ref.detach()).abs() / ref.detach().abs()).max()) <= 2e-5

    c = Call()
    ins = [c.inp(t, f"z{i}") for i, t in enumerate(z)]
    dz = [c.out(t.shape, f32, f"dz{i}") for i, t in enumerate(z)]
    _ok(c.run(L.tlod_pa_atf_loss_bwd_f32, _tables(ins), nt, lt, c.inp(g_loss, "g_loss"),
              _tables(dz)))
    c.check()
    for t in range(14):
        top = float(zd[t].grad.abs().max())
        assert float((dz[t].payload.cpu().double() - zd[t].grad).abs().max()) <= 2e-5 * top, t
    assert float(dz[1].payload[0]) == 0.0 and float(dz[4].payload[0]) == 0.0

    # a label outside its range, an empty term and a repeated gradient buffer are refused
    for bad_n, bad_l in (([0] + n[1:], label), (n, [2] + label[1:]),
                         (n, label[:6] + [R + 1] + label[7:])):
        c = Call()
        ins = [c.inp(t, f"z{i}") for i, t in enumerate(z)]
        loss = c.out((14,), f32, "loss")
        st = c.run(L.tlod_pa_atf_loss_f32, _tables(ins), (ctypes.c_int * 14)(*bad_n),
                   (ctypes.c_int * 14)(*bad_l), loss)
        assert st == TLOD_EINVAL
        c.check_rejected()
    c = Call()
    ins = [c.inp(t, f"z{i}") for i, t in enumerate(z)]
    dz = [c.out(t.shape, f32, f"dz{i}") for i, t in enumerate(z)]
    st = c.run(L.tlod_pa_atf_loss_bwd_f32, _tables(ins), nt, lt, c.inp(g_loss, "g_loss"),
               _tables(dz[:13] + dz[:1]))
    assert st == TLOD_EINVAL
    c.check_rejected()


# ------------------------------------------------------------------ proposal subsampling
TLOD_EWORKSPACE, TLOD_EUNSUPPORTED = -3, -4


def _rpn_case(pre):
    from helpers import rpn_outputs
    from oracle.boxes import generate_anchors
    base = generate_anchors(scales=np.array([4, 8, 16, 32]), ratios=np.array([0.5, 1, 2]))
    base = np.ascontiguousarray(base, np.float32)
    B, A, H, W = 2, base.shape[0], 5, 7
    prob, deltas = rpn_outputs(np.random.default_rng(pre), B, A, H, W, delta_scale=0.0)
    im_info = np.array([[H * 16, W * 16, 1.0], [H * 16 - 9, W * 16 - 20, 1.0]], np.float32)
    return [torch.from_numpy(x) for x in (prob, deltas, im_info, base)], (B, A, H, W)


@pytest.mark.parametrize("pre", [100, 2000])     # < N = 420 <
def test_proposal_keep(pre):
    from oracle import rpn as orpn
    L = lib()
    ins, (B, A, H, W) = _rpn_case(pre)
    cap = min(pre, A * H * W)
    ref = orpn.proposal_layer(*[x.numpy() for x in ins], 16, pre, cap, 0.7)
    q = L.tlod_proposal_workspace_bytes(B, A, H, W, pre)
    for over, want in ((q, 0), (q - 1, TLOD_EWORKSPACE)):
        c = Call()
        kept, counts = c.out((B, cap, 4), f32, "kept"), c.out((B,), i32, "counts")
        st = c.run(L.tlod_proposal_keep_f32, *[c.inp(x, f"in{i}") for i, x in enumerate(ins)],
                   B, A, H, W, 16, pre, 0.7, kept, counts, c.ws(q).ptr, over)
        assert st == want, (st, lib().tlod_last_error())
        if want:
            c.check_rejected()
            continue
        c.check()                                  # the rows past the survivors are written: 0
        np.testing.assert_array_equal(kept.payload.cpu().numpy(), ref[:, :, 1:])
        n = counts.payload.cpu().numpy()
        assert (n > 0).all() and (n <= cap).all()
        for b in range(B):
            assert (ref[b, :n[b], 1:].sum(1) > 0).all() and (ref[b, n[b]:, 1:] == 0).all()


@pytest.mark.parametrize("explicit", [False, True])
def test_proposal_pick(explicit):
    L = lib()
    B, cap, post, head = 2, 40, 16, 4
    g = torch.Generator().manual_seed(8)
    kept = torch.rand(B, cap, 4, generator=g) + 1
    counts = torch.tensor([30, 3], dtype=i32)
    kept[0, 30:], kept[1, 3:] = 0, 0
    pick = torch.tensor([5, 0, 25, 7, 99], dtype=i32)          # 99: out of range, a zero row
    off = torch.tensor([0, 5, 5], dtype=i32)

    def run(c, post_, head_, cap_=cap):
        rois = c.out((B, post, 5), f32, "rois")
        st = c.run(L.tlod_proposal_pick_f32, c.inp(kept, "kept"), c.inp(counts, "counts"), B, cap_,
                   post_, head_, c.inp(pick, "pick") if explicit else None,
                   c.inp(off, "pick_off") if explicit else None, 3, rois)
        return st, rois

    c = Call()
    st, rois = run(c, post, head)
    _ok(st)
    c.check()                                                   # padding and column 0 included
    r = rois.payload.cpu()
    assert (r[0, :, 0] == 0).all() and (r[1, :, 0] == 1).all()
    assert torch.equal(r[0, :4, 1:], kept[0, :4]) and torch.equal(r[1, :3, 1:], kept[1, :3])
    assert (r[1, 3:, 1:] == 0).all()
    if explicit:
        assert torch.equal(r[0, 4:8, 1:], kept[0, [9, 4, 29, 11]])
        assert (r[0, 8:, 1:] == 0).all()
    else:
        assert (r[0, 4:, 1:].sum(1) > 0).all()                  # 12 of the 26 others
    for args, want in (((post, post + 1), TLOD_EINVAL), ((post, -1), TLOD_EINVAL),
                       ((0, 0), TLOD_EINVAL), ((post, head, 16385), TLOD_EUNSUPPORTED)):
        c = Call()
        st, _ = run(c, *args)
        assert st == want
        c.check_rejected()
    if explicit:                                                # pick without pick_off
        c = Call()
        rois = c.out((B, post, 5), f32, "rois")
        st = c.run(L.tlod_proposal_pick_f32, c.inp(kept, "kept"), c.inp(counts, "counts"), B, cap,
                   post, head, c.inp(pick, "pick"), None, 3, rois)
        assert st == TLOD_EINVAL
        c.check_rejected()


def test_proposal_subsample():
    L = lib()
    pre, post, head = 2000, 64, 16
    ins, (B, A, H, W) = _rpn_case(pre)
    q = L.tlod_proposal_subsample_workspace_bytes(B, A, H, W, pre)
    assert q > L.tlod_proposal_workspace_bytes(B, A, H, W, pre)
    assert L.tlod_proposal_subsample_workspace_bytes(0, A, H, W, pre) == 0
    outs = []
    for over, want in ((q, 0), (q, 0), (q - 1, TLOD_EWORKSPACE)):
        c = Call()
        rois = c.out((B, post, 5), f32, "rois")
        st = c.run(L.tlod_proposal_subsample_f32, *[c.inp(x, f"in{i}") for i, x in enumerate(ins)],
                   B, A, H, W, 16, pre, post, head, 0.7, 21, rois, c.ws(q).ptr, over)
        assert st == want, (st, lib().tlod_last_error())
        if want:
            c.check_rejected()
        else:
            c.check()
            outs.append(rois.payload.cpu().clone())
    assert torch.equal(outs[0], outs[1])                        # one seed, one draw
    from tlod.rpn.proposal import proposal_keep
    _, counts = proposal_keep(*[x.cuda() for x in ins], 16, pre, 0.7)
    for b in range(B):                                          # the row count of the rule
        n = int(counts[b])
        rows = min(n, head) + min(max(n - head, 0), post - head)
        assert int((outs[0][b, :, 1:].sum(1) > 0).sum()) == rows and n > head
    c = Call()
    rois = c.out((B, post, 5), f32, "rois")
    st = c.run(L.tlod_proposal_subsample_f32, *[c.inp(x, f"in{i}") for i, x in enumerate(ins)],
               B, A, H, W, 16, pre, post, post + 1, 0.7, 21, rois, c.ws(q).ptr, q)
    assert st == TLOD_EINVAL
    c.check_rejected()
