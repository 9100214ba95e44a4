"""Guard bands and poisoned outputs around the IDF extension of the C ABI (include/tlod_idf.h),
with tests/abi_guard.Call as it is: every output starts as poison and must be fully written,
every input must be bit-equal afterwards, no guard byte may change, the workspace is exactly
the queried size, one byte less is refused before anything is launched (pure poison left), and
so is an inconsistent NULL form.  The NULL-argument forms the header allows are run too.
Values are checked against tests/ref_idf.py in fp64."""
import numpy as np
import pytest
import torch

import ref_idf
from abi_guard import TLOD_EWORKSPACE, Call

pytestmark = pytest.mark.gpu
f32 = torch.float32
TLOD_EINVAL = -1


def lib():
    from tlod import _lib
    return _lib.lib()


def _ok(st, what=""):
    assert st == 0, (what, st, lib().tlod_last_error().decode(errors="replace"))


def _ws(c, q, over):
    ws = c.ws(q)
    return (ws.ptr if ws is not None else None), (q if over is None else over)


def guard_case(launch, verify):
    """launch(c, over) -> (status, query, outputs): the full call with an exact workspace,
    then (when it has one) the same call claiming one byte less."""
    c = Call()
    st, q, outs = launch(c, None)
    _ok(st, launch.__name__)
    c.check()
    assert verify(outs) is None
    if q > 0:
        c2 = Call()
        st2, q2, _ = launch(c2, q - 1)
        assert q2 == q and st2 == TLOD_EWORKSPACE, (launch.__name__, st2, q)
        c2.check_rejected()
    return q


def _maps(N, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(N, C, H, W, generator=g)
    b = a + 0.5 * torch.randn(N, C, H, W, generator=g)
    return a, b


def _close(got, ref, rtol):
    got, ref = got.double().cpu(), ref.double().cpu()
    err = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
    assert err <= rtol, err


@pytest.mark.parametrize("shape", [(1, 24, 5, 7), (2, 512, 37, 75)])
def test_dam(shape):
    L = lib()
    N, C, H, W = shape
    x = _maps(N, C, H, W, 1)[0]
    avg, thr = ref_idf.dam_parts(x.double())
    ref = ref_idf.dam(x.double())[:, 0]

    def launch(c, over):
        q = L.tlod_idf_dam_workspace_bytes(N, H, W)
        att = c.out((N, H, W), f32, "att")
        st = c.run(L.tlod_idf_dam_f32, c.inp(x, "x"), N, C, H, W, att, *_ws(c, q, over))
        return st, q, (att,)

    def verify(o):
        got = o[0].payload.cpu().double()
        diff = (got > 0) != (ref > 0)
        assert int(diff.sum()) <= 0.01 * diff.numel()
        assert (((avg - thr).abs() <= 1e-5 * thr)[:, 0][diff]).all()
        on = (got > 0) & (ref > 0)
        assert int(on.sum()) > 0.2 * on.numel()
        assert ((got - ref).abs()[on] <= 1e-6 * ref[on]).all()
    assert guard_case(launch, verify) > 0


@pytest.mark.parametrize("shape", [(1, 24, 5, 7), (2, 512, 37, 75)])
def test_sep_fwd_with_modulation(shape):
    L = lib()
    N, C, H, W = shape
    a, b = _maps(N, C, H, W, 2)
    att_a, att_b = ref_idf.dam(a), ref_idf.dam(b)

    def launch(c, over):
        q = L.tlod_idf_sep_fwd_workspace_bytes(N, H, W)
        outs = (c.out(shape, f32, "a_out"), c.out(shape, f32, "b_out"),
                c.out((N, H, W), f32, "d"), c.out((N,), f32, "dist"))
        st = c.run(L.tlod_idf_sep_fwd_f32, c.inp(a, "a"), c.inp(b, "b"),
                   c.inp(att_a[:, 0], "att_a"), c.inp(att_b[:, 0], "att_b"), N, C, H, W, *outs,
                   *_ws(c, q, over))
        return st, q, outs

    def verify(o):
        ra, rb = ref_idf.modulate(a, b, att_a, att_b)
        assert torch.equal(o[0].payload.cpu(), ra) and torch.equal(o[1].payload.cpu(), rb)
        e = (a.double() - b.double()) * att_b.double() + 1e-6
        _close(o[2].payload, e.norm(2, dim=1), 1e-6)
        _close(o[3].payload, ref_idf.distance(a.double(), b.double(), att_b.double()), 1e-6)
    assert guard_case(launch, verify) > 0


def test_sep_fwd_null_forms():
    """att_b NULL = weight 1 and no modulation outputs (dist1); a modulation without its
    attention maps, or with one output only, is refused before any launch."""
    L = lib()
    N, C, H, W = 1, 256, 12, 20
    a, b = _maps(N, C, H, W, 3)
    q = L.tlod_idf_sep_fwd_workspace_bytes(N, H, W)

    c = Call()
    d, dist = c.out((N, H, W), f32, "d"), c.out((N,), f32, "dist")
    _ok(c.run(L.tlod_idf_sep_fwd_f32, c.inp(a, "a"), c.inp(b, "b"), None, None, N, C, H, W, None,
              None, d, dist, *_ws(c, q, None)))
    c.check()
    _close(d.payload, (a.double() - b.double() + 1e-6).norm(2, dim=1), 1e-6)
    _close(dist.payload, ref_idf.distance(a.double(), b.double()), 1e-6)

    for give_att, both in ((False, True), (True, False)):
        c = Call()
        att = c.inp(torch.rand(N, H, W), "att") if give_att else None
        a_out, b_out = c.out(a.shape, f32, "a_out"), c.out(a.shape, f32, "b_out")
        d, dist = c.out((N, H, W), f32, "d"), c.out((N,), f32, "dist")
        st = c.run(L.tlod_idf_sep_fwd_f32, c.inp(a, "a"), c.inp(b, "b"), att, att, N, C, H, W,
                   a_out, b_out if both else None, d, dist, *_ws(c, q, None))
        assert st == TLOD_EINVAL
        c.check_rejected()


@pytest.mark.parametrize("shape", [(1, 24, 5, 7), (2, 512, 37, 75)])
def test_sep_bwd(shape):
    L = lib()
    N, C, H, W = shape
    a, b = _maps(N, C, H, W, 4)
    att_a, att_b = ref_idf.dam(a), ref_idf.dam(b)
    g = torch.Generator().manual_seed(5)
    ga_out, gb_out = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    g_dist = torch.randn(N, generator=g)
    e = (a.double() - b.double()) * att_b.double() + 1e-6
    d64 = e.norm(2, dim=1, keepdim=True)
    t = g_dist.double().view(N, 1, 1, 1) / (H * W) * att_b.double() * e / d64

    c = Call()
    g_a, g_b = c.out(shape, f32, "g_a"), c.out(shape, f32, "g_b")
    _ok(c.run(L.tlod_idf_sep_bwd_f32, c.inp(a, "a"), c.inp(b, "b"), c.inp(att_a[:, 0], "att_a"),
              c.inp(att_b[:, 0], "att_b"), c.inp(d64[:, 0].float(), "d"), c.inp(ga_out, "g_a_out"),
              c.inp(gb_out, "g_b_out"), c.inp(g_dist, "g_dist"), N, C, H, W, g_a, g_b))
    c.check()
    _close(g_a.payload, ga_out.double() * (1 + att_b.double()) + t, 1e-6)
    _close(g_b.payload, gb_out.double() * (1 + att_a.double()) - t, 1e-6)

    # NULL g_*_out: the distance term alone; att_a is then unused and may be NULL
    c = Call()
    g_a, g_b = c.out(shape, f32, "g_a"), c.out(shape, f32, "g_b")
    _ok(c.run(L.tlod_idf_sep_bwd_f32, c.inp(a, "a"), c.inp(b, "b"), None,
              c.inp(att_b[:, 0], "att_b"), c.inp(d64[:, 0].float(), "d"), None, None,
              c.inp(g_dist, "g_dist"), N, C, H, W, g_a, g_b))
    c.check()
    _close(g_a.payload, t, 1e-6)
    assert torch.equal(g_a.payload, -g_b.payload)

    # one upstream gradient without the other: refused, nothing written
    c = Call()
    g_a, g_b = c.out(shape, f32, "g_a"), c.out(shape, f32, "g_b")
    st = c.run(L.tlod_idf_sep_bwd_f32, c.inp(a, "a"), c.inp(b, "b"), c.inp(att_a[:, 0], "att_a"),
               c.inp(att_b[:, 0], "att_b"), c.inp(d64[:, 0].float(), "d"), c.inp(ga_out, "g_a_out"),
               None, c.inp(g_dist, "g_dist"), N, C, H, W, g_a, g_b)
    assert st == TLOD_EINVAL
    c.check_rejected()


@pytest.mark.parametrize("n_img,R,label", [(6, 256, 0), (6, 300, 1), (0, 5, 1)])
def test_domain_loss_and_backward(n_img, R, label):
    L = lib()
    g = torch.Generator().manual_seed(6 + R)
    z_img = torch.randn(n_img, 2, generator=g) * 2
    z_ins = torch.randn(R, 2, generator=g) * 3
    z_ins[1] = torch.tensor([18.0, -2.0]) if label == 1 else torch.tensor([-2.0, 18.0])  # clamped
    g_loss = torch.randn(n_img + 1, generator=g)
    zi, zn = z_img.double().requires_grad_(True), z_ins.double().requires_grad_(True)
    terms = [ref_idf.cross_entropy2(zi[i:i + 1], label) for i in range(n_img)]
    terms.append(ref_idf.focal_loss(zn, label, 3.0))
    ref = torch.stack(terms)
    (ref * g_loss.double()).sum().backward()

    c = Call()
    loss = c.out((n_img + 1,), f32, "loss")
    _ok(c.run(L.tlod_idf_domain_loss_f32, c.inp(z_img, "z_img") if n_img else None, n_img, label,
              c.inp(z_ins, "z_ins"), R, label, 3.0, loss))
    c.check()
    _close(loss.payload, ref.detach(), 2e-5)

    c = Call()
    dz_img = c.out((n_img, 2), f32, "dz_img") if n_img else None
    dz_ins = c.out((R, 2), f32, "dz_ins")
    _ok(c.run(L.tlod_idf_domain_loss_bwd_f32, c.inp(z_img, "z_img") if n_img else None, n_img,
              label, c.inp(z_ins, "z_ins"), R, label, 3.0, c.inp(g_loss, "g_loss"), dz_img, dz_ins))
    c.check()
    if n_img:
        _close(dz_img.payload, zi.grad, 2e-5)
    _close(dz_ins.payload, zn.grad, 2e-5)
    assert torch.count_nonzero(dz_ins.payload[1]).item() == 0

    # a label outside {0, 1} is refused before any launch
    c = Call()
    loss = c.out((n_img + 1,), f32, "loss")
    st = c.run(L.tlod_idf_domain_loss_f32, c.inp(z_img, "z_img") if n_img else None, n_img, 2,
               c.inp(z_ins, "z_ins"), R, label, 3.0, loss)
    assert st == TLOD_EINVAL
    c.check_rejected()
    c = Call()
    dz_ins = c.out((R, 2), f32, "dz_ins")
    st = c.run(L.tlod_idf_domain_loss_bwd_f32, None, 0, label, c.inp(z_ins, "z_ins"), R, 3, 3.0,
               c.inp(g_loss[-1:], "g_loss"), None, dz_ins)
    assert st == TLOD_EINVAL
    c.check_rejected()
