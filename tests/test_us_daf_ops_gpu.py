"""The US-DAF kernels alone (csrc/us_daf.hip through tlod.da.us_daf) against the CPU
restatement (tests/ref_us_daf.py).

Labels: bit-exact against the literal Python loop.  Losses: the returned fp32 sigmoid within
2 ulp of CPU torch.sigmoid; losses and logit gradients against the fp64 torch composition
evaluated from that returned fp32 s at test_losses_gpu.close (rtol 2e-5); gates bit-identical
to that composition's (inputs keep every column-0 element loss at least 1e-4 from 0.5)."""
import math

import numpy as np
import pytest
import torch

from ref_us_daf import PLANTED_LABELS, da_losses_from_sigmoid, planted_rois, scale_labels
from test_losses_gpu import close

pytestmark = pytest.mark.gpu
dev = "cuda"

MAPS = [(1, 1, 1), (2, 5, 7), (1, 12, 20), (1, 37, 75)]
ROWS = [(1, 1), (3, 5), (256, 300), (128, 300)]
G = (0.7, 1.3, -0.4, 2.0)  # upstream gradients of the four losses


@pytest.mark.parametrize("R", [1, 3, 256, 300])
def test_scale_labels_bit_exact(R, monkeypatch):
    from tlod.da.us_daf import roi_scale_labels
    r = planted_rois(R, seed=R)
    want = scale_labels(r)
    assert want[:len(PLANTED_LABELS)].tolist() == PLANTED_LABELS[:R]
    got = roi_scale_labels(torch.from_numpy(r).to(dev).view(1, R, 5))
    assert got.shape == (R, 3) and torch.equal(got.cpu(), want)
    monkeypatch.setenv("TLOD_FUSED_LOSSES", "0")
    assert torch.equal(roi_scale_labels(torch.from_numpy(r).to(dev)).cpu(), want)


def _col0_loss(z0, y):
    s = torch.sigmoid(z0.double())
    return -(y * torch.log(s + 1e-10) + (1 - y) * torch.log(1 - s + 1e-10))


def _inputs(shape_s, shape_t, n_s, n_t, seed):
    """Image logits, instance logits (column 0 kept 1e-3 away from the gate threshold in loss
    units) and planted RoIs of both domains, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    z_img = [torch.randn(B, 1, H, W, generator=g) * 2 for B, H, W in (shape_s, shape_t)]
    z_ins, rois = [], []
    for k, (n, y) in enumerate(((n_s, 1.0), (n_t, 0.0))):
        z = torch.randn(n, 4, generator=g) * 1.5
        near = (_col0_loss(z[:, 0], y) - 0.5).abs() < 1e-3
        z[near, 0] += 0.25 if y == 1.0 else -0.25  # deeper into the gated-off side
        z_ins.append(z)
        rois.append(torch.from_numpy(planted_rois(n, seed=seed + k)))
    return z_img, z_ins, rois


def _ulp_diff(a, b):
    return (a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()) \
        .abs().max().item()


def _reference(s_img, s_ins, rois, gates=None):
    """fp64 composition from the returned fp32 s: the four losses, dL/dz of sum G_k L_k for the
    four logit tensors, own gates, column-0 element losses."""
    losses, dz_img, dz_ins, own, col0 = [], [], [], [], []
    for k, y in enumerate((1.0, 0.0)):
        si = s_img[k].detach().cpu().double().requires_grad_(True)
        sn = s_ins[k].detach().cpu().double().requires_grad_(True)
        img, ins, gate, c0 = da_losses_from_sigmoid(si, y, sn, rois[k].numpy(),
                                                    None if gates is None else gates[k].cpu())
        (G[2 * k] * img + G[2 * k + 1] * ins).backward()
        losses += [img.detach(), ins.detach()]
        dz_img.append(si.grad * (si * (1 - si)).detach())
        dz_ins.append(sn.grad * (sn * (1 - sn)).detach())
        own.append(gate)
        col0.append(c0)
    return losses, dz_img, dz_ins, own, col0


def _run(z_img, z_ins, rois, packed, gate_override=None):
    """The device run: ((4 losses), s (4), gates (2), logit gradients (img_s, img_t, ins_s,
    ins_t))."""
    from tlod.da.us_daf import us_daf_da_losses, us_daf_da_losses_packed
    r = [x.to(dev) for x in rois]
    if packed:
        Bs, n_s = z_img[0].shape[0], z_ins[0].shape[0]
        zi = torch.cat(z_img, 0).to(dev).requires_grad_(True)
        zn = torch.cat(z_ins, 0).to(dev).requires_grad_(True)
        losses, s, gates = us_daf_da_losses_packed(zi, zn, torch.cat(r, 0), Bs, n_s, gate_override)
        sum(g * l for g, l in zip(G, losses)).backward()
        grads = (zi.grad[:Bs], zi.grad[Bs:], zn.grad[:n_s], zn.grad[n_s:])
    else:
        leaves = [x.clone().to(dev).requires_grad_(True) for x in z_img + z_ins]
        losses, s, gates = us_daf_da_losses(*leaves, r[0].view(1, -1, 5), r[1], gate_override)
        sum(g * l for g, l in zip(G, losses)).backward()
        grads = tuple(x.grad for x in leaves)
    assert not any(x.requires_grad for x in s + gates)
    return losses, s, gates, grads


def _check(z_img, z_ins, rois, packed, margin=1e-4):
    losses, s, gates, grads = _run(z_img, z_ins, rois, packed)
    for got, z in zip(s, z_img + z_ins):
        assert got.shape == z.shape
        d = _ulp_diff(got.cpu(), torch.sigmoid(z))
        print("sigmoid ulp", d)
        assert d <= 2, d
    ref_l, ref_di, ref_dn, own, col0 = _reference(s[:2], s[2:], rois)
    for k in range(2):
        assert ((col0[k] - 0.5).abs() >= margin).all(), (col0[k] - 0.5).abs().min()
        assert torch.equal(gates[k].cpu(), own[k].float())
        close(grads[k].cpu(), ref_di[k])
        close(grads[2 + k].cpu(), ref_dn[k])
    for k in range(4):
        print("loss", k, float(losses[k]), float(ref_l[k]))
        close(losses[k].detach().cpu().reshape(1), ref_l[k].reshape(1))
    return losses, s, gates, grads


@pytest.mark.parametrize("packed", [False, True], ids=["separate", "packed"])
@pytest.mark.parametrize("case", range(4))
def test_losses_forward_backward(case, packed):
    shape_s = MAPS[case]
    shape_t = shape_s if packed else MAPS[(case + 1) % 4]  # separate: two map shapes
    n_s, n_t = ROWS[case]
    z_img, z_ins, rois = _inputs(shape_s, shape_t, n_s, n_t, seed=10 + case)
    _check(z_img, z_ins, rois, packed)


@pytest.mark.parametrize("packed", [False, True], ids=["separate", "packed"])
def test_gate_planted_rows(packed):
    """Rows well on both sides of the gate (source s = 0.55 on, 0.70 off; target s = 0.45 on,
    0.30 off): gated-off rows get exactly zero column-0 gradient and still count in the 4 R
    denominator."""
    def logit(p):
        return math.log(p / (1 - p))
    z_img, z_ins, rois = _inputs((1, 3, 4), (1, 3, 4), 4, 4, seed=3)
    z_ins[0][:, 0] = torch.tensor([logit(0.55), logit(0.70), logit(0.55), logit(0.70)])
    z_ins[1][:, 0] = torch.tensor([logit(0.45), logit(0.30), logit(0.30), logit(0.45)])
    losses, s, gates, grads = _check(z_img, z_ins, rois, packed, margin=0.09)
    assert gates[0].tolist() == [1, 0, 1, 0] and gates[1].tolist() == [1, 0, 0, 1]
    for k, y in enumerate((1.0, 0.0)):
        dz = grads[2 + k].cpu()
        off = gates[k].cpu() == 0
        assert (dz[off, 0] == 0).all() and (dz[~off, 0] != 0).all()
        assert (dz[:, 1:] != 0).all()
        # the sum over the counted elements over all 4 R = 16 elements, zeros included
        sn = s[2 + k].cpu().double()
        lab = torch.cat([torch.full((4, 1), y), scale_labels(rois[k].numpy())], 1).double()
        e = -(lab * torch.log(sn + 1e-10) + (1 - lab) * torch.log(1 - sn + 1e-10))
        e[off, 0] = 0
        close(losses[2 * k + 1].detach().cpu().reshape(1), (e.sum() / 16).reshape(1))

    # an override replaces the loss's own gates
    flip = tuple(1 - g for g in gates)
    l2, _, g2, grads2 = _run(z_img, z_ins, rois, packed, gate_override=flip)
    ref_l, _, ref_dn, _, _ = _reference(s[:2], s[2:], rois, gates=flip)
    for k in range(2):
        assert torch.equal(g2[k], flip[k])
        close(l2[2 * k + 1].detach().cpu().reshape(1), ref_l[2 * k + 1].reshape(1))
        close(grads2[2 + k].cpu(), ref_dn[k])


def test_saturation():
    """Image logits +30: s is exactly 1, the target's loss is the -100 clamp value, the
    source's is 0, and dz is exactly 0; mixed +-30 logits everywhere stay finite and meet the
    composition."""
    z_img, z_ins, rois = _inputs((1, 5, 7), (1, 5, 7), 6, 7, seed=4)
    sat = [torch.full_like(z, 30.0) for z in z_img]
    losses, s, _, grads = _run(sat, z_ins, rois, True)
    assert (s[0] == 1).all() and (s[1] == 1).all()
    assert float(losses[0]) == 0.0 and float(losses[2]) == 100.0
    assert (grads[0] == 0).all() and (grads[1] == 0).all()

    g = torch.Generator().manual_seed(5)
    for z in z_img + z_ins:
        z.copy_(torch.where(torch.rand(z.shape, generator=g) < 0.5, -30.0, 30.0))
    for packed in (False, True):
        # column-0 element losses are ~0 or log(1e-10) = 23: far from the gate's 0.5
        losses, s, _, grads = _check(z_img, z_ins, rois, packed, margin=0.4)
        assert all(torch.isfinite(x).all() for x in losses + grads)
        # log(1e-10) where an instance output saturates against its label
        assert float(losses[1]) > 1.0 and float(losses[3]) > 1.0
        sat1 = s[0] == 1
        assert sat1.any() and (grads[0][sat1] == 0).all() and (grads[1][s[1] == 1] == 0).all()


def test_two_runs_are_bit_identical():
    z_img, z_ins, rois = _inputs(MAPS[3], MAPS[3], 256, 300, seed=6)
    for packed in (False, True):
        a, b = _run(z_img, z_ins, rois, packed), _run(z_img, z_ins, rois, packed)
        for x, y in zip(a, b):
            assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(x, y))


def test_fused_matches_unfused(monkeypatch):
    """TLOD_FUSED_LOSSES=0 (the torch composition): the same losses and gradients under close,
    identical gates."""
    z_img, z_ins, rois = _inputs(MAPS[2], MAPS[2], 128, 300, seed=7)
    for packed in (False, True):
        fused = _run(z_img, z_ins, rois, packed)
        monkeypatch.setenv("TLOD_FUSED_LOSSES", "0")
        plain = _run(z_img, z_ins, rois, packed)
        monkeypatch.delenv("TLOD_FUSED_LOSSES")
        for k in range(4):
            close(fused[0][k].detach().reshape(1), plain[0][k].detach().reshape(1))
            close(fused[3][k], plain[3][k])
        assert torch.equal(fused[2][0], plain[2][0]) and torch.equal(fused[2][1], plain[2][1])


def test_argument_errors():
    from tlod.da.us_daf import us_daf_da_losses
    z = torch.zeros(1, 1, 2, 2)
    with pytest.raises(RuntimeError):  # CPU tensors never reach the kernels
        us_daf_da_losses(z, z, torch.zeros(2, 4), torch.zeros(2, 4), torch.zeros(2, 5),
                         torch.zeros(2, 5))
