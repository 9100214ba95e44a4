"""The PT-MAF kernels (csrc/pt_maf.hip) alone: the foreground / background maps and the gt
cell mask bit-exact against the torch expressions / the literal loops, the masked NLL and the
KD KL (forward and backward) against the torch compositions in fp64 from the same fp32
inputs, at the bar of the fused losses (tests/test_losses_gpu.close, rtol 2e-5), and every
kernel bit-identical from run to run."""
import pytest
import torch
import torch.nn.functional as F

from ref_pt_maf import fgbg_maps as ref_maps
from ref_pt_maf import gt_cell_mask as ref_mask
from test_losses_gpu import close

pytestmark = pytest.mark.gpu
dev = "cuda"

SHAPES = [(1, 12, 12, 20), (2, 3, 5, 7), (1, 12, 37, 75), (2, 1, 1, 1)]
HIGH, LOW = 0.7, 0.1


# ------------------------------------------------------------------------------ maps
def _prob(B, A, H, W, kind, seed=0):
    """fp32 RPN-like probabilities (B, 2A, H, W); channels A.. are the object side."""
    g = torch.Generator().manual_seed(seed + 17 * H + W)
    if kind == "structured":  # wide logits: cells on both sides of both thresholds
        obj = torch.sigmoid(torch.randn(B, A, H, W, generator=g) * 4 - 6)
        obj[:, :, 0, 0] = 0.95 - 0.2 * torch.arange(B).view(B, 1)  # a different maximum per image
        if H * W > 1:
            obj[:, :, -1, -1] = 0.01
    elif kind == "equal":
        obj = torch.full((B, A, H, W), 0.375)
    else:  # "planted": cells exactly at m * high and m * low, and their neighbours
        obj = torch.full((B, A, H, W), 0.3)
        m = torch.tensor(0.8125)
        vals = [m, m * HIGH, m * LOW, torch.nextafter(m * HIGH, m), torch.nextafter(m * HIGH, -m),
                torch.nextafter(m * LOW, m), torch.nextafter(m * LOW, -m)]
        flat = obj.view(B, A, -1)
        for i, v in enumerate(vals[:H * W]):
            flat[:, :, i] = v
    return torch.cat([1 - obj, obj], 1).contiguous()


def _check_maps(prob, A):
    from tlod.da.pt_maf import fgbg_maps
    f, b, stats = fgbg_maps(prob.to(dev), A, HIGH, LOW)
    f, b, stats = f.cpu(), b.cpu(), stats.cpu()
    for i in range(prob.shape[0]):
        rf, rb, m, ratio_f, ratio_b = ref_maps(prob[i:i + 1], A, HIGH, LOW)
        assert torch.equal(f[i], rf[0]) and torch.equal(b[i], rb[0])
        ref = torch.stack([m, rf.sum(), rb.sum(), ratio_f, ratio_b])
        assert torch.equal(stats[i], ref), (stats[i], ref)
    return f, b, stats


@pytest.mark.parametrize("B,A,H,W", SHAPES)
@pytest.mark.parametrize("kind", ["structured", "equal", "planted"])
def test_fgbg_maps_bit_exact(B, A, H, W, kind):
    prob = _prob(B, A, H, W, kind)
    f, b, stats = _check_maps(prob, A)
    if kind == "structured" and H * W > 1:
        assert (f.sum((1, 2)) > 0).all() and (b.sum((1, 2)) > 0).all()
        if B > 1:
            assert stats[0, 0] != stats[1, 0]  # the two images have different maxima
    if kind == "equal":
        assert (f == 1).all() and (b == 0).all() and (stats[:, 3] == 1).all()
    if kind == "planted" and H * W >= 7:
        flat = f.view(B, -1), b.view(B, -1)
        # cell 1 sits exactly at m * high and cell 2 at m * low: strict compares leave both out
        assert (flat[0][:, 1] == 0).all() and (flat[1][:, 2] == 0).all()
        assert (flat[0][:, 3] == 1).all() and (flat[0][:, 4] == 0).all()
        assert (flat[1][:, 5] == 0).all() and (flat[1][:, 6] == 1).all()


def test_fgbg_maps_switch_matches(monkeypatch):
    """TLOD_FUSED_LOSSES=0: the torch composition gives the same bits."""
    from tlod.da.pt_maf import fgbg_maps
    prob = _prob(2, 3, 5, 7, "structured").to(dev)
    a = fgbg_maps(prob, 3, HIGH, LOW)
    monkeypatch.setenv("TLOD_FUSED_LOSSES", "0")
    b = fgbg_maps(prob, 3, HIGH, LOW)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------ masked NLL
def _nll_ref(score, cells, need):
    """fp64 torch composition: per image nll_loss(log_softmax, label on the map else -1,
    ignore_index=-1), 0 for an empty map."""
    s = score.detach().double().cpu().requires_grad_(True)
    out = []
    for i in range(s.shape[0]):
        c = cells[i:i + 1].cpu()
        if int(c.sum()) == 0:
            out.append(s[i].sum() * 0.0)
            continue
        lab = torch.where(c == 1, torch.full_like(c, float(need[i])).long(),
                          torch.full_like(c, -1).long())
        out.append(F.nll_loss(F.log_softmax(s[i:i + 1], 1), lab, ignore_index=-1))
    return s, torch.stack(out)


def _nll_inputs(B, H, W, seed, K=3):
    g = torch.Generator().manual_seed(seed)
    scores = [(torch.randn(B, 2, H, W, generator=g) * 3).to(dev).requires_grad_(True)
              for _ in range(K)]
    maps = [(torch.rand(B, H, W, generator=g) < 0.4).float().to(dev) for _ in range(K)]
    need = torch.tensor([1.0, 0.0][:B], device=dev)  # labels 1 and 0 in one batch
    return scores, maps, need


@pytest.mark.parametrize("B,A,H,W", SHAPES)
def test_masked_nll2(B, A, H, W):
    from tlod.da.pt_maf import masked_nll2
    scores, maps, need = _nll_inputs(B, H, W, 100 + H)
    maps[1].zero_()                       # an empty map
    maps[2].zero_()
    maps[2].view(B, -1)[:, (H * W) // 2] = 1.0  # a one-cell map
    pairs = list(zip(scores, maps)) + [(scores[0], maps[2])]  # a score used by two pairs
    loss = masked_nll2(need, pairs)
    assert loss.shape == (4, B)
    gw = torch.arange(1, 4 * B + 1, device=dev, dtype=torch.float32).view(4, B) / 7
    (loss * gw).sum().backward()
    assert torch.isfinite(loss).all()
    assert (loss[1] == 0).all() and torch.count_nonzero(scores[1].grad).item() == 0
    refs = [_nll_ref(s, m, need) for s, m in pairs]
    for k, (s64, r) in enumerate(refs):
        close(loss[k].cpu(), r.detach())
        (r * gw[k].double().cpu()).sum().backward()
    close(scores[0].grad.cpu(), refs[0][0].grad + refs[3][0].grad)
    close(scores[2].grad.cpu(), refs[2][0].grad)
    assert not torch.isnan(scores[0].grad).any() and not torch.isnan(scores[1].grad).any()


def test_masked_nll2_switch_matches(monkeypatch):
    from tlod.da.pt_maf import masked_nll2
    scores, maps, need = _nll_inputs(2, 5, 7, 3)
    maps[1].zero_()
    fused = masked_nll2(need, list(zip(scores, maps)))
    fused.sum().backward()
    g = [s.grad.clone() for s in scores]
    for s in scores:
        s.grad = None
    monkeypatch.setenv("TLOD_FUSED_LOSSES", "0")
    plain = masked_nll2(need, list(zip(scores, maps)))
    plain.sum().backward()
    close(fused, plain.detach())
    for a, s in zip(g, scores):
        close(a, s.grad)
    assert torch.count_nonzero(scores[1].grad).item() == 0


# ------------------------------------------------------------------------------ KD KL
def _kd_ref(student, teacher, weight, T, rpn_shape=None):
    """fp64 torch composition of PT_MAF_train.py:449-451 (one of its two parts)."""
    s = student.detach().double().cpu().requires_grad_(True)
    t, w = teacher.double().cpu(), weight.double().cpu()
    p1, p2 = F.softmax(s / T, 1), F.softmax(t / T, 1)
    if rpn_shape is not None:
        A, H, W = rpn_shape
        p1, p2 = p1.view(1, 2 * A, H, W), p2.view(1, 2 * A, H, W)
    else:
        w = w.unsqueeze(1)
    loss = (1. / (w.sum() + 1)) * (w * p1 * torch.log(p1 / p2)).sum()
    return s, loss


def _kd_rows(R, C, seed, mag=2.0):
    g = torch.Generator().manual_seed(seed)
    s = (torch.randn(R, C, generator=g) * mag).to(dev).requires_grad_(True)
    t = (torch.randn(R, C, generator=g) * mag).to(dev)
    w = (torch.rand(R, generator=g) < 0.3).float().to(dev)
    w[0] = 1.0
    return s, t, w


@pytest.mark.parametrize("T", [1.0, 3.0])
@pytest.mark.parametrize("R,C", [(256, 9), (7, 21), (1, 2)])
def test_kd_kl_rows(R, C, T):
    from tlod.da.pt_maf import kd_kl_rows
    s, t, w = _kd_rows(R, C, R + C)
    loss = kd_kl_rows(s, t, w, T)
    (loss * 1.5).backward()
    s64, ref = _kd_ref(s, t, w, T)
    (ref * 1.5).backward()
    close(loss.cpu(), ref.detach())
    close(s.grad.cpu(), s64.grad)


@pytest.mark.parametrize("T", [1.0, 3.0])
@pytest.mark.parametrize("A,H,W", [(12, 12, 20), (3, 5, 7)])
def test_kd_kl_rpn_strided(A, H, W, T):
    from tlod.da.pt_maf import kd_kl_rpn
    g = torch.Generator().manual_seed(A + H + W)
    s = (torch.randn(1, 2, A * H, W, generator=g) * 2).to(dev).requires_grad_(True)
    t = (torch.randn(1, 2, A * H, W, generator=g) * 2).to(dev)
    cells = (torch.rand(H, W, generator=g) < 0.3).float().to(dev)
    loss = kd_kl_rpn(s, t, cells, T)
    loss.backward()
    s64, ref = _kd_ref(s, t, cells, T, (A, H, W))
    ref.backward()
    close(loss.cpu(), ref.detach())
    close(s.grad.cpu(), s64.grad)


def test_kd_kl_edge_cases():
    from tlod.da.pt_maf import kd_kl_rows
    s, t, w = _kd_rows(37, 9, 5)
    loss = kd_kl_rows(s, t, torch.zeros_like(w), 3.0)  # all-zero weights
    loss.backward()
    assert loss.item() == 0.0 and torch.count_nonzero(s.grad).item() == 0
    s.grad = None
    same = kd_kl_rows(s, s.detach().clone(), w, 3.0)  # student == teacher
    same.backward()
    s64, ref = _kd_ref(s, s.detach(), w, 3.0)
    close(same.cpu(), ref.detach())
    assert abs(same.item()) <= 1e-12
    for T in (1.0, 3.0):  # scores of magnitude 30: no overflow
        s, t, w = _kd_rows(64, 9, 11, mag=30.0)
        big = kd_kl_rows(s, t, w, T)
        big.backward()
        s64, ref = _kd_ref(s, t, w, T)
        ref.backward()
        assert torch.isfinite(big) and torch.isfinite(s.grad).all()
        close(big.cpu(), ref.detach())
        close(s.grad.cpu(), s64.grad)


def test_kd_kl_switch_matches(monkeypatch):
    from tlod.da.pt_maf import kd_kl_rows, kd_kl_rpn
    s, t, w = _kd_rows(256, 9, 2)
    g = torch.Generator().manual_seed(4)
    rs = torch.randn(1, 2, 3 * 5, 7, generator=g).to(dev)
    rt = torch.randn(1, 2, 3 * 5, 7, generator=g).to(dev)
    cells = (torch.rand(5, 7, generator=g) < 0.5).float().to(dev)
    fused = (kd_kl_rows(s, t, w, 3.0), kd_kl_rpn(rs, rt, cells, 3.0))
    monkeypatch.setenv("TLOD_FUSED_LOSSES", "0")
    plain = (kd_kl_rows(s, t, w, 3.0), kd_kl_rpn(rs, rt, cells, 3.0))
    for a, b in zip(fused, plain):
        close(a, b.detach())


# ------------------------------------------------------------------------------ gt cell mask
def _boxes(rows, pad=6):
    gt = torch.zeros(1, pad, 5)
    for i, r in enumerate(rows):
        gt[0, i] = torch.tensor(r + [1.0])
    return gt


MASK_CASES = {
    "none": ([], 0),
    "thin": ([[33.0, 20.0, 47.9, 100.0], [10.0, 50.0, 200.0, 63.0]], 2),  # empty ranges
    "last": ([[250.0, 100.0, 320.0, 192.0], [0.0, 0.0, 320.0, 16.0]], 2),  # last row / column
    "overlap": ([[20.0, 20.0, 120.0, 120.0], [60.0, 40.0, 200.0, 90.0], [16.0, 16.0, 32.0, 32.0]],
                3),
    "padded": ([[20.0, 20.0, 120.0, 120.0], [200.0, 100.0, 300.0, 180.0]], 1),  # num < rows
}


@pytest.mark.parametrize("case", sorted(MASK_CASES))
def test_gt_cell_mask_bit_exact(case):
    from tlod.da.pt_maf import gt_cell_mask
    rows, num = MASK_CASES[case]
    gt = _boxes(rows)
    H, W = 12, 20
    got = gt_cell_mask(gt.to(dev), torch.tensor([num], device=dev), H, W).cpu()
    ref = ref_mask(gt, num, H, W)
    assert torch.equal(got, ref)
    if case in ("none", "thin"):
        assert got.sum() == 0
    if case == "last":
        assert got[11, 19] == 1 and got[0, 19] == 1
    if case == "padded":
        assert got[8, 15] == 0 and got[3, 3] == 1


# ------------------------------------------------------------------------------ determinism
def test_kernels_bit_identical_across_runs():
    from tlod.da.pt_maf import fgbg_maps, gt_cell_mask, kd_kl_rpn, masked_nll2

    def run():
        prob = _prob(1, 12, 37, 75, "structured").to(dev)
        out = list(fgbg_maps(prob, 12, HIGH, LOW))
        scores, maps, need = _nll_inputs(1, 37, 75, 9)
        loss = masked_nll2(need, list(zip(scores, maps)))
        loss.sum().backward()
        out += [loss.detach()] + [s.grad for s in scores]
        g = torch.Generator().manual_seed(1)
        s = torch.randn(1, 2, 12 * 37, 75, generator=g).to(dev).requires_grad_(True)
        t = torch.randn(1, 2, 12 * 37, 75, generator=g).to(dev)
        cells = gt_cell_mask(_boxes(MASK_CASES["overlap"][0]).to(dev),
                             torch.tensor([3], device=dev), 37, 75)
        kd = kd_kl_rpn(s, t, cells, 3.0)
        kd.backward()
        return out + [cells, kd.detach(), s.grad]

    for a, b in zip(run(), run()):
        assert torch.equal(a, b)
