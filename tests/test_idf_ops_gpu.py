"""The IDF kernels (csrc/idf.hip through tlod.da.idf) against the CPU restatement
(tests/ref_idf.py) in fp64.

Shapes: (1, 512, 24, 40); (1, 24, 5, 7) — fewer pixels than a wave, C no multiple of the 16
channel slices; (2, 512, 37, 75) — two images (a threshold each), 2775 pixels (no multiple of
64, 44 workgroups per image); (1, 256, 48, 80) with NULL attention: dist1.

Bars:
  att       the on / off pattern of the fp64 restatement, except cells whose avg lies within
            1e-5 thr of the threshold (at most 1 % of the cells); on-values within 1e-6 relative;
  dist      within 1e-6 relative of fp64;
  a_out, b_out   bit-equal to the fp32 composition a * (1 + att);
  gradients max |g - g64| / max |g64| at most 2 x the same measure of the fp32 restatement (CPU
            autograd) on the same inputs, measured here; floor 2^-24, the half ulp of the largest
            element, below which no fp32 result can be held;
  domain losses and their gradients within 2e-5 (the project's fused-loss bar) of the torch
            composition, rows with softmax[label] < 1e-6 included."""
import functools
import math

import pytest
import torch

import ref_idf

pytestmark = pytest.mark.gpu
dev = "cuda"

SHAPES = [(1, 512, 24, 40), (1, 24, 5, 7), (2, 512, 37, 75)]
HALF_ULP = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def case(shape):
    """Inputs and the fp64 / fp32 CPU references of one shape, computed once and shared."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(C + H)
    a = torch.randn(shape, generator=g)
    b = a + 0.5 * torch.randn(shape, generator=g)
    c = {"a": a, "b": b, "att_a": ref_idf.dam(a), "att_b": ref_idf.dam(b)}
    c["ga"], c["gb"] = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    c["gd"] = torch.randn(N, generator=g) * 50
    for dt, key in ((torch.float64, "64"), (torch.float32, "32")):
        x, y = a.clone().to(dt).requires_grad_(True), b.clone().to(dt).requires_grad_(True)
        ta, tb = c["att_a"].to(dt), c["att_b"].to(dt)
        ao, bo = ref_idf.modulate(x, y, ta, tb)
        dist = ref_idf.distance(x, y, tb)
        ((ao * c["ga"].to(dt)).sum() + (bo * c["gb"].to(dt)).sum()
         + (dist * c["gd"].to(dt)).sum()).backward()
        c["dist" + key], c["ao" + key], c["bo" + key] = dist.detach(), ao.detach(), bo.detach()
        c["gx" + key], c["gy" + key] = x.grad, y.grad
    return c


def _dev(c, *keys):
    return [c[k].to(dev) for k in keys]


def _rel_max(got, ref):
    return float((got.double().cpu() - ref.double()).abs().max()) / float(ref.double().abs().max())


def _att_rule(got, x64):
    """got (N, H, W) against the fp64 restatement of x64: the 1 % / 1e-5 thr rule."""
    avg, thr = ref_idf.dam_parts(x64)
    ref = ref_idf.dam(x64)[:, 0]
    got = got.double().cpu()
    diff = (got > 0) != (ref > 0)
    print("att cells", diff.numel(), "on", int((ref > 0).sum()), "differ", int(diff.sum()))
    assert int(diff.sum()) <= 0.01 * diff.numel()
    assert (((avg - thr).abs() <= 1e-5 * thr)[:, 0][diff]).all()
    on = (got > 0) & (ref > 0)
    assert 0.2 * on.numel() < int(on.sum()) < 0.8 * on.numel()
    rel = ((got - ref).abs()[on] / ref[on]).max()
    print("att on-values rel", float(rel))
    assert rel <= 1e-6


@pytest.mark.parametrize("shape", SHAPES)
def test_dam_matches_fp64(shape):
    from tlod.da.idf import dam
    c = case(shape)
    for key in ("a", "b"):
        att = dam(c[key].to(dev))
        assert att.shape == (shape[0], shape[2], shape[3]) and att.dtype == torch.float32
        _att_rule(att, c[key].double())


def test_dam_thresholds_are_per_image():
    """A batched call gives each image the map of its own single-image call, bit for bit; the
    second image is shifted so that one batch-wide threshold would blank the first."""
    from tlod.da.idf import dam
    x = case((2, 512, 37, 75))["a"].clone()
    x[1] += 1.0
    x = x.to(dev)
    both = dam(x)
    for n in range(2):
        assert torch.equal(both[n:n + 1], dam(x[n:n + 1]))
        assert 0.2 < float((both[n] > 0).float().mean()) < 0.8


@pytest.mark.parametrize("shape", SHAPES)
def test_separation_forward(shape):
    from tlod.da.idf import separation
    c = case(shape)
    a, b, ta, tb = _dev(c, "a", "b", "att_a", "att_b")
    ao, bo, dist = separation(a, b, ta[:, 0], tb[:, 0])
    assert torch.equal(ao.cpu(), c["ao32"]) and torch.equal(bo.cpu(), c["bo32"])
    rel = ((dist.double().cpu() - c["dist64"]).abs() / c["dist64"]).max()
    print("dist", dist.tolist(), "rel", float(rel))
    assert dist.shape == (shape[0],) and rel <= 1e-6


@pytest.mark.parametrize("shape", SHAPES)
def test_separation_gradients(shape):
    from tlod.da.idf import separation
    c = case(shape)
    a, b, ta, tb, ga, gb, gd = _dev(c, "a", "b", "att_a", "att_b", "ga", "gb", "gd")
    a.requires_grad_(True)
    b.requires_grad_(True)
    ao, bo, dist = separation(a, b, ta[:, 0], tb[:, 0])
    ((ao * ga).sum() + (bo * gb).sum() + (dist * gd).sum()).backward()
    for got, k in ((a.grad, "gx"), (b.grad, "gy")):
        e_dev, e_32 = _rel_max(got, c[k + "64"]), _rel_max(c[k + "32"], c[k + "64"])
        print(k, "device", e_dev, "fp32 restatement", e_32)
        assert e_dev <= 2 * max(e_32, HALF_ULP), (k, e_dev, e_32)
    # the distance term alone (no gradient into the modulated maps: NULL g_*_out)
    a.grad = b.grad = None
    _, _, dist = separation(a, b, ta[:, 0], tb[:, 0])
    (dist * gd).sum().backward()
    x = c["a"].double().requires_grad_(True)
    (ref_idf.distance(x, c["b"].double(), c["att_b"].double()) * c["gd"].double()).sum().backward()
    x32 = c["a"].clone().requires_grad_(True)
    (ref_idf.distance(x32, c["b"], c["att_b"]) * c["gd"]).sum().backward()
    e_dev, e_32 = _rel_max(a.grad, x.grad), _rel_max(x32.grad, x.grad)
    print("t alone: device", e_dev, "fp32 restatement", e_32)
    assert e_dev <= 2 * max(e_32, HALF_ULP)
    assert torch.equal(a.grad, -b.grad)


def test_dist1_null_attention():
    from tlod.da.idf import plain_distance
    g = torch.Generator().manual_seed(9)
    a, b = torch.randn(1, 256, 48, 80, generator=g), torch.randn(1, 256, 48, 80, generator=g)
    dist = plain_distance(a.to(dev), b.to(dev))
    ref = ref_idf.distance(a.double(), b.double())
    assert dist.shape == (1,) and not dist.requires_grad
    assert abs(float(dist) - float(ref)) <= 1e-6 * float(ref)


def test_zero_attention_gives_an_exactly_zero_distance_term():
    """att_b = 0: d = sqrt(C) 1e-6 everywhere and t = 0 exactly, so g_a is g_a_out (1 + 0) bit
    for bit and neither gradient depends on the distance's upstream gradient."""
    from tlod.da.idf import separation
    c = case((1, 24, 5, 7))
    a, b, ta, ga, gb = _dev(c, "a", "b", "att_a", "ga", "gb")
    tb = torch.zeros_like(ta)
    grads = []
    for scale in (0.0, 1e6):
        x, y = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        ao, bo, dist = separation(x, y, ta[:, 0], tb[:, 0])
        ((ao * ga).sum() + (bo * gb).sum() + scale * dist.sum()).backward()
        grads.append((x.grad, y.grad))
        assert abs(float(dist) - math.sqrt(24) * 1e-6) <= 1e-6 * math.sqrt(24) * 1e-6
    assert torch.equal(grads[0][0], ga) and torch.equal(grads[1][0], ga)
    assert torch.equal(grads[0][1], grads[1][1])


def test_equal_maps():
    from tlod.da.idf import separation
    c = case((1, 24, 5, 7))
    a, ta, tb = _dev(c, "a", "att_a", "att_b")
    x, y = a.clone().requires_grad_(True), a.clone().requires_grad_(True)
    _, _, dist = separation(x, y, ta[:, 0], tb[:, 0])
    want = math.sqrt(24) * 1e-6  # 4.899e-6
    assert abs(float(dist) - want) <= 1e-6 * want
    dist.sum().backward()
    assert torch.isfinite(x.grad).all() and torch.isfinite(y.grad).all()
    assert torch.equal(x.grad, -y.grad)
    on = (tb[:, 0] > 0).unsqueeze(1).expand_as(x.grad)
    assert (x.grad[on] > 0).all() and torch.count_nonzero(x.grad[~on]).item() == 0


def test_two_runs_are_bit_identical():
    from tlod.da.idf import dam, separation
    c = case((2, 512, 37, 75))
    a, b, ga, gb, gd = _dev(c, "a", "b", "ga", "gb", "gd")
    runs = []
    for _ in range(2):
        x, y = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        ta, tb = dam(x), dam(y)
        ao, bo, dist = separation(x, y, ta, tb)
        ((ao * ga).sum() + (bo * gb).sum() + (dist * gd).sum()).backward()
        runs.append((ta, tb, ao.detach(), bo.detach(), dist.detach(), x.grad, y.grad))
    for u, v in zip(*runs):
        assert torch.equal(u, v)


def test_fused_switch_off_agrees(monkeypatch):
    """TLOD_FUSED_IDF=0 (the torch compositions on the device) against the kernels."""
    from tlod.da import idf
    c = case((1, 512, 24, 40))
    a, b = _dev(c, "a", "b")
    ta, tb = idf.dam(a), idf.dam(b)
    ao, bo, dist = idf.separation(a, b, ta, tb)
    monkeypatch.setenv("TLOD_FUSED_IDF", "0")
    assert not idf.fused_idf()
    ta0, tb0 = idf.dam(a), idf.dam(b)
    _att_rule(ta0, c["a"].double())
    assert int(((ta > 0) != (ta0 > 0)).sum()) <= 0.01 * ta.numel()
    ao0, bo0, dist0 = idf.separation(a, b, ta, tb)
    assert torch.equal(ao, ao0) and torch.equal(bo, bo0)
    assert abs(float(dist) - float(dist0)) <= 2e-6 * float(dist)


@pytest.mark.parametrize("n_img,R,label", [(6, 256, 0), (6, 300, 1), (1, 5, 1)])
def test_domain_losses_match_the_torch_composition(n_img, R, label):
    from tlod.da.idf import domain_losses, domain_losses_torch
    g = torch.Generator().manual_seed(R)
    z_img = (torch.randn(n_img, 2, generator=g) * 2).to(dev)
    z_ins = torch.randn(R, 2, generator=g) * 3
    z_ins[2] = torch.tensor([18.0, -2.0]) if label == 1 else torch.tensor([-2.0, 18.0])
    z_ins[3] = -z_ins[2]  # the confident-and-right row: p = 1 - 2e-9
    z_ins = z_ins.to(dev)
    w = torch.randn(n_img + 1, generator=g).to(dev)
    out = []
    for fn in (domain_losses, domain_losses_torch):
        zi, zn = z_img.clone().requires_grad_(True), z_ins.clone().requires_grad_(True)
        loss = fn(zi, label, zn, label, 3.0)
        (loss * w).sum().backward()
        out.append((loss.detach(), zi.grad, zn.grad))
    assert float(torch.softmax(z_ins, 1)[2, label]) < 1e-6
    for got, ref, name in zip(out[0], out[1], ("loss", "dz_img", "dz_ins")):
        err = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
        print(name, err)
        assert got.shape == ref.shape and err <= 2e-5, (name, err)
    assert torch.count_nonzero(out[0][2][2]).item() == 0  # the clamp's zero gradient
