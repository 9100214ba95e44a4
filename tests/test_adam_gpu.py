"""Fused clip_gradient + Adam (tlod_adam_clip_pack_f32, tlod.optim.FusedAdamClip) and the
fused optimizers' checkpoints.

The measure of every comparison with torch: an fp64 restatement of the update is the truth,
torch's own fp32 optimizer (foreach=False) on the same gradients has a max abs error E_torch
against it per tensor, and the fused result's error must be at most
max(2 * E_torch, 4 ulp of the largest |parameter|): both are fp32 evaluations of one formula
that differ only in association (torch's lerp against two products, where the bias
corrections divide), and a result cannot be asked to be closer than a few roundings of its
own magnitude.
"""
import math

import pytest
import torch

from fused_optim import B1, B2, EPS, Truth, check_bar  # shared with test_fused_optim_*.py

pytestmark = pytest.mark.gpu


def two_groups(ws, bs, lr=0.01):
    return [{"params": ws, "lr": lr, "weight_decay": 5e-4},
            {"params": bs, "lr": 2 * lr, "weight_decay": 0.0}]


def torch_step(opt, params, grads, clip):
    """clip_gradient(model, clip) (net_utils.py:38-49) then the torch optimizer's step."""
    for p, g in zip(params, grads):
        p.grad = None if g is None else g.clone()
    have = [p for p in params if p.grad is not None]
    if clip > 0:
        tot = torch.sqrt(sum(p.grad.norm() ** 2 for p in have))
        s = clip / max(float(tot), clip)
        for p in have:
            p.grad.mul_(s)
    opt.step()


def fused_step(opt, params, grads):
    opt.zero_grad()
    for p, g in zip(params, grads):
        if g is not None:
            p.grad = g.clone()
    return opt.step()


def clones(params):
    return [torch.nn.Parameter(p.detach().clone()) for p in params]


@pytest.fixture(scope="module")
def mlp_case():
    """The parameters of Linear(300, 200) -> ReLU -> Linear(200, 350) (a 70000-element weight:
    two chunks; a 350-element bias: the scalar path) and five steps of assigned gradients,
    random values times logspace(-9, 1): eps matters for part of every tensor."""
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(300, 200), torch.nn.ReLU(),
                            torch.nn.Linear(200, 70000 // 200)).cuda()
    params = [p.detach().clone() for p in m.parameters()]
    params = [p for p in params if p.dim() > 1] + [p for p in params if p.dim() == 1]
    g = torch.Generator(device="cuda").manual_seed(1)
    grads = [[(torch.randn(p.numel(), device="cuda", generator=g) *
               torch.logspace(-9, 1, p.numel(), device="cuda")).view_as(p) for p in params]
             for _ in range(5)]
    return params, grads


@pytest.mark.parametrize("clip", [10.0, 1e-3, 0.0])
def test_fused_adam_matches_torch(clip, mlp_case):
    """Five steps over the chunk paths (vector and scalar, a chunk boundary) with clipping
    that bites (10, 1e-3) and none, against the bar of this module's docstring; the returned
    norm is the unclipped gradient norm.  (MI355X: E_fused / E_torch between 0.21 and 1.45 on
    the weights; the biases under the 4-ulp floor.)"""
    from tlod.optim import FusedAdamClip
    params, grads = mlp_case
    pf, pt = clones(params), clones(params)
    fo = FusedAdamClip(two_groups(pf[:2], pf[2:]), clip_norm=clip)
    to = torch.optim.Adam(two_groups(pt[:2], pt[2:]), foreach=False)
    truth = Truth(two_groups(params[:2], params[2:]), clip)
    for gs in grads:
        norm = fused_step(fo, pf, gs)
        torch_step(to, pt, gs, clip)
        truth.step(gs)
        want = math.sqrt(sum(float((x.double() ** 2).sum()) for x in gs))
        assert abs(float(norm) - want) <= 1e-5 * want
    check_bar(pf, pt, truth.params, f"clip {clip}")
    assert fo.steps.tolist() == [5] * 4


def test_per_parameter_steps():
    """A parameter without a gradient keeps its value, exp_avg, exp_avg_sq and step count
    (torch.optim.Adam skips it likewise): a count advanced by mistake would show as a wrong
    bias correction after the later steps."""
    from tlod.optim import FusedAdamClip
    torch.manual_seed(0)
    used, unused = torch.nn.Linear(8, 8).cuda(), torch.nn.Linear(8, 8).cuda()
    params = [p.detach().clone() for p in list(used.parameters()) + list(unused.parameters())]
    pf, pt = clones(params), clones(params)
    grp = lambda ps: [{"params": ps, "lr": 0.01, "weight_decay": 5e-4}]
    fo = FusedAdamClip(grp(pf), clip_norm=10.0)
    to = torch.optim.Adam(grp(pt), foreach=False)
    truth = Truth(grp(params), 10.0)
    g = torch.Generator(device="cuda").manual_seed(2)
    for step in range(4):
        gs = [torch.randn(p.shape, device="cuda", generator=g) for p in params]
        if step == 1:
            gs[2] = gs[3] = None
            before = [x.detach().clone() for x in pf[2:] + fo.exp_avg[2:] + fo.exp_avg_sq[2:]]
        fused_step(fo, pf, gs)
        if step == 1:
            after = pf[2:] + fo.exp_avg[2:] + fo.exp_avg_sq[2:]
            assert all(torch.equal(a.detach(), b) for a, b in zip(after, before))
            assert fo.steps.tolist() == [2, 2, 1, 1]
        torch_step(to, pt, gs, 10.0)
        truth.step(gs)
    check_bar(pf, pt, truth.params, "steps")
    fs, ts = fo.state_dict()["state"], to.state_dict()["state"]
    assert sorted(fs) == sorted(ts) == [0, 1, 2, 3]
    for i in fs:
        assert fs[i]["step"].dtype == torch.float32 and fs[i]["step"].dim() == 0
        assert float(fs[i]["step"]) == float(ts[i]["step"]) == (4 if i < 2 else 3)


def test_device_side_active_skip():
    """tlod_adam_clip_f32 on a two-parameter table: the second parameter's `active` reads 0
    in the first call (data parallel: no rank produced its gradient, its slot is zero), so
    its p, m, v and step count stay bit-unchanged; it joins at the second call with the bias
    corrections of its own first step."""
    import numpy as np
    from tlod import _lib
    from tlod.optim import _ADAM_DESC, _ADAM_STATE
    torch.manual_seed(4)
    dev = "cuda"
    pa, pb = torch.randn(5000, device=dev) * 0.05, torch.randn(300, device=dev) * 0.05
    ps = [pa.clone(), pb.clone()]
    m = [torch.zeros_like(p) for p in ps]
    v = [torch.zeros_like(p) for p in ps]
    gr = [torch.empty_like(p) for p in ps]
    steps = torch.zeros(2, dtype=torch.int32, device=dev)
    corr = torch.zeros(2, 2, device=dev)
    active = torch.tensor([1.0, 0.0], device=dev)
    partials, norm_scale = torch.empty(2, device=dev), torch.zeros(2, device=dev)
    lr, wd = 0.01, 5e-4
    rows = np.array([(ps[i].data_ptr(), gr[i].data_ptr(), m[i].data_ptr(), v[i].data_ptr(),
                      ps[i].numel(), lr, wd, active.data_ptr() + 4 * i, corr.data_ptr() + 8 * i)
                     for i in range(2)], dtype=_ADAM_DESC)
    srows = np.array([(steps.data_ptr() + 4 * i, active.data_ptr() + 4 * i,
                       corr.data_ptr() + 8 * i) for i in range(2)], dtype=_ADAM_STATE)
    up = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to(dev)
    chunks, states = up(rows), up(srows)

    def call():
        _lib.check(_lib.lib().tlod_adam_clip_f32(
            _lib.ptr(chunks), 2, _lib.ptr(states), 2, 1.0, B1, B2, EPS, 10.0,
            _lib.ptr(partials), _lib.ptr(norm_scale), _lib.stream_of(partials)), "adam_clip")

    pt = clones([pa, pb])
    grp = lambda q: [{"params": q, "lr": lr, "weight_decay": wd}]
    to = torch.optim.Adam(grp(pt), foreach=False)
    truth = Truth(grp([pa, pb]), 10.0)
    g = torch.Generator(device=dev).manual_seed(5)
    g0 = [torch.randn(5000, device=dev, generator=g), torch.zeros(300, device=dev)]
    g1 = [torch.randn(5000, device=dev, generator=g), torch.randn(300, device=dev, generator=g)]
    for x, y in zip(gr, g0):
        x.copy_(y)
    call()
    assert torch.equal(ps[1], pb) and not m[1].any() and not v[1].any()
    assert steps.tolist() == [1, 0] and not corr[1].any()
    assert not torch.equal(ps[0], pa)
    active.fill_(1.0)
    for x, y in zip(gr, g1):
        x.copy_(y)
    call()
    assert steps.tolist() == [2, 1]
    for gs in ([g0[0], None], g1):
        torch_step(to, pt, gs, 10.0)
        truth.step(gs)
    check_bar(ps, pt, truth.params, "active")


@pytest.mark.parametrize("clip", [0.0, 10.0])
def test_fused_adam_pack_update(clip, monkeypatch):
    """The 3x3 weights a FusedAdamClip owns are updated by tiles that also write their
    split-bf16 packs: after every step the cached packs (the same objects, PACK_GEN unchanged)
    are bit-identical to packs made from the updated weights, and the weights match the
    chunk-only update (TLOD_SGD_PACK=0) bit for bit.  Ragged channel counts, a BN-scaled
    input-gradient pack, Cin = 3."""
    from tlod import conv
    from tlod.optim import FusedAdamClip
    shapes = [(40, 24), (64, 64), (80, 36), (16, 3), (33, 65)]
    g = torch.Generator(device="cuda").manual_seed(1)

    def params():
        torch.manual_seed(3)
        ws = [torch.nn.Parameter(torch.randn(co, ci, 3, 3, device="cuda") * 0.05)
              for co, ci in shapes]
        return ws + [torch.nn.Parameter(torch.randn(40, device="cuda"))]

    pa, pb = params(), params()
    scale = torch.rand(80, device="cuda") + 0.5
    groups = lambda ps: [{"params": ps[:-1], "lr": 0.01, "weight_decay": 5e-4},
                         {"params": ps[-1:], "lr": 0.02, "weight_decay": 0.0}]
    monkeypatch.setenv("TLOD_SGD_PACK", "1")
    fo = FusedAdamClip(groups(pa), clip_norm=clip)
    monkeypatch.setenv("TLOD_SGD_PACK", "0")
    ro = FusedAdamClip(groups(pb), clip_norm=clip)
    assert all(getattr(w, "_tlod_pack_owner", False) for w in pa[:-1])
    assert not any(getattr(w, "_tlod_pack_owner", False) for w in pb)

    def packs():
        out = []
        for w in pa[:-1]:
            out += [conv.pack_bs(w, False), conv.pack_bs(w, True)]
        return out + [conv.pack_bs(pa[2], True, scale)]
    first = packs()
    gen = conv.PACK_GEN[0]
    start = [p.detach().clone() for p in pa]
    for step in range(3):
        rs = [torch.randn(p.shape, device="cuda", generator=g) for p in pa]
        for ps, opt in ((pa, fo), (pb, ro)):
            opt.zero_grad()
            sum((p * r).sum() for p, r in zip(ps, rs)).backward()
            opt.step()
        for a, b in zip(pa, pb):
            assert torch.equal(a.detach(), b.detach())
        now = packs()
        assert conv.PACK_GEN[0] == gen and all(x is y for x, y in zip(now, first))
        fresh = []
        for w in pa[:-1]:
            fresh += [conv._pack_bs(w, False), conv._pack_bs(w, True)]
        fresh.append(conv._pack_bs(pa[2], True, scale))
        for i, (x, y) in enumerate(zip(now, fresh)):
            assert torch.equal(x, y), (step, i)
    assert not any(torch.equal(a.detach(), s) for a, s in zip(pa, start))
    assert fo.steps.tolist() == ro.steps.tolist() == [3] * 6


def test_learning_rate_decay():
    """adjust_learning_rate (param_group['lr'] *= 0.1) between steps takes effect at the next
    step; steps that change nothing reuse the uploaded tables."""
    from tlod.optim import FusedAdamClip
    torch.manual_seed(6)
    params = [torch.randn(40, 30, device="cuda") * 0.1, torch.randn(30, device="cuda") * 0.1]
    pf, pt = clones(params), clones(params)
    fo = FusedAdamClip(two_groups(pf[:1], pf[1:]), clip_norm=10.0)
    to = torch.optim.Adam(two_groups(pt[:1], pt[1:]), foreach=False)
    truth = Truth(two_groups(params[:1], params[1:]), 10.0)
    g = torch.Generator(device="cuda").manual_seed(7)
    builds = []
    for step in range(4):
        if step == 2:
            for grp in fo.param_groups + to.param_groups + truth.groups:
                grp["lr"] *= 0.1
        gs = [torch.randn(p.shape, device="cuda", generator=g) for p in params]
        fo.zero_grad()
        sum((p * r).sum() for p, r in zip(pf, gs)).backward()  # gradients land in the arena
        fo.step()
        builds.append(fo.table_builds)
        torch_step(to, pt, gs, 10.0)
        truth.step(gs)
    check_bar(pf, pt, truth.params, "lr decay")
    assert builds[1] == builds[0] and builds[3] == builds[2] and builds[2] == builds[0] + 1


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_checkpoint_round_trip(kind):
    """state_dict() / load_state_dict() in torch's layout: two steps, a hand-over in either
    direction between the fused optimizer and torch's, two more steps; fused to fused is
    bit-identical to four uninterrupted steps.  A parameter that never had a gradient has no
    state entry."""
    from tlod.optim import FusedAdamClip, FusedSGDClip
    torch.manual_seed(8)
    params = [torch.randn(70, 33, device="cuda") * 0.1, torch.randn(50, 20, device="cuda") * 0.1,
              torch.randn(33, device="cuda") * 0.1, torch.randn(20, device="cuda") * 0.1]
    clip = 10.0
    grp = lambda ps: two_groups(ps[:2], ps[2:])

    def fused(ps):
        return FusedAdamClip(grp(ps), clip_norm=clip) if kind == "adam" else \
            FusedSGDClip(grp(ps), momentum=0.9, clip_norm=clip)

    def plain(ps):
        return torch.optim.Adam(grp(ps), foreach=False) if kind == "adam" else \
            torch.optim.SGD(grp(ps), momentum=0.9, foreach=False)

    g = torch.Generator(device="cuda").manual_seed(9)
    grads = [[torch.randn(p.shape, device="cuda", generator=g) for p in params] for _ in range(4)]
    for gs in grads:
        gs[1] = None  # never a gradient: no state, in either optimizer

    def run(first, second):
        """Two steps with first(params), its state handed to second(same params), two more."""
        ps = clones(params)
        opt = first(ps)
        for i in range(4):
            if i == 2 and second is not None:
                sd = opt.state_dict()
                assert sorted(sd["state"]) == [0, 2, 3]
                opt = second(ps)
                opt.load_state_dict(sd)
                assert sorted(opt.state_dict()["state"]) == [0, 2, 3]
            if isinstance(opt, torch.optim.Optimizer):
                torch_step(opt, ps, grads[i], clip)
            else:
                fused_step(opt, ps, grads[i])
        return ps

    truth = Truth(grp(params), clip, kind)
    for gs in grads:
        truth.step(gs)
    t4, f4 = run(plain, None), run(fused, None)
    check_bar(f4, t4, truth.params, f"{kind} fused")
    check_bar(run(fused, plain), t4, truth.params, f"{kind} fused->torch")
    check_bar(run(plain, fused), t4, truth.params, f"{kind} torch->fused")
    for a, b in zip(run(fused, fused), f4):
        assert torch.equal(a.detach(), b.detach())


def test_detector_adam_step():
    """DAF-VGG16 with make_optimizer(optimizer="adam"): the fused step against clip_gradient +
    torch.optim.Adam on the same gradients; the packs it wrote are the ones the next forward
    reads; fused=False gives the torch optimizer."""
    from tlod import conv
    from tlod.detector.train import (SyntheticCityscapes, build_model, clip_gradient_,
                                     make_optimizer, train_step)
    from tlod.optim import FusedAdamClip
    dev = torch.device("cuda:0")
    model = build_model("daf", dev, "vgg16")
    opt = make_optimizer(model, 2e-3, optimizer="adam")
    assert isinstance(opt, FusedAdamClip) and opt.clip_norm == 10.0
    data = SyntheticCityscapes(dev, H=192, W=320, G=4, pool=1, seed=7)
    batch = data.next()
    opt.zero_grad()
    model.total_loss(model(*batch), 0.1).backward()
    live = [(i, p) for i, p in enumerate(opt.params) if p.grad is not None]
    n0 = len(opt.param_groups[0]["params"])
    cl = clones([p for _, p in live])
    grads = [p.grad.detach().clone() for _, p in live]
    tgroups = [{"params": [c for c, (i, _) in zip(cl, live) if (i < n0) == first],
                "lr": grp["lr"], "weight_decay": grp["weight_decay"]}
               for first, grp in ((True, opt.param_groups[0]), (False, opt.param_groups[1]))]
    to = torch.optim.Adam(tgroups, foreach=False)
    truth = Truth(tgroups, 10.0)
    for c, gr in zip(cl, grads):
        c.grad = gr.clone()
    clip_gradient_(cl, 10.0)
    to.step()
    truth.step(grads)
    opt.step()
    check_bar([p for _, p in live], cl, truth.params, "daf-vgg16")
    del truth, to, cl, grads

    loss = train_step(model, opt, batch)
    assert math.isfinite(float(loss))
    owned = 0
    for p in opt.params:
        if getattr(p, "_tlod_pack_owner", False):
            for (dgrad, _), (_, pk, scale) in getattr(p, "_tlod_packs", {}).items():
                assert conv.pack_bs(p, dgrad, scale) is pk
                assert torch.equal(pk, conv._pack_bs(p, dgrad, scale)), (tuple(p.shape), dgrad)
                owned += 1
    assert owned > 0
    del model, opt

    model = build_model("daf", dev, "vgg16")
    plain = make_optimizer(model, 2e-3, optimizer="adam", fused=False)
    assert isinstance(plain, torch.optim.Adam)
    assert math.isfinite(float(train_step(model, plain, batch)))
