"""The numpy restatement of the fused optimizer steps (tests/fused_optim.py) is right, and the
cases tests/test_fused_optim_gpu.py pins the device to can see what they should — without a
GPU (the case list is imported, so the two cannot drift apart).

  truth        over every case and both optimizers the restated parameters stay within
               max(2 * E_torch, 4 ulp of max |p|) of the fp64 truth after every step, E_torch
               the error of torch.optim.SGD / Adam (foreach=False) on the CPU; the restated
               gradient norm stays within its derived bound of the fp64 norm;
  inputs       no float32 intermediate of any case is subnormal (an exact 0 is allowed) or
               overflows, so bit equality with the device cannot hinge on the denormal mode;
  sensitivity  each defect of MUTATIONS, put into the restatement, changes at least one bit
               of what at least one case expects.

Measured (run with -s for every figure): the restated norm is 0 to 1.41 u (u = 2^-24) from
the fp64 norm where the bounds are 6.5 u (1000-element chunks) to 133 u (65536 elements on
the scalar path); E_restated / E_torch lies between 1.0 and 4.9 (SGD) and 1.0 and 2.7
(Adam), above 2 only where both errors sit under the 4-ulp floor; the smallest nonzero
intermediate of any case is 8.9e-32.  Every mutation is killed: most by ten or more of the 44
(case, optimizer) runs, norm_only_count_0 by the norm_only case alone, inactive_row_updated
and inactive_count_advanced by the inactive case alone, shared_step_count by inactive and
schedule.
"""
import numpy as np
import pytest
import torch

import fused_optim as F
import test_fused_optim_gpu as G

f32 = np.float32
U = 2.0 ** -24
PAIRS = [(c, k) for c in G.CASES for k in G.KINDS]
PAIR_IDS = [f"{c.name}-{k}" for c, k in PAIRS]


def _bits(arrays):
    return [(a.shape, np.ascontiguousarray(a).tobytes()) for a in arrays]


_BASE = {}


def baseline(case, kind):
    key = (case.name, kind)
    if key not in _BASE:
        _BASE[key] = _bits(G.run_expected(case, kind))
    return _BASE[key]


# ------------------------------------------------------------------ against the fp64 truth
def norm_bound(layout):
    """The relative error bound of the restated gradient norm.  A partial is a sum of
    float32 squares fl(fl(g*gs)^2), each three roundings away from (g*gs)^2, added along a
    chain of at most D float32 additions, the first of which (to a zero accumulator) is exact:
    at most D + 2 roundings per term, so the partial's relative error is at most
    gamma = (D + 2) u / (1 - (D + 2) u), u = 2^-24 (all terms are non-negative).
    D = ceil(count / 1024) + 2 + 6 + 2 on the 16-byte path (the lane's chain, the four
    accumulators, the shuffle tree, the four waves), ceil(count / 256) + 6 + 2 on the scalar
    path.  The partials are added in double (2^-53 a step, nothing next to u), so the sum of
    squares carries the largest chunk's gamma, and the square root halves it.  (The final
    rounding of the root to float32 could add u / 2 on top; the assertion does without.)"""
    worst = 0.0
    for _, _, c, vec in layout:
        n = abs(c)
        D = -(-n // 1024) + 2 + 6 + 2 if vec else -(-n // 256) + 6 + 2
        worst = max(worst, (D + 2) * U / (1 - (D + 2) * U))
    return worst / 2


def _torch_step(opt, params, grads, clip, frozen):
    """clip_gradient over every gradient, then the torch optimizer's step over those that are
    not frozen (a table's norm-only rows)."""
    for p, g in zip(params, grads):
        p.grad = None if g is None else g.clone()
    have = [p for p in params if p.grad is not None]
    if clip > 0:
        tot = torch.sqrt(sum(p.grad.norm() ** 2 for p in have))
        s = clip / max(float(tot), clip)
        for p in have:
            p.grad.mul_(s)
    for i in frozen:
        params[i].grad = None
    opt.step()


@pytest.mark.parametrize("case,kind", PAIRS, ids=PAIR_IDS)
def test_restatement_against_fp64_truth(case, kind):
    ts = case.tensors
    start = [torch.from_numpy(p.copy()) for p in case.params]
    hp = G.group_hparams(case, -1)
    grp = lambda ps: [{"params": [p for p, t in zip(ps, ts) if t.group == gi], "lr": lr,
                       "weight_decay": wd} for gi, (lr, wd) in enumerate(hp)]
    truth = F.Truth(grp(start), case.clip, kind, G.MOMENTUM)
    pt = [torch.nn.Parameter(p.clone()) for p in start]
    to = torch.optim.SGD(grp(pt), momentum=G.MOMENTUM, foreach=False) if kind == "sgd" else \
        torch.optim.Adam(grp(pt), foreach=False)
    if case.warm:
        for i, st in enumerate(case.state0):
            m, v = torch.from_numpy(st[0].copy()), torch.from_numpy(st[1].copy())
            truth.m[i], truth.v[i], truth.t[i] = m.double(), v.double(), case.t0
            to.state[pt[i]] = {"momentum_buffer": m.clone()} if kind == "sgd" else \
                {"step": torch.tensor(float(case.t0)), "exp_avg": m.clone(),
                 "exp_avg_sq": v.clone()}
    frozen = [i for i, t in enumerate(ts) if t.norm_only]
    rp = G.Replay(case, kind)
    worst_ratio = 0.0
    for s in range(case.nsteps):
        for groups in (truth.groups, to.param_groups):
            for g, (lr, wd) in zip(groups, G.group_hparams(case, s)):
                g["lr"], g["weight_decay"] = lr, wd
        dead = case.inactive.get(s, ())
        gs = [None if g is None or i in dead else g for i, g in enumerate(case.grads(s))]
        g64 = [None if g is None else torch.from_numpy(g.astype(np.float64) * case.gs)
               for g in gs]
        g32 = [None if g is None else torch.from_numpy(g * f32(case.gs)) for g in gs]
        res, layout = rp.step(s)
        truth.step(g64, norm_only=frozen)
        _torch_step(to, pt, g32, case.clip, frozen)
        rel = abs(float(res.total) - truth.norm) / truth.norm
        bound = norm_bound(layout)
        print(f"{case.name} {kind} step {s}: norm {float(res.total):.9g} fp64 {truth.norm:.12g} "
              f"rel err {rel:.3e} ({rel / U:.2f} u)  bound {bound:.3e} ({bound / U:.1f} u)")
        assert rel <= bound
        worst_ratio = max(worst_ratio, F.check_bar(
            [torch.from_numpy(p) for p in rp.params], pt, truth.params,
            f"{case.name} {kind} step {s}"))
    print(f"SUMMARY {case.name} {kind}: worst E_restated / E_torch {worst_ratio:.3f}")


# ------------------------------------------------------------------ the inputs
@pytest.mark.parametrize("case,kind", PAIRS, ids=PAIR_IDS)
def test_no_subnormal_or_overflowing_intermediate(case, kind):
    with F.Watch() as w:
        G.run_expected(case, kind)
    print(f"{case.name} {kind}: intermediates in [{w.lo:.3e}, {w.hi:.3e}]")
    assert w.bad == 0 and w.hi < float(np.finfo(np.float32).max)
    assert w.lo >= F.TINY, f"a subnormal intermediate: {w.lo!r}"


def test_cases_reach_what_they_name():
    """The regimes and paths the case list claims, read off the restatement."""
    by = {c.name: c for c in G.CASES}
    counts = sorted({abs(c) for _, _, c, _ in G.table_layout(by["counts"], 0)})
    assert counts == [1, 2, 3, 4, 255, 256, 257, 1024, 1028, 65535, 65536]
    second = [(c, vec) for _, off, c, vec in G.table_layout(by["counts"], 0) if off]
    assert second == [(1, False), (4, True), (2, False)]  # of 65537, 65540, 65538
    assert [vec for *_, vec in G.table_layout(by["grad_misaligned"], 0)] == \
        [False, False, False, False, True]
    assert all(vec for *_, vec in G.table_layout(by["state_misaligned"], 0))
    for kind in G.KINDS:
        for name, want in (("under", "one"), ("off", "one"), ("over1.5", 1.5),
                           ("over1e4", 1e4)):
            for gs in ("1", "8th", "3rd"):
                rp = G.Replay(by[f"gs_{gs}_clip_{name}"], kind)
                res, _ = rp.step(0)
                if want == "one":
                    assert float(res.scale) == 1.0
                else:
                    assert abs(1 / float(res.scale) / want - 1) < 1e-3
        rp = G.Replay(by["total_eq_clip"], kind)
        for s in range(3):
            res, _ = rp.step(s)
            assert float(res.total) == by["total_eq_clip"].clip and float(res.scale) == 1.0
        rp = G.Replay(by["schedule"], kind)
        scales = [float(rp.step(s)[0].scale) for s in range(3)]
        assert scales[0] < 1.0 and scales[1] == 1.0


# ------------------------------------------------------------------ sensitivity
def _grad_term(fn):
    return lambda mp: mp.setattr(F, "grad_term", fn)


def _sgd1(tail):
    """sgd1 with another update of (b, p) from d."""
    def make(mp):
        def sgd1(g, p, b, gs, scale, wd, lr, momentum):
            return tail(F.grad_term(g, p, gs, scale, wd), p, b, f32(lr), f32(momentum))
        mp.setattr(F, "sgd1", sgd1)
    return make


def _adam1(den, consts=None):
    """adam1 with another denominator, or other constants."""
    def make(mp):
        def adam1(g, p, m, v, gs, scale, wd, step, c2, k):
            d = F.grad_term(g, p, gs, scale, wd)
            m = k.b1 * m + k.omb1 * d
            v = k.b2 * v + (k.omb2 * d) * d
            return p - f32(step) * (m / den(v, f32(c2), k.eps)), m, v
        mp.setattr(F, "adam1", adam1)
    return make


def _swap_lr(mp):
    orig = G.group_hparams

    def swapped(case, s):
        (l0, w0), (l1, w1) = orig(case, s)
        return [[l1, w0], [l0, w1]]
    mp.setattr(G, "group_hparams", swapped)


def _wrap(name, fn):
    """Replace F.<name> by fn(original)."""
    return lambda mp: mp.setattr(F, name, fn(getattr(F, name)))


def _one_chain(orig):
    def chunk_sumsq(grad, gs, vec):
        t = F._vec(grad) * f32(gs)
        sq = t * t
        return np.add.accumulate(sq, dtype=np.float32)[-1] if sq.size else f32(0)
    return chunk_sumsq


def _fma_tail(d, p, b, lr, mom):
    b = mom * b + d
    return f32(p.astype(np.float64) - np.float64(lr) * b.astype(np.float64)), b


def _nesterov_tail(d, p, b, lr, mom):
    b = mom * b + d
    return p - lr * (d + mom * b), b


def _keep_advances(mp):
    live = F.is_live
    mp.setattr(F, "advances", lambda active: live(active))
    mp.setattr(F, "is_live", lambda active: True)


# name -> (the optimizers it touches, how to put it into the restatement)
MUTATIONS = {
    "no_weight_decay": (G.KINDS, _wrap("grad_term", lambda o: lambda g, p, gs, sc, wd:
                                       o(g, p, gs, sc, 0.0))),
    "half_weight_decay": (G.KINDS, _wrap("grad_term", lambda o: lambda g, p, gs, sc, wd:
                                         o(g, p, gs, sc, f32(wd) * f32(0.5)))),
    "wd_before_clip": (G.KINDS, _grad_term(lambda g, p, gs, sc, wd:
                                           (g * f32(gs) + f32(wd) * p) * f32(sc))),
    "scale_before_gs": (G.KINDS, _grad_term(lambda g, p, gs, sc, wd:
                                            (g * f32(sc)) * f32(gs) + f32(wd) * p)),
    "gs_in_update_only": (G.KINDS, _wrap("chunk_sumsq", lambda o: lambda grad, gs, vec:
                                         o(grad, 1.0, vec))),
    "gs_in_norm_only": (G.KINDS, _wrap("grad_term", lambda o: lambda g, p, gs, sc, wd:
                                       o(g, p, 1.0, sc, wd))),
    "momentum_0.89": (("sgd",), _wrap("sgd1", lambda o: lambda g, p, b, gs, sc, wd, lr, mom:
                                      o(g, p, b, gs, sc, wd, lr, 0.89))),
    "dampening": (("sgd",), _sgd1(lambda d, p, b, lr, mom:
                                  (lambda nb: (p - lr * nb, nb))(mom * b + (f32(1) - mom) * d))),
    "nesterov": (("sgd",), _sgd1(_nesterov_tail)),
    "fused_multiply_add": (("sgd",), _sgd1(_fma_tail)),
    "lr_swapped": (G.KINDS, _swap_lr),
    "chunk_dropped_from_norm": (G.KINDS, _wrap("grad_norm", lambda o: lambda partials, clip:
                                               o(partials[:-1] if len(partials) > 1
                                                 else partials, clip))),
    "norm_only_count_0": (G.KINDS, _wrap("row_counts", lambda o: lambda c:
                                         (max(c, 0), max(c, 0)))),
    "tail_skipped": (G.KINDS, _wrap("row_counts", lambda o: lambda c:
                                    (abs(c) // 4 * 4, max(c, 0) // 4 * 4))),
    "torch_clip_form": (G.KINDS, _wrap("clip_scale", lambda o: lambda total, clip:
                                       min(f32(1), f32(clip) / (f32(total) + f32(1e-6)))
                                       if clip > 0 else f32(1))),
    "norm_in_one_chain": (G.KINDS, _wrap("chunk_sumsq", _one_chain)),
    "inactive_row_updated": (G.KINDS, _keep_advances),
    "inactive_count_advanced": (("adam",), _wrap("advances", lambda o: lambda active: True)),
    "shared_step_count": (("adam",), _wrap("shared_counts", lambda o: lambda counts:
                                           {k: max(counts.values()) for k in counts})),
    "eps_inside_sqrt": (("adam",), _adam1(lambda v, c2, eps: np.sqrt(v + eps) * c2)),
    "c2_divides": (("adam",), _adam1(lambda v, c2, eps: np.sqrt(v) / c2 + eps)),
    "one_minus_float32_beta": (("adam",), _wrap("adam_consts", lambda o: lambda b1, b2, eps:
                                                F.AdamK(f32(b1), f32(1.0 - float(f32(b1))),
                                                        f32(b2), f32(1.0 - float(f32(b2))),
                                                        f32(eps)))),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_mutation_is_killed(name, monkeypatch):
    kinds, apply = MUTATIONS[name]
    base = {(c.name, k): baseline(c, k) for c in G.CASES for k in kinds}
    apply(monkeypatch)
    killers = [f"{c.name}-{k}" for c in G.CASES for k in kinds
               if _bits(G.run_expected(c, k)) != base[(c.name, k)]]
    print(f"MUTATION {name}: killed by {len(killers)} of {len(base)}: {' '.join(killers)}")
    assert killers, f"no case sees {name}: a case is missing"


def test_min_form_of_the_clip_scale_is_the_same_function():
    """min(1, clip / total) in place of clip / fmaxf(total, clip) is no defect: float32
    division is correctly rounded and monotone, so for total > clip the quotient is
    clip / total on both sides (never above 1), and for total <= clip, total = 0 included,
    both give exactly 1 (clip / clip, against min(1, q) with q >= 1 or q = inf).  No input can
    tell the two apart, so no case can kill it; checked here on every case's norms and on
    the neighbours of total = clip, and the killable relative of it
    (torch.nn.utils.clip_grad_norm_'s clip / (total + 1e-6), clamped) is in MUTATIONS."""
    def min_form(total, clip):
        with np.errstate(divide="ignore", over="ignore"):
            return min(f32(1), f32(clip) / f32(total)) if clip > 0 else f32(1)
    pairs = []
    for case in G.CASES:
        rp = G.Replay(case, "sgd")
        for s in range(case.nsteps):
            pairs.append((rp.step(s)[0].total, f32(case.clip)))
    for clip in (f32(1e-3), f32(0.75), f32(10), f32(1e4)):
        x = clip
        for _ in range(3):
            x = np.nextafter(x, f32(np.inf))
            pairs.append((x, clip))
        x = clip
        for _ in range(3):
            x = np.nextafter(x, f32(0))
            pairs.append((x, clip))
        pairs += [(clip, clip), (f32(0), clip), (f32(F.TINY), clip), (f32(3e38), clip),
                  (f32(np.inf), clip)]
    assert len(pairs) > 100
    for total, clip in pairs:
        assert F.clip_scale(total, clip).tobytes() == min_form(total, clip).tobytes(), \
            (total, clip)


def test_truth_is_shared_with_the_adam_tests():
    import test_adam_gpu
    assert test_adam_gpu.Truth is F.Truth and test_adam_gpu.check_bar is F.check_bar
