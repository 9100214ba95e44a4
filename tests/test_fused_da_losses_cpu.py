"""The restatements and truths of tests/fused_da_losses.py are right, and the cases
tests/test_fused_da_losses_gpu.py holds the device to can see what they should, without a GPU
(the case list is imported, so the two cannot drift apart).

  truth        for every case the restatement (the kernel's own order, numpy's libm) passes the
               very check the device gets; the truths agree with the project's torch
               compositions run in float64 (tlod.da.idf.domain_losses_torch, tests/ref_idf.py's
               focal_loss and cross_entropy2, tests/ref_selftrain.py's efocal_loss,
               tlod.da.us_daf.bce_margin, tests/ref_us_daf.py's da_losses_from_sigmoid,
               tests/ref_pt_maf.py's masked_nll, _kd_ref of tests/test_pt_maf_ops_gpu.py,
               tlod.da.pa_atf.losses_torch, tlod.da.idf.dam_torch / separation_torch and
               tests/ref_idf.py's dam and distance) and,
               where mpmath imports, with mpmath at 80 digits to 2^-48 (every row of the domain
               losses; up to 4096 logits a tensor of the US-DAF sigmoids and the rest in
               np.longdouble; up to 150 rows a case of the KD loss, the planted ones among
               them; up to 200 rows a PA-ATF term; every pixel of the IDF maps);
  conditions   no rounded-once truth is within 2^-45 of a float32 tie, no focal p within 2^-45
               of the clamp's midpoint, every gate element loss is 16 u or more from 0.5 (from
               the mpmath values where it imports, float64 and np.longdouble otherwise); no
               rounded-once bar exceeds half an ulp plus 2^-40 of its scale and no bounded bar
               16 u of its scale;
  sensitivity  each defect of MUTATIONS, put into the restatement, fails that same check in at
               least one case (run with -s for the cases that catch each); and for a second
               sweep that is never written, a wrong sign on every element below 2e-5 of the
               largest and a KD normaliser that counts the weights once per row, a case that
               tests/test_losses_gpu.close passes and the new check fails.

Who catches what (48 cases): the clamp defects (`<=`, the double 1e-6, no clamp) the five focal
cases with the planted clamp rows; a swapped logit column all eleven domain-loss cases; the
unguarded q = 0 focal_gamma_half alone; NEAR_0 dropped from the backward, the divisor n, the
gate on every column, a shifted scale label, `<` at 400 and area + 1 all six US-DAF cases; the
gate at 0.49 edge1025 and seam (the planted +-0.4375); the unclamped divisor `one` (no target
rows); the log clamp and the 1e-12 floor the five cases with saturated logits; the US-DAF
second sweep seam alone, masked_nll2's the two 113 x 145 cases, the KD backward's `cap` alone;
the KD forward's one stride the six cases past 1024 rows; the per-row normaliser the four RPN
cases; 1 / T dropped the seven cases with T = 3; every PA-ATF defect (n - label, the zeros
counted as n, the clamp or the switch removed, the switch at 99, the CLUB column) all three
PA-ATF cases; every DAM / separation defect (`<=`, a threshold over the batch, a map
modulated by its own attention or without the one, +t for g_b, a sum for the mean, eps
dropped) all seven IDF cases, the mean the six past one pixel, and eps as a float32 the two
whose gradient is the distance term alone.

The focal compositions clamp the float64 softmax at the double 1e-6 where the kernel clamps
the float32 one at 1e-6f (3e-9 apart): the focal loss is compared at 1e-8 and rows within 1e-8
of the clamp are left out of that comparison (they are what the clamp cases are for).
da_losses_from_sigmoid and bce_margin start from the float32 sigmoid the kernel saves; they
add NEAR_0 in float64 where the kernel adds it in float32, so they agree to 1e-6.
"""
import math

import numpy as np
import pytest
import torch

import fused_da_losses as D
import test_fused_da_losses_gpu as G
from test_losses_gpu import close

f32 = np.float32
_BASE = {}


def baseline(fam, case):
    if (fam, case) not in _BASE:
        _BASE[(fam, case)] = (G.expected(fam, case), G.truth(fam, case))
    return _BASE[(fam, case)]


def _cases(fam):
    return pytest.mark.parametrize("case", G.FAMILIES[fam].cases, ids=lambda c: c.name)


# ------------------------------------------------------------------ truth and conditions
@pytest.mark.parametrize("fam,case", G.ALL, ids=G.ALL_IDS)
def test_restatement_within_its_bars(fam, case):
    exp, tru = baseline(fam, case)
    bad, fig = G.check(fam, case, exp, exp, tru)
    G._report(fam, case, fig, "restatement")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("fam,case", G.ALL, ids=G.ALL_IDS)
def test_caps(fam, case):
    _, tru = baseline(fam, case)
    once, bounded = G.FAMILIES[fam].caps(case, tru)
    for name, t, bar, scale in once:
        cap = D.half_ulp32(t) + D.RCAP * np.asarray(scale)
        assert np.all(np.asarray(bar) <= cap * (1 + 1e-12)), name
    for name, t, bar, scale in bounded:
        assert np.all(np.asarray(bar) <= D.CAP * np.asarray(scale) * (1 + 1e-9) + D.TINY), name
    assert once or bounded


@_cases("dl")
def test_dl_ties(case):
    i = G.dl_inputs(case)
    img, ins = G.dl_tie_rows(i)
    assert img.size == 0 and ins.size == 0
    if not case.ef and case.R >= 16:  # the clamp rows are there, on both sides and on 1e-6f
        p, _, _ = D._pq(D._x(i["z_ins"], case.label_ins))
        p32 = p.astype(np.float32)
        near = np.abs(p / 1e-6 - 1) < 1e-5
        assert (p32[near] < f32(1e-6)).sum() >= 3 and (p32[near] > f32(1e-6)).sum() >= 3
        assert (p32 == f32(1e-6)).sum() == 1


@_cases("us")
def test_us_ties_and_gate_margin(case):
    i = G.us_inputs(case)
    assert not any(b.size for b in G.us_tie_elems(i))
    _, tru = baseline("us", case)
    for tag in "st":
        e0 = tru["e0_" + tag]
        assert e0.size == 0 or D.gate_margin(e0).min() >= 16
        if e0.size >= 12 and not case.gated:  # some rows gated on and some off
            assert 0 < tru["gate_" + tag].sum() < e0.size
    exp, _ = baseline("us", case)
    for tag in "st":  # the restated gate and s are the truth's
        assert np.array_equal(exp["gate_" + tag], tru["gate_" + tag].astype(np.float32))
        for k in ("s_img_", "s_ins_"):
            assert G._bytes(exp[k + tag]) == G._bytes(tru[k + tag][0].astype(np.float32))


def test_cases_reach_what_they_name():
    by = {c.name: c for c in G.US_CASES}
    c = by["seam"]
    assert c.Bs * c.Hs * c.Ws + 4 * c.ns == 262148 > 1024 * 256
    assert c.Bt * c.Ht * c.Wt + 4 * c.nt != 262148
    exp, _ = baseline("us", by["edge1025"])
    s = np.concatenate([exp["s_img_s"], exp["s_ins_t"].ravel()])
    assert (s == 0).any() and (s == 1).any()
    assert ((s > 0) & (s < D.TINY)).any()  # the subnormal sigmoid of -90
    lab = D.scale_labels(G.us_inputs(by["edge1025"])["roiss"][1])
    assert lab.sum(0).min() >= 2 and np.all(lab.sum(1) == 1)
    area = lambda w, h: f32(w) * f32(h)
    assert area(20, 20.000002) > 400 > area(20, 19.999998) and area(100, 99.99999) < 10000
    c = next(c for c in G.NLL_CASES if c.name == "cap_two_cells")
    assert c.H * c.W == 64 * 256 + 1
    assert list(np.flatnonzero(G.nll_inputs(c)["maps"][0].ravel())) == [16383, 16384]
    for c in G.NLL_CASES:
        i = G.nll_inputs(c)
        assert c.K == 1 or i["scores"][1] is i["scores"][0]
    kinds = {G.KINDS[(k + b + len(c.name)) % 5] for c in G.NLL_CASES if c.maps == "mixed"
             for k in range(c.K) for b in range(c.B)}
    assert kinds == set(G.KINDS)


# ------------------------------------------------------------------ mpmath
def _mp():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 80
    return mp


def _agree(t, ref, what, tol=2.0 ** -48, floor=0.0):
    t = np.asarray(t, np.float64).ravel()
    for a, b in zip(t, ref):
        assert abs(a - b) <= tol * abs(b) + floor, (what, a, float(b))


def _mp_tie_free(mp, ref, what):
    for b in ref:
        b = abs(b)
        if b == 0:
            continue
        e = max(int(mp.floor(mp.log(b, 2))) - 23, -149)
        frac = mp.frac(b / mp.mpf(2) ** e)
        assert abs(frac - mp.mpf(1) / 2) * mp.mpf(2) ** e > mp.mpf(2) ** -45 * b, (what, float(b))


@_cases("dl")
def test_dl_truth_is_mpmath(case):
    mp = _mp()
    i, (_, tru) = G.dl_inputs(case), baseline("dl", case)
    g = [mp.mpf(float(f32(x))) for x in case.gloss]
    gamma = mp.mpf(case.gamma)

    def xs(z, label):
        return [mp.mpf(float(r[1 - label])) - mp.mpf(float(r[label])) for r in z]
    x = xs(i["z_img"], case.label_img)
    ce = [mp.log1p(mp.exp(v)) for v in x]
    dz = [g[k] * (-1 / (1 + mp.exp(-v))) for k, v in enumerate(x)]
    _agree(tru["ce"][0], ce, "ce")
    _agree(tru["dz_img"][0][:, case.label_img], dz, "dz_img")
    _mp_tie_free(mp, ce, "ce")
    _mp_tie_free(mp, dz, "dz_img")
    gr = g[case.n_img] / case.R
    terms, dzn = [], []
    mid = mp.mpf(D.clamp_midpoint())
    for v in xs(i["z_ins"], case.label_ins):
        p, q, lp = 1 / (1 + mp.exp(v)), 1 / (1 + mp.exp(-v)), -mp.log1p(mp.exp(v))
        if case.ef:
            terms.append(-mp.exp(-gamma * p) * lp)
            dzn.append(gr * mp.exp(-gamma * p) * (gamma * p * lp - 1) * q)
            continue
        assert abs(p - mid) > mp.mpf(2) ** -45 * mid
        if p < mid:
            c = mp.mpf(float(f32(1e-6)))
            terms.append(-(1 - c) ** gamma * mp.log(c))
            dzn.append(mp.mpf(0))
        else:
            terms.append(-q ** gamma * lp)
            dzn.append(gr * (gamma * q ** gamma * p * lp - q ** (gamma + 1)))
    _agree(tru["terms"], terms, "terms")
    _agree(tru["dz_ins"][0][:, case.label_ins], dzn, "dz_ins")
    _mp_tie_free(mp, dzn, "dz_ins")
    assert (tru["exact"]["dz_ins"][0][:, 0] == np.array([d == 0 for d in dzn])).all()
    assert float(tru["focal"]) == float(f32(float(mp.fsum(terms) / case.R)))


@_cases("us")
def test_us_sigmoid_truth_is_mpmath(case):
    """mpmath for up to 4096 logits of each tensor (the planted ones are first and last); the
    rest of the 512 x 512 map in np.longdouble."""
    mp = _mp()
    i, (_, tru) = G.us_inputs(case), baseline("us", case)
    for dom, tag in enumerate("st"):
        for name, z in (("s_img_", i["z_imgs"][dom]), ("s_ins_", i["z_inss"][dom])):
            z, t = z.ravel(), tru[name + tag][0].ravel()
            pick = np.arange(z.size) if z.size <= 4096 else np.r_[0:2048, z.size - 2048:z.size]
            ref = [1 / (1 + mp.exp(-mp.mpf(float(v)))) for v in z[pick]]
            _agree(t[pick], ref, name + tag)
            _mp_tie_free(mp, ref, name + tag)
            zl = z.astype(np.longdouble)
            el = np.exp(-np.abs(zl))
            sl = np.where(zl >= 0, 1 / (1 + el), el / (1 + el))
            assert np.all(np.abs(t - sl) <= 2.0 ** -48 * sl)
        e0 = tru["e0_" + tag]
        s0 = tru["s_ins_" + tag][0][:, 0].astype(np.float32) if e0.size else []
        for k, s in enumerate(s0):  # the gate's element loss, from the float32 operand
            op = f32(s) + f32(1e-10) if dom == 0 else (f32(1) - f32(s)) + f32(1e-10)
            ref = -mp.log(mp.mpf(float(op)))
            assert abs(e0[k] - ref) <= 2.0 ** -48 * abs(ref) + 1e-300
            assert abs(ref - mp.mpf(1) / 2) >= 16 * D.U


# ------------------------------------------------------------------ the torch compositions
def _t64(a, grad=False):
    t = torch.from_numpy(np.asarray(a, np.float64).copy())
    return t.requires_grad_(True) if grad else t


def _near(a, b, what, rel, scale):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64).reshape(np.shape(a))
    err = np.abs(a - b)
    assert np.all(err <= rel * (np.abs(b) + scale)), (what, float(err.max()))


@_cases("dl")
def test_dl_truth_is_the_torch_composition(case):
    import ref_idf
    import ref_selftrain
    from tlod.da.idf import domain_losses_torch
    i, (_, tru) = G.dl_inputs(case), baseline("dl", case)
    zi, zn = _t64(i["z_img"], True), _t64(i["z_ins"], True)
    loss = domain_losses_torch(zi, case.label_img, zn, case.label_ins, case.gamma, case.ef)
    (loss * _t64(np.array(case.gloss, np.float32))).sum().backward()
    n = case.n_img
    focal = math.fsum(tru["terms"]) / case.R
    _near(tru["ce"][0], loss[:n].detach().numpy(), "ce", 1e-12, 1.0)
    # a loss is judged on max(1, |term|): torch's log(softmax) parts ways with log1p below 1e-16
    _near(focal, loss[n].item(), "focal", 1e-12 if case.ef else 1e-8, 1.0)
    other = (ref_selftrain.efocal_loss if case.ef else ref_idf.focal_loss)(
        zn.detach(), case.label_ins, case.gamma)
    _near(focal, other.item(), "focal (tests/ref_*)", 1e-12 if case.ef else 1e-8, 1.0)
    for k in range(n):
        _near(tru["ce"][0][k], ref_idf.cross_entropy2(zi[k:k + 1].detach(), case.label_img)
              .item(), "ce (ref_idf)", 1e-12, 1.0)
    g = np.abs(np.asarray(case.gloss, np.float64))
    _near(tru["dz_img"][0], zi.grad.numpy(), "dz_img", 1e-12, g[:n, None])
    p, _, _ = D._pq(D._x(i["z_ins"], case.label_ins))
    keep = case.ef | (np.abs(p / 1e-6 - 1) > 1e-8)
    if case.gamma < 1:  # the composition's own inf * 0 where 1 - p is 0 in double
        dead = 1.0 - p == 0.0
        assert dead.any() and np.isnan(zn.grad.numpy()[dead]).all()
        assert np.all(np.abs(tru["dz_ins"][0][dead]) < 1e-20 * g[n] / case.R)
        keep &= ~dead
    _near(tru["dz_ins"][0][keep], zn.grad.numpy()[keep], "dz_ins", 1e-12, g[n] / case.R)


@_cases("us")
def test_us_truth_is_the_torch_composition(case):
    import ref_us_daf
    from tlod.da.us_daf import bce_margin
    i, (exp, tru) = G.us_inputs(case), baseline("us", case)
    loss = tru["loss"][0]
    for dom, tag in enumerate("st"):
        y = 1.0 - dom
        si, sn = _t64(exp["s_img_" + tag], True), _t64(exp["s_ins_" + tag], True)
        gate = None if i["gates_in"] is None else _t64(i["gates_in"][dom])
        rois = torch.from_numpy(i["roiss"][dom])
        n = sn.shape[0]
        if n == 0:  # the composition cannot take an empty head; the fused contract is 0
            img = torch.nn.BCELoss()(si.reshape(-1, 1), torch.full_like(si, y).reshape(-1, 1))
            _near(loss[2 * dom], img.item(), "img loss", 1e-6, 0.0)
            assert loss[2 * dom + 1] == 0.0 and exp["loss"][2 * dom + 1] == 0.0
            continue
        img, ins, own, col0 = ref_us_daf.da_losses_from_sigmoid(si, y, sn, rois, gate)
        _near(loss[2 * dom], img.item(), "img loss", 1e-6, 0.0)
        _near(loss[2 * dom + 1], ins.item(), "ins loss", 1e-6, 0.0)
        # s + NEAR_0 rounds to s in float32 from s = 2^-9 up: an absolute 6e-8 at s = 1
        _near(tru["e0_" + tag], col0.numpy(), "e0", 1e-6, 0.1)
        if gate is None:
            assert np.array_equal(own.numpy(), tru["gate_" + tag])
        lab = torch.cat([torch.full((n, 1), y), torch.from_numpy(D.scale_labels(i["roiss"][dom]))],
                        1).double()
        assert torch.equal(lab[:, 1:].float(), ref_us_daf.scale_labels(rois).float())
        ins2, a = bce_margin(sn, lab, gate)
        _near(ins.item(), ins2.item(), "bce_margin", 1e-14, 0.0)
        # the exact backward against autograd through the same compositions
        (case.gloss[2 * dom] * img + case.gloss[2 * dom + 1] * ins2).backward()
        s64 = sn.detach().numpy()
        p64 = si.detach().numpy()
        gi, gn = case.gloss[2 * dom] / p64.size, case.gloss[2 * dom + 1] / (4 * n)
        _near(exp["dz_ins_" + tag], sn.grad.numpy() * s64 * (1 - s64), "dz_ins", 2e-6,
              1e-7 * abs(gn))
        _near(exp["dz_img_" + tag], si.grad.numpy() * p64 * (1 - p64), "dz_img", 2e-6,
              1e-7 * abs(gi))


@_cases("nll")
def test_nll_truth_is_the_torch_composition(case):
    import ref_pt_maf
    i, (exp, tru) = G.nll_inputs(case), baseline("nll", case)
    HW = case.H * case.W
    for k in range(case.K):
        for b in range(case.B):
            s = _t64(i["scores"][k][b:b + 1], True)
            cells = torch.from_numpy(i["maps"][k][b:b + 1])
            ref = ref_pt_maf.masked_nll(s, int(i["need"][b]), cells)
            (float(i["gout"][k, b]) * ref).backward()
            t = tru["loss"][0][k, b]
            assert abs(t - ref.item()) <= 1e-12 * max(1.0, abs(t))
            g = tru["dscore"][0][k, b]
            # the truth divides by the kernel's float32 g = gout / count
            _near(g, s.grad.numpy().reshape(2, HW), "dscore", 1e-6, 1e-14)
            assert exp["count"][k, b] == float(cells.sum())
            if int(cells.sum()) == 0:
                assert t == 0 and not g.any() and exp["loss"][k, b] == 0


def _kd_rows(case):
    """(student, teacher) as (R, C) float32 rows, whatever the case's layout."""
    i = G.kd_inputs(case)
    idx = np.arange(i["R"])[:, None] * i["rs"] + np.arange(i["C"])[None, :] * i["cs"]
    return i, i["student"].ravel()[idx], i["teacher"].ravel()[idx], idx


@_cases("kd")
def test_kd_truth_is_the_torch_composition(case):
    """_kd_ref's p1 log(p1 / p2) in float64 carries an absolute 1e-16 per class, so the loss is
    judged on max(1, |term|) and the gradient on its scale; a 0 / 0 of the composition (both
    softmaxes 0 in double) only arises in the planted e^-104 rows, which are left to mpmath."""
    from test_pt_maf_ops_gpu import _kd_ref
    i, (_, tru) = G.kd_inputs(case), baseline("kd", case)
    s, t = torch.from_numpy(i["student"]), torch.from_numpy(i["teacher"])
    if case.form == "rpn":
        sref, ref = _kd_ref(s, t, torch.from_numpy(i["weight"].reshape(case.H, case.W)), case.T,
                            (case.A, case.H, case.W))
    else:
        sref, ref = _kd_ref(s, t, torch.from_numpy(i["weight"]), case.T)
    (ref * case.gout).backward()
    out, _, scale = tru["out"]
    assert abs(out[0] - ref.item()) <= 1e-12 * max(1.0, abs(out[0]), scale[0])
    d, _, sc = tru["dstudent"]
    # the truth divides by the float32 normaliser the kernel saved
    ratio = float(f32(out[1])) / out[1]
    got, want = d * ratio, sref.grad.numpy().ravel()
    ok = np.isfinite(want)
    assert ok.mean() > 0.99
    assert np.all(np.abs(got - want)[ok] <= 1e-11 * (np.abs(want[ok]) + sc[ok]) + 1e-300)


@_cases("kd")
def test_kd_truth_is_mpmath(case):
    """Up to 150 rows of each case in mpmath (the planted rows are the first five and the
    last), and the loss of the cases of at most 2200 rows."""
    mp = _mp()
    i, S, Tt, idx = _kd_rows(case)
    _, tru = baseline("kd", case)
    R, C, T = i["R"], i["C"], mp.mpf(float(f32(case.T)))
    w = i["weight"].ravel()[np.arange(R) % i["wmod"]]
    N = mp.fsum(mp.mpf(float(x)) for x in i["weight"].ravel()[:min(R, i["wmod"])]) + 1
    g = mp.mpf(case.gout) / mp.mpf(float(f32(float(N)))) / T
    rows = np.arange(R) if R <= 2200 else np.r_[0:75, R - 75:R]
    d, _, sc = tru["dstudent"]
    total = mp.mpf(0)
    for r in rows if R <= 2200 else rows[:150]:
        z1 = [mp.mpf(float(v)) / T for v in S[r]]
        z2 = [mp.mpf(float(v)) / T for v in Tt[r]]
        lse1 = mp.log(mp.fsum(mp.exp(v) for v in z1))
        lse2 = mp.log(mp.fsum(mp.exp(v) for v in z2))
        l1, l2 = [v - lse1 for v in z1], [v - lse2 for v in z2]
        kl = mp.fsum(mp.exp(a) * (a - b) for a, b in zip(l1, l2))
        total += mp.mpf(float(w[r])) * kl
        assert abs(tru["kl"][r] - kl) <= 2.0 ** -48 * abs(kl) + 2.0 ** -70, (r, float(kl))
        ref = [g * mp.mpf(float(w[r])) * mp.exp(a) * ((a - b) - kl) for a, b in zip(l1, l2)]
        # 2^-48 of the element, or 2^-60 of the scale where the factor itself cancels
        for c in range(C):
            k = idx[r, c]
            assert abs(d[k] - ref[c]) <= 2.0 ** -48 * abs(ref[c]) + 2.0 ** -60 * sc[k], (r, c)
        if w[r] != 0:
            _mp_tie_free(mp, ref, f"dstudent row {r}")
    assert abs(tru["out"][0][1] - N) <= 2.0 ** -48 * N
    _mp_tie_free(mp, [N], "sum w + 1")
    if R <= 2200:
        loss = total / N
        assert abs(tru["out"][0][0] - loss) <= 2.0 ** -48 * abs(loss) + 1e-300
        _mp_tie_free(mp, [loss], "loss")


def test_kd_cases_reach_what_they_name():
    for case in G.KD_CASES:
        i, S, Tt, _ = _kd_rows(case)
        _, tru = baseline("kd", case)
        assert D.tie_margin(tru["out"][0]).min() >= G.TIE
        assert not ((D.tie_margin(tru["dstudent"][0]) < G.TIE) & ~tru["zeros"]).any()
        if case.name == "equal":
            assert np.array_equal(S, Tt) and tru["out"][0][0] == 0 and not tru["dstudent"][0].any()
        elif case.R >= 64:
            assert np.array_equal(S[1], Tt[1]) and (S[2] != Tt[2]).sum() == 1
            assert G.ulps(S[2], Tt[2]).max() <= 1 and tru["kl"][4] > 10
    cap = next(c for c in G.KD_CASES if c.name == "cap")
    i = G.kd_inputs(cap)
    assert cap.R == 1024 * 256 + 1 and i["weight"][-1] == 1


def test_normaliser_per_row_passes_close_and_fails_the_bar(monkeypatch):
    """sum w counted once per row (9 anchors share each weight) instead of once per weight:
    with one weight of 2^-19 the loss and the gradient move by 1.5e-5, under close's 2e-5."""
    case = next(c for c in G.KD_CASES if c.name == "rpn_one_small_weight")
    exp, tru = baseline("kd", case)
    monkeypatch.setattr(D, "kd_norm_rows", lambda R, wmod: np.arange(R))
    got = G.expected("kd", case)
    assert got["out"][0] != exp["out"][0]
    assert _close_passes(got["out"][:1], exp["out"][:1])
    assert _close_passes(got["dstudent"], exp["dstudent"])
    bad, _ = G.check("kd", case, got, exp, tru)
    assert len(bad) == 2


# ------------------------------------------------------------------ PA-ATF
@_cases("pa")
def test_pa_cases_reach_what_they_name(case):
    i, (exp, tru) = G.pa_inputs(case), baseline("pa", case)
    n = list(case.n)
    assert n.count(max(n)) == 1 and max(n) == 1025
    for k in range(D.PA_TERMS):  # no rounded-once gradient near a float32 tie
        v, _, _ = tru["dz"][k]
        assert not ((D.tie_margin(v) < G.TIE) & ~tru["exact"][k][0]).any()
    past = [tru["exact"][k][0].sum() for k in range(D.PA_IMG)]
    assert sum(past) >= 8  # +-100.5 and +-745 under both labels, at both ends
    for k, ones in zip((D.PA_IMG, D.PA_IMG + 1), case.ones):
        dead = 2 * ones == n[k]
        assert tru["exact"][k][0].all() == dead and (not dead or not exp["dz"][k].any())
    assert i["gloss"][case.gloss_zero] == 0


def test_pa_ones_cover_the_list():
    seen = set()
    for c in G.PA_CASES:
        for n, ones in zip(c.n[D.PA_IMG:D.PA_IMG + D.PA_INS], c.ones):
            seen |= {k for k, v in (("0", 0), ("1", 1), ("n-1", n - 1), ("n", n), ("n/2", n / 2))
                     if ones == v}
    assert seen == {"0", "1", "n-1", "n", "n/2"}
    assert {c.gloss_zero < D.PA_IMG for c in G.PA_CASES} == {True, False}


@_cases("pa")
def test_pa_truth_is_the_torch_composition(case):
    """losses_torch in float64.  Its sigmoid is 1.0 from 37 up, so its BCE reads the clamp's
    100 at a logit of 99.5 where the kernel's softplus reads 99.5, and its backward floors
    p (1 - p) at 1e-12, which bites from 27.6 up: the planted image logits of +-40 and +-99.5
    are moved to +-20 for this comparison (both sides then compute the same thing); +-100.5 and
    +-745, where both give the clamp and a zero gradient, stay."""
    from tlod.da.pa_atf import losses_torch
    i = G.pa_inputs(case)
    z = [x.copy() for x in i["z"]]
    for x in z[:D.PA_IMG]:
        far = (np.abs(x) > 25) & (np.abs(x) <= 100)
        x[far] = np.sign(x[far]) * 20
    tru = D.pa_atf_truth(z, i["n"], i["label"], i["gloss"])
    zt = [_t64(x, True) for x in z]
    a, b = D.PA_IMG, D.PA_IMG + D.PA_INS
    ref = losses_torch(zt[:a], list(case.img_labels), zt[a:b], list(case.ones), zt[b:],
                       list(case.club_labels))
    (ref * _t64(i["gloss"])).sum().backward()
    for k in range(D.PA_TERMS):
        assert abs(float(tru["loss"][k]) - ref[k].item()) <= 2.0 ** -23 * max(1, ref[k].item())
        v, _, sc = tru["dz"][k]
        _near(v, zt[k].grad.numpy(), f"dz[{k}]", 1e-12, sc)


@_cases("pa")
def test_pa_truth_is_mpmath(case):
    mp = _mp()
    i, (_, tru) = G.pa_inputs(case), baseline("pa", case)
    for k in range(D.PA_TERMS):
        n, lab = case.n[k], i["label"][k]
        g = mp.mpf(float(i["gloss"][k])) / n
        v = tru["dz"][k][0].reshape(n, -1)
        x = i["z"][k].reshape(n, -1)[:200]
        ref = []
        for r, row in enumerate(x):
            if k < D.PA_IMG:
                u = -mp.mpf(float(row[0])) if lab else mp.mpf(float(row[0]))
                live = mp.log1p(mp.exp(u)) < 100
                assert abs(mp.log1p(mp.exp(u)) - 100) > mp.mpf(2) ** -20
                ref.append((-1 if lab else 1) * g / (1 + mp.exp(-u)) if live else mp.mpf(0))
            elif k < D.PA_IMG + D.PA_INS:
                s = 1 / (1 + mp.exp(-mp.mpf(float(row[0]))))
                ref.append(g * (n - 2 * lab) / n * s * (1 - s))
            else:
                xx = mp.mpf(float(row[1 - lab])) - mp.mpf(float(row[lab]))
                ref.append(-g / (1 + mp.exp(-xx)))
        col = lab if k >= D.PA_IMG + D.PA_INS else 0
        _agree(v[:200, col], ref, f"dz[{k}]", floor=1e-300)
        _mp_tie_free(mp, ref, f"dz[{k}]")


# ------------------------------------------------------------------ IDF DAM / separation
@_cases("sep")
def test_sep_cases_reach_what_they_name(case):
    i, (exp, tru) = G.sep_inputs(case), baseline("sep", case)
    assert not any(v.size for v in G.sep_tie_elems(i))
    N, C, P = i["x"].shape
    # the constant map: avg == thr in every pixel, everything kept; image 0 drops some
    assert (exp["att"][1] != 0).all() and len(set(exp["att"][1].tolist())) == 1
    assert np.array_equal(tru["thr"][0][1].astype(np.float32), exp["att"][1][0])
    assert P == 1 or ((exp["att"][0] == 0).any() and (exp["att"][0] != 0).any())
    assert case.C in (1, 15, 16, 17, 33) and P in (1, 63, 64, 65, 129)
    if P >= 63:
        d = tru["d"][0]
        assert np.allclose(d[:, 1], np.sqrt(C) * 1e-6, rtol=1e-12)     # a == b
        assert np.allclose(d[:, 2], np.sqrt(C) * 1e-6, rtol=1e-12)     # zero attention
        e = (i["a"].astype(np.float64) - i["b"]) * i["att_b"][:, None, :] + 1e-6
        assert (e[:, :5, 0] > 0).any() and (e[:, :5, 0] < 0).any()     # e crosses zero
        assert np.abs(e[:, :5, 0]).max() < 1e-7  # a - b rounds in float32
        zero_w = i["att_b"] == 0
        if case.mode == "zero_up":
            assert tru["zeros"].any() and not exp["g_a"][tru["zeros"]].any()
        elif case.mode == "mod":  # the distance term is exactly 0: g_a is g_a_out (1 + 0)
            assert np.array_equal(exp["g_a"].transpose(0, 2, 1)[zero_w],
                                  i["g_a_out"].transpose(0, 2, 1)[zero_w])


@_cases("sep")
def test_sep_truth_is_the_torch_composition(case):
    import ref_idf
    from tlod.da.idf import dam_torch, separation_torch
    i, (exp, tru) = G.sep_inputs(case), baseline("sep", case)
    N, C, P = i["x"].shape
    r4 = lambda v, g=False: _t64(v.reshape(N, C, case.H, case.W), g)
    r3 = lambda v: _t64(v.reshape(N, case.H, case.W))
    x = r4(i["x"])
    avg = torch.sigmoid(x).mean(1).reshape(N, P).numpy()
    _near(tru["avg"][0], avg, "avg", 1e-13, 0.0)
    att = dam_torch(x).reshape(N, P).numpy()
    keep0 = (exp["att"][0] != 0)  # the constant image sits on its threshold: float64 decides
    assert np.array_equal(att[0] != 0, keep0)   # it by its own rounding, float32 keeps it
    for n in range(N):
        one = ref_idf.dam(x[n:n + 1]).reshape(P).numpy()
        assert np.array_equal(one, att[n])
    a, b = r4(i["a"], True), r4(i["b"], True)
    ao, bo, d, dist = separation_torch(a, b, r3(i["att_a"]), r3(i["att_b"]))
    _near(tru["d"][0], d.detach().reshape(N, P).numpy(), "d", 1e-9, 0.0)
    _near(tru["dist"][0], dist.detach().numpy(), "dist", 1e-9, 0.0)
    m = (i["a"] * (np.float32(1) + i["att_b"])[:, None, :]).astype(np.float32)
    assert G._bytes(exp["a_out"]) == G._bytes(m)
    f = separation_torch(a.detach().float(), b.detach().float(), r3(i["att_a"]).float(),
                         r3(i["att_b"]).float())
    assert G._bytes(exp["a_out"]) == G._bytes(f[0].reshape(N, C, P).numpy())
    assert G._bytes(exp["b_out"]) == G._bytes(f[1].reshape(N, C, P).numpy())
    loss = (dist * _t64(i["g_dist"])).sum()
    if case.mode != "dist":
        loss = loss + (ao * r4(i["g_a_out"])).sum() + (bo * r4(i["g_b_out"])).sum()
    loss.backward()
    # the truth divides by the float32 d the kernel saved: 6e-8 relative in the distance term
    for name, t in (("g_a", a), ("g_b", b)):
        v, _, sc = tru[name]
        _near(v, t.grad.reshape(N, C, P).numpy(), name, 1e-6, 1e-7 * sc)
    pd = separation_torch(a.detach(), b.detach(), None, None, modulate=False)[3]
    _near(tru["plain_dist"][0], pd.numpy(), "plain_dist", 1e-12, 0.0)
    for n in range(N):
        _near(tru["plain_dist"][0][n], ref_idf.distance(a[n:n + 1].detach(),
                                                        b[n:n + 1].detach()).item(),
              "plain_dist (ref_idf)", 1e-12, 0.0)


@_cases("sep")
def test_sep_truth_is_mpmath(case):
    """avg, thr, d, dist and both gradients of every pixel in mpmath."""
    mp = _mp()
    i, (_, tru) = G.sep_inputs(case), baseline("sep", case)
    N, C, P = i["x"].shape
    M = lambda v: mp.mpf(float(v))
    pix = list(range(P))
    for n in range(N):
        avgs = [mp.fsum(1 / (1 + mp.exp(-M(v))) for v in i["x"][n, :, p]) / C for p in pix]
        _agree(tru["avg"][0][n, pix], avgs, "avg")
        _mp_tie_free(mp, avgs, "avg")
        a32 = tru["avg"][0][n].astype(np.float32)
        thr = mp.fsum(M(v) for v in a32) / P
        _agree(tru["thr"][0][n:n + 1], [thr], "thr")
        _mp_tie_free(mp, [thr], "thr")
        ds = []
        for p in pix:
            w = M(i["att_b"][n, p])
            e = [(M(i["a"][n, c, p]) - M(i["b"][n, c, p])) * w + M(1e-6) for c in range(C)]
            d = mp.sqrt(mp.fsum(v * v for v in e))
            ds.append(d)
            d32 = M(np.float32(float(d)))
            k = M(i["g_dist"][n]) / P * w / d32
            for name, sgn, up, att in (("g_a", 1, "g_a_out", "att_b"), ("g_b", -1, "g_b_out",
                                                                       "att_a")):
                ref = [sgn * k * e[c] + (0 if i[up] is None else M(i[up][n, c, p])
                                        * (1 + M(i[att][n, p]))) for c in range(C)]
                v, _, sc = tru[name]
                for c in range(C):
                    assert abs(v[n, c, p] - ref[c]) <= 2.0 ** -48 * abs(ref[c]) \
                        + 2.0 ** -60 * sc[n, c, p], (name, n, c, p)
                _mp_tie_free(mp, [r for c, r in enumerate(ref)
                                  if not tru["zeros"][n, c, p]], name)
        _agree(tru["d"][0][n, pix], ds, "d")
        _mp_tie_free(mp, ds, "d")
        dist = mp.fsum(ds) / P
        _agree(tru["dist"][0][n:n + 1], [dist], "dist")
        _mp_tie_free(mp, [dist], "dist")


# ------------------------------------------------------------------ sensitivity
def _set(name, value):
    return lambda mp: mp.setattr(D, name, value)


def _labels_lt(rois):
    r = np.asarray(rois, np.float32).reshape(-1, 5)
    area = (r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2])
    return np.stack([area < 400, (area >= 400) & (area < 10000), area >= 10000],
                    1).astype(np.float32)


def _labels_plus_one(rois):
    r = np.asarray(rois, np.float32).reshape(-1, 5)
    area = (r[:, 3] - r[:, 1] + f32(1)) * (r[:, 4] - r[:, 2] + f32(1))
    return np.stack([area <= 400, (area > 400) & (area < 10000), area >= 10000],
                    1).astype(np.float32)


# name -> (the swap, the keyword the restatement takes with it)
MUTATIONS = {
    "clamp_le": (_set("clamp_test", lambda p32, c: p32 <= c), {}),
    "clamp_at_the_double_1e-6": (_set("P_FLOOR", np.float64(1e-6)), {}),
    "clamp_removed": (_set("clamp_test", lambda p32, c: np.zeros(p32.shape, bool)), {}),
    "label_column_for_the_other": (_set("other_logit", lambda label: label), {}),
    "q0_not_guarded": (_set("focal_q0", lambda q: np.zeros(q.shape, bool)), {}),
    "near0_dropped_from_the_backward": (_set("near0_bwd", lambda: f32(0)), {}),
    "near0_1e-9": (_set("NEAR_0", f32(1e-9)), {}),
    "gate_at_0.49": (_set("gate_test", lambda e0: e0 > f32(0.49)), {}),
    "divisor_n": (_set("ins_denom", lambda n: f32(max(n, 1))), {}),
    "divisor_not_clamped": (_set("ins_denom", lambda n: f32(4) * f32(n)), {}),
    "gate_on_every_column": (_set("gate_column", lambda c: c >= 0), {}),
    "scale_label_shifted": (_set("label_column", lambda c: c % 3), {}),
    "small_lt_400": (_set("scale_labels", _labels_lt), {}),
    "area_plus_one": (_set("scale_labels", _labels_plus_one), {}),
    "log_clamp_removed": (_set("LOG_CLAMP", f32(-np.inf)), {}),
    "grad_floor_removed": (_set("GRAD_FLOOR", f32(0)), {}),
    "us_second_sweep_unwritten": (_set("sweep_rows", lambda n: np.arange(min(n, 1024 * 256))),
                                  {"held": 0.0}),
    "nll_second_sweep_unwritten": (_set("cells_visited", lambda n: np.arange(min(n, 64 * 256))),
                                   {"held": 0.0}),
    "nll_count_plus_one": (_set("nll_count", lambda cells: cells + 1), {}),
    "nll_map_nonzero": (_set("on_map", lambda m: m >= 0), {}),
    "kd_normaliser_per_row": (_set("kd_norm_rows", lambda R, wmod: np.arange(R)), {}),
    "kd_normaliser_without_one": (_set("kd_norm_plus", lambda: 0.0), {}),
    "kd_weight_by_anchor": (_set("kd_weight_index", lambda r, wmod: (r // 9) % wmod), {}),
    "kd_forward_one_stride": (_set("kd_fwd_rows", lambda R: np.arange(min(R, 1024))), {}),
    "kd_second_sweep_unwritten": (_set("kd_bwd_rows", lambda R: np.arange(min(R, 1024 * 256))),
                                  {"held": 0.0}),
    "kd_gradient_without_1_over_T": (_set("kd_temperature_in_gradient", lambda T: 1.0), {}),
    "pa_n_minus_label": (_set("pa_ins_factor", lambda n, label: n - label), {}),
    "pa_zeros_counted_as_n": (_set("pa_ins_zeros", lambda n, label: n), {}),
    "pa_clamp_removed": (_set("PA_CLAMP", np.inf), {}),
    "pa_switch_removed": (_set("pa_switch", lambda sp: sp < np.inf), {}),
    "pa_switch_at_99": (_set("pa_switch", lambda sp: sp < 99.0), {}),
    "pa_club_other_column": (_set("pa_club_other", lambda label: label), {}),
    "dam_drop_le": (_set("dam_drop", lambda avg, thr: avg <= thr), {}),
    "dam_threshold_over_the_batch": (_set("dam_thr_images", lambda N: [list(range(N))] * N), {}),
    "modulated_by_its_own_attention": (_set("modulate", lambda a, att: a * (
        f32(1) + (att[::-1] if att.shape[1] == 1 else np.roll(att, 1, 1)))[:, None, :]), {}),
    "modulation_without_one": (_set("modulate", lambda a, att: a * att[:, None, :]), {}),
    "sep_b_gets_plus_t": (_set("sep_sign_b", lambda: 1.0), {}),
    "sep_mean_is_a_sum": (_set("sep_mean_over", lambda P: 1.0), {}),
    "sep_eps_dropped": (_set("SEP_EPS", 0.0), {}),
    "sep_eps_float32": (_set("SEP_EPS", float(f32(1e-6))), {}),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_mutation_is_killed(name, monkeypatch):
    base = {fc: baseline(*fc) for fc in G.ALL}
    swap, kw = MUTATIONS[name]
    swap(monkeypatch)
    killers = []
    for (fam, case), (exp, tru) in base.items():
        kws = kw if fam in ("us", "nll", "kd") else {}
        with np.errstate(all="ignore"):
            bad, _ = G.check(fam, case, G.expected(fam, case, **kws), exp, tru)
        if bad:
            killers.append(f"{fam}-{case.name}[{bad[0].split(':')[0]}]")
    print(f"MUTATION {name}: killed by {len(killers)} of {len(base)}: {' '.join(killers)}")
    assert killers, f"no case sees {name}: a case is missing"


def _close_passes(a, b):
    try:
        close(torch.from_numpy(np.asarray(a, np.float32)), torch.from_numpy(
            np.asarray(b, np.float32)))
    except AssertionError:
        return False
    return True


def test_unwritten_second_sweep_passes_close_and_fails_the_bar(monkeypatch):
    """masked_nll2_bwd without its grid stride leaves cell 16384 of a 113 x 145 map unwritten.
    In cap_two_cells that cell is decided by 20, so what it should hold is 2e-9 of the other
    cell's gradient: a buffer that held zeros passes close and fails the element's bar."""
    case = next(c for c in G.NLL_CASES if c.name == "cap_two_cells")
    exp, tru = baseline("nll", case)
    monkeypatch.setattr(D, "cells_visited", lambda n: np.arange(min(n, 64 * 256)))
    got = G.expected("nll", case, held=0.0)
    assert G._bytes(got["dscore"]) != G._bytes(exp["dscore"])
    assert _close_passes(got["dscore"], exp["dscore"]) and _close_passes(got["loss"], exp["loss"])
    bad, _ = G.check("nll", case, got, exp, tru)
    assert bad and bad[0].startswith("dscore")


@pytest.mark.parametrize("fam,name,out", [("dl", "focal_r513", "dz_ins"),
                                          ("dl", "efocal_r513", "dz_ins"),
                                          ("nll", "cap_full", "dscore")])
def test_wrong_sign_on_small_elements_passes_close_and_fails_the_bar(fam, name, out):
    case = next(c for c in G.FAMILIES[fam].cases if c.name == name)
    exp, tru = baseline(fam, case)
    got = dict(exp)
    small = np.abs(exp[out]) < 2e-5 / 2 * np.abs(exp[out]).max()
    assert (small & (exp[out] != 0)).sum() >= 4
    got[out] = np.where(small, -exp[out], exp[out])
    assert _close_passes(got[out], exp[out])
    bad, _ = G.check(fam, case, got, exp, tru)
    assert bad and bad[0].startswith(out)
