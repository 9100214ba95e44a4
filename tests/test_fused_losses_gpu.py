"""The fused RPN, RCNN and DAF losses (csrc/losses.hip, tlod.detector.losses) pinned to
tests/fused_losses.py through rpn_losses, rcnn_losses, daf_da_losses and
daf_da_losses_packed.

For every case:

  exact      dbbox, box_sel, dbox, every contract zero (ignored anchors, images
             B..B_total-1, rows R..R_total-1, every gradient when no anchor is kept, the
             losses of an empty domain, dcls under a zero upstream gradient) equal the numpy
             float32 restatement byte for byte (tobytes());
  1 ulp      the smooth-L1 loss scalars are within 1 float32 ulp of
             float32(fsum(terms) / denom) (equality is expected, see fused_losses.py);
  bounded    cls_prob, dscore, dcls, the CE / NLL / BCE losses, the consistency loss, dins
             and the image-level dscore are within their derived bar of the fp64 truth,
             element by element; no bar is looser than 16 u (u = 2^-24) times its scale;
  twice      a second run of the case gives identical bytes; the packed DA entry point gives
             the bytes of the split one.

The cases and their inputs are built in numpy without a GPU; tests/test_fused_losses_cpu.py
imports them to hold the restatement and the truth to the torch compositions and to show that
every plausible defect moves some expectation beyond its bar.

Measured on an MI355X (run with -s for every figure; worst over the cases, in u of the scale
and as a share of the derived bar, which assumes 2 ulp for expf and logf):

  quantity                      bar (worst case)             device worst       case
  RPN loss_cls                  11.3 u * mean max(1,|term|)  0.69 u  (0.25)     tail
  RPN dscore                    15.5 u * |gloss/count|       3.02 u  (0.77)     two_in_flight
  RCNN cls_prob, C = 9          <= 13 u of the element       4.37 u  (0.64)     agnostic37*
  RCNN cls_prob, C = 21         16 u of the element (cap)    6.94 u  (0.48)     second_stride
  RCNN cls_prob, two live       5.1 u of the element         (0.49 of the bar)  partial
  RCNN loss_cls                 16 u * mean max(1,|term|)    0.79 u  (0.35)     agnostic37
  RCNN dcls                     16 u * |gloss/R| (cap)       4.88 u  (0.64)     c21, agnostic37
  DA image NLL, BCE, cst loss   11.3 u / 6 u / 16 u * scale  0.67 u  (0.26)     needs_crossed
  DA image dscore               15.5 u * |gloss/npix|        2.24 u  (0.63)     packable
  DA dins                       7 u * scale + |2 gm| err(c)  0.96 u  (0.25)     two_source
  smooth-L1 loss scalars        1 ulp                        0 ulp, every case

Every exact piece matched bit for bit in every case, every case gave the same bytes twice, and
the packed DA entry point the bytes of the split one.  (rpn-one_row's loss_cls reads 0.98 of
its bar: the truth is log1p(e^-104) = 6.8e-46, the device's 0, the bar that term itself.)

Built with `<=` at the smooth-L1 cut the library fails rpn-sigma0.7 alone (dbbox), with
minibatch = 255 the three DA cases with a second block, with __expf for expf every RCNN case
from 37 rows up (cls_prob of the planted two-live rows) and rpn-two_in_flight (dscore);
tests/test_losses_gpu.py passes the first and the last.
"""
import zlib
from collections import namedtuple

import numpy as np
import pytest

import fused_losses as F

f32 = np.float32
U = F.U


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _n32(rng, shape, scale=1.0):
    return (scale * rng.standard_normal(shape)).astype(np.float32)


# logit pairs planted in kept rows / pixels: equal, signed zeros, differences of 20, 40 and 104
# either way (at 104 the loser's expf underflows to exactly 0: no subnormal), both near 1e4
PAIRS = [(1.5, 1.5), (0.0, -0.0), (-0.0, 0.0), (-0.25, 19.75), (19.75, -0.25), (0.5, 40.5),
         (40.5, 0.5), (-2.0, 102.0), (102.0, -2.0), (1e4, 1e4 - 0.75), (1e4 - 3.0, 1e4)]

# ------------------------------------------------------------------ RPN
RPN = namedtuple("RPN", "name B Bt A H W sigma labels")
RPN_CASES = [
    RPN("one_row", 1, 1, 1, 1, 1, 3.0, "all1"),
    RPN("two_images", 2, 2, 9, 5, 7, 3.0, "sampled"),       # 630 rows, image boundary at 315
    RPN("two_in_flight", 1, 1, 9, 13, 17, 3.0, "all0"),     # 1989 rows: u = 0, 1 only
    RPN("tail", 1, 1, 3, 37, 37, 3.0, "sampled"),           # 4107 = 4096 + 11
    RPN("tail_one_last", 1, 1, 3, 37, 37, 3.0, "one_last"),
    RPN("two_of_three", 2, 3, 3, 6, 5, 3.0, "sampled"),
    RPN("two_of_three_none", 2, 3, 3, 6, 5, 3.0, "none"),
    RPN("sigma1", 1, 1, 3, 4, 4, 1.0, "sampled"),           # the cut at exactly 1.0
    # at sigma 3 and 1 both branches give the same bits at |d| = cut (s2 * cut rounds to 1);
    # at 0.7 it is 1 - 2^-24, so which branch took the cut shows in dbbox
    RPN("sigma0.7", 1, 1, 3, 4, 4, 0.7, "all1"),
]
RPN_GLOSS = (2.0, 0.5)
_INPUTS = {}


def rpn_inputs(c):
    if c in _INPUTS:
        return _INPUTS[c]
    rng = _rng("rpn" + c.name)
    ahw = c.A * c.H * c.W
    rows = c.B * ahw
    score = _n32(rng, (c.Bt, 2 * c.A, c.H, c.W), 3.0)
    bbox = _n32(rng, (c.Bt, 4 * c.A, c.H, c.W))
    tgt = _n32(rng, (c.B, 4 * c.A, c.H, c.W), 0.3)
    inw = (rng.random(tgt.shape) < 0.3).astype(np.float32)
    outw = ((rng.random(tgt.shape) < 0.5) / 256.0).astype(np.float32)
    lab = rng.integers(0, 2, rows).astype(np.float32)
    if c.labels == "sampled":
        lab[rng.random(rows) < 0.9] = -1.0
        lab[0], lab[rows - 1], lab[rows - 3 if rows > 3 else 0] = 1.0, 0.0, 1.0
    elif c.labels in ("all1", "all0"):
        lab[:] = 1.0 if c.labels == "all1" else 0.0
    else:
        lab[:] = -1.0
        if c.labels == "one_last":
            lab[rows - 1] = 1.0
    kept = np.flatnonzero(lab != -1)
    sf = score.reshape(-1)
    shift = len(c.name)  # another part of the list first in each case
    for j, r in enumerate(kept[:len(PAIRS)]):
        b, q = divmod(int(r), ahw)
        a0, a1 = PAIRS[(j + shift) % len(PAIRS)]
        sf[b * 2 * ahw + q], sf[b * 2 * ahw + ahw + q] = a0, a1
    cut = f32(1) / F.sigma2(c.sigma)
    inside = np.nextafter(cut, f32(0))
    plants = [cut, -cut, inside, -inside, f32(0), np.nextafter(cut, f32(2) * cut)]
    bf, tf, iw, ow = bbox.reshape(-1), tgt.reshape(-1), inw.reshape(-1), outw.reshape(-1)
    n = min(len(plants), rows * 4)
    bf[:n], tf[:n], iw[:n], ow[:n] = plants[:n], 0.0, 1.0, 1.0 / 256
    _INPUTS[c] = dict(score=score, labels=lab.reshape(c.B, 1, c.A * c.H, c.W), bbox=bbox,
                           tgt=tgt, inw=inw, outw=outw, B=c.B, B_total=c.Bt, A=c.A, H=c.H,
                           W=c.W, sigma=c.sigma, gloss=RPN_GLOSS)
    return _INPUTS[c]


# ------------------------------------------------------------------ RCNN
RCNN = namedtuple("RCNN", "name R Rt C agnostic gloss", defaults=((1.0, 3.0),))
RCNN_CASES = [
    RCNN("one_row", 1, 1, 2, False),
    RCNN("agnostic37", 37, 37, 9, True),
    RCNN("agnostic37_box_only", 37, 37, 9, True, (None, 3.0)),  # _grad_pair's zero fill
    RCNN("partial", 256, 556, 9, False),
    RCNN("partial_agnostic", 256, 556, 9, True),
    RCNN("second_stride", 1025, 1025, 21, False),               # row 1024: thread 0 again
    RCNN("c21", 300, 300, 21, False),
]


def rcnn_inputs(c):
    if c in _INPUTS:
        return _INPUTS[c]
    rng = _rng("rcnn" + c.name)
    R, C = c.R, c.C
    bw = 4 if c.agnostic else 4 * C
    cls = _n32(rng, (c.Rt, C), 2.0)
    box = _n32(rng, (c.Rt, bw))
    lab = rng.integers(0, C, R)
    lab[0] = C - 1
    if R > 1:
        lab[1] = 0
    lab[R // 4:R // 2] = 0  # a block of background rows with zero weights
    tgt = _n32(rng, (R, 4), 0.5)
    if R >= 37:
        cls[2] = 1.25                                   # all equal
        cls[3] = cls[3] * 0.125
        cls[3, C // 2] += 60.0                          # one logit 60 above the rest
        cls[4] = -1e4 + rng.integers(0, 40, C) / 8.0    # all near -1e4
        # two live logits, the rest dead (expf gives exactly 0): z = 1 + e with one rounding,
        # so cls_prob of the smaller one is held to about 6 u relative down to 2^-20
        live = np.arange(R // 2, R // 2 + min(40, R // 4))
        for j, r in enumerate(live):
            a, b = rng.choice(C, 2, replace=False)
            cls[r] = -200.0
            # mostly where e^t is just above 2^-20: there an exponent formed as a rounded
            # product t * log2(e) (a fast-math exp) is off by up to 11 u of the element
            cls[r, a], cls[r, b] = 0.0, -f32(rng.uniform(11.2, 13.8) if j % 4 else
                                             rng.uniform(5.5, 11.0))
        lab[R - 1] = C - 1                              # the last class's gather, last row
        lab[R - 2] = max(int(lab[R - 2]), 1)
    inw = np.repeat((lab > 0).astype(np.float32)[:, None], 4, 1)
    outw = inw * rng.choice(np.array([1.0, 0.25], np.float32), (R, 1))
    # d = +-1 exactly (the cut at sigma 1), one ulp inside, 0
    one_in = np.nextafter(f32(1), f32(0))
    for r, vals in ((0, [1.0, -1.0, 0.0, one_in]), (R - 1, [-one_in, 0.0, 1.0, -1.0])):
        col = 0 if c.agnostic else 4 * lab[r]
        box[r, col:col + 4], tgt[r], inw[r], outw[r] = vals, 0.0, 1.0, 1.0
    _INPUTS[c] = dict(cls=cls, box=box, labels=lab, tgt=tgt, inw=inw, outw=outw, R=R,
                           R_total=c.Rt, C=C, agnostic=c.agnostic, sigma=1.0,
                           gloss=tuple(0.0 if g is None else g for g in c.gloss))
    return _INPUTS[c]


# ------------------------------------------------------------------ DA
DA = namedtuple("DA", "name Bs Bt Hs Ws Ht Wt ns nt need_s need_t")
DA_CASES = [
    DA("ones", 1, 1, 1, 1, 1, 1, 1, 1, (1,), (0,)),
    DA("two_source", 2, 1, 9, 11, 5, 6, 512, 300, (1, 0), (0,)),
    # source block 1 has 44 rows; target rows >= 512 are past both blocks: label 1
    DA("needs_crossed", 2, 2, 3, 5, 4, 4, 300, 600, (1, 0), (0, 1)),
    DA("second_stride", 1, 1, 37, 29, 3, 5, 7, 0, (1,), (0,)),  # 1073 pixels, no target rows
    DA("no_instances", 1, 1, 4, 4, 3, 5, 0, 0, (1,), (0,)),
    DA("packable", 2, 1, 5, 6, 5, 6, 300, 7, (0, 1), (0,)),     # one map size: packed too
]
DA_W = (1.0, 0.5, 2.0, 0.25, 3.0, 0.125)   # on (img_s, ins_s, img_t, ins_t, cst_s, cst_t)
DA_KERNEL_ORDER = (0, 1, 4, 2, 3, 5)       # the kernel's [img, ins, cst] x [source, target]


def da_inputs(c):
    if c in _INPUTS:
        return _INPUTS[c]
    rng = _rng("da" + c.name)
    scores = [_n32(rng, (c.Bs, 2, c.Hs, c.Ws), 2.0), _n32(rng, (c.Bt, 2, c.Ht, c.Wt), 2.0)]
    for sc in scores:
        B, _, H, W = sc.shape
        if H * W >= len(PAIRS):
            for j, (a0, a1) in enumerate(PAIRS):
                sc[B - 1, 0].reshape(-1)[j], sc[B - 1, 1].reshape(-1)[j] = a0, a1
    needs = [np.array(c.need_s, np.float32), np.array(c.need_t, np.float32)]
    inss = [rng.uniform(0.02, 0.98, n).astype(np.float32) for n in (c.ns, c.nt)]
    gloss = tuple(DA_W[i] for i in DA_KERNEL_ORDER)
    cons = F.da(scores, needs, inss, gloss)["cons"]
    for dom, x in enumerate(inss):
        # the consistency mean does not depend on the instances, so x = c can be planted
        plants = [0.0, 1.0, 1 - 2.0 ** -24, 2.0 ** -24, 1e-20, 0.5, cons[dom]]
        for start in (0, 256, 512):  # under every block's label
            n = min(len(plants), max(x.size - start, 0))
            x[start:start + n] = plants[:n]
        if x.size == 1:
            x[0] = 0.5
    _INPUTS[c] = dict(scores=scores, needs=needs, inss=inss, gloss=gloss)
    return _INPUTS[c]


# ------------------------------------------------------------------ what is compared, and how
# family -> (cases, inputs, restatement, truth, exact outputs, 1-ulp scalars, bounded outputs)
FAMILIES = {
    "rpn": (RPN_CASES, rpn_inputs, "rpn", "rpn_truth", ("count", "dbbox"), ("loss_box",),
            ("loss_cls", "dscore")),
    "rcnn": (RCNN_CASES, rcnn_inputs, "rcnn", "rcnn_truth", ("box_sel", "dbox"), ("loss_box",),
             ("prob", "loss_cls", "dcls")),
    "da": (DA_CASES, da_inputs, "da", "da_truth", (), (),
           ("loss", "cons", "dscore_s", "dscore_t", "dins_s", "dins_t")),
}
ALL = [(fam, c) for fam, spec in FAMILIES.items() for c in spec[0]]
ALL_IDS = [f"{fam}-{c.name}" for fam, c in ALL]


def expected(fam, case):
    """The restatement's outputs of the case."""
    return getattr(F, FAMILIES[fam][2])(**FAMILIES[fam][1](case))


def truth(fam, case):
    return getattr(F, FAMILIES[fam][3])(**FAMILIES[fam][1](case))


def ulps(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def _bytes(x):
    return np.ascontiguousarray(x, dtype=np.float32).tobytes()


def check(fam, case, got, exp, tru):
    """got (name -> array, from the device or from a restatement with a defect put in)
    against the restatement exp and the truth tru.  Returns (violations, figures): figures
    maps each bounded output to (worst error in u of its scale, worst error / bar)."""
    _, _, _, _, exact, ulp1, bounded = FAMILIES[fam]
    bad, fig = [], {}
    for name in exact:
        if name not in got:
            continue
        g, e = np.asarray(got[name], np.float32), np.asarray(exp[name], np.float32)
        if g.shape != e.shape or _bytes(g) != _bytes(e):
            n = int(np.count_nonzero(g.ravel().view(np.int32) != e.ravel().view(np.int32))) \
                if g.shape == e.shape else -1
            bad.append(f"{name}: {n} of {e.size} elements differ from the restatement")
    for name in ulp1:
        g, e = f32(got[name]), f32(exp[name])
        d = int(ulps(g, e)) if np.isfinite(g) and np.isfinite(e) else 1 << 30
        fig[name + " (ulp)"] = (float(d), float(d))
        if d > 1:
            bad.append(f"{name}: {g!r} is {d} ulp from the restated {e!r}")
    for name in bounded:
        if name not in got:
            continue
        t, bar, scale = (np.asarray(x, np.float64) for x in tru[name])
        g = np.asarray(got[name], np.float64).reshape(t.shape)
        bar, scale = np.broadcast_to(bar, t.shape), np.broadcast_to(scale, t.shape)
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs(g - t)
            err = np.where(np.isfinite(err), err, np.inf)
            over = err > bar
            inu = np.where(scale > 0, err / (U * np.where(scale > 0, scale, 1)), 0.0)
            ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1), 0.0)
        fig[name] = (float(inu.max()) if inu.size else 0.0, float(ratio.max()) if ratio.size
                     else 0.0)
        if over.any():
            i = int(np.argmax(np.where(over, err / np.maximum(bar, 1e-300), 0)))
            bad.append(f"{name}: {int(over.sum())} of {t.size} beyond the bar, worst at {i}: "
                       f"got {g.ravel()[i]!r} truth {t.ravel()[i]!r} bar {bar.ravel()[i]:.3e}")
        # contract zeros, and anything scaled by a zero upstream gradient: the restatement's
        # bytes (a zero's sign follows the IEEE product)
        zero = (bar.ravel() == 0) & (t.ravel() == 0)
        if zero.any():
            gz = np.asarray(got[name], np.float32).ravel()[zero]
            ez = np.asarray(exp[name], np.float32).ravel()[zero]
            if _bytes(gz) != _bytes(ez):
                n = int(np.count_nonzero(gz.view(np.int32) != ez.view(np.int32)))
                bad.append(f"{name}: {n} of {int(zero.sum())} contract zeros differ")
    return bad, fig


# ------------------------------------------------------------------ on the device
dev = "cuda"


def _t(a, grad=False):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t.requires_grad_(True) if grad else t


def _np(t):
    return t.detach().cpu().numpy()


def run_rpn(case):
    from tlod.detector.losses import rpn_losses
    i = rpn_inputs(case)
    s, b = _t(i["score"], True), _t(i["bbox"], True)
    lc, lb = rpn_losses(s, b, _t(i["labels"]), _t(i["tgt"]), _t(i["inw"]), _t(i["outw"]),
                        sigma=i["sigma"])
    (RPN_GLOSS[0] * lc + RPN_GLOSS[1] * lb).backward()
    # count is not returned: it is what loss_cls and dscore were divided by, and shows there
    return {"loss_cls": _np(lc), "loss_box": _np(lb),
            "dscore": _np(s.grad).ravel(), "dbbox": _np(b.grad).ravel()}


def run_rcnn(case):
    from tlod.detector.losses import rcnn_losses
    i = rcnn_inputs(case)
    c, b = _t(i["cls"], True), _t(i["box"], True)
    prob, sel, lc, lb = rcnn_losses(c, b, _t(i["labels"]), _t(i["tgt"]), _t(i["inw"]),
                                    _t(i["outw"]), i["agnostic"], i["sigma"])
    g0, g1 = case.gloss
    (g1 * lb if g0 is None else g0 * lc + g1 * lb).backward()
    return {"prob": _np(prob), "box_sel": _np(sel), "loss_cls": _np(lc), "loss_box": _np(lb),
            "dcls": _np(c.grad), "dbox": _np(b.grad)}


def _da_out(got, grads):
    import torch
    loss = _np(torch.stack([got[i] for i in DA_KERNEL_ORDER]))
    return dict(loss=loss, dscore_s=grads[0], dscore_t=grads[1], dins_s=grads[2],
                dins_t=grads[3])


def run_da(case):
    import torch
    from tlod.detector.losses import daf_da_losses
    i = da_inputs(case)
    xs = [_t(i["scores"][0], True), _t(i["scores"][1], True),
          _t(i["inss"][0][:, None], True), _t(i["inss"][1][:, None], True)]
    got = daf_da_losses(*xs, _t(i["needs"][0]), _t(i["needs"][1]))
    (torch.stack(got) @ _t(np.array(DA_W, np.float32))).backward()
    return _da_out(got, [_np(x.grad) for x in xs])


def run_da_packed(case):
    import torch
    from tlod.detector.losses import daf_da_losses_packed
    i = da_inputs(case)
    sc = _t(np.concatenate(i["scores"], 0), True)
    ins = _t(np.concatenate(i["inss"])[:, None], True)
    got = daf_da_losses_packed(sc, ins, case.Bs, case.ns, _t(i["needs"][0]), _t(i["needs"][1]))
    (torch.stack(got) @ _t(np.array(DA_W, np.float32))).backward()
    gs, gi = _np(sc.grad), _np(ins.grad)
    return _da_out(got, [gs[:case.Bs], gs[case.Bs:], gi[:case.ns], gi[case.ns:]])


RUN = {"rpn": run_rpn, "rcnn": run_rcnn, "da": run_da}


def _same_bytes(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert _bytes(a[k]) == _bytes(b[k]), f"{what}: {k} differs"


def _report(fam, case, fig, what="device"):
    for name, (inu, ratio) in sorted(fig.items()):
        print(f"FIGURE {what} {fam}-{case.name} {name}: {inu:.3f} u of scale, "
              f"{ratio:.3f} of the bar")


@pytest.mark.gpu
@pytest.mark.parametrize("fam,case", ALL, ids=ALL_IDS)
def test_device_against_restatement_and_truth(fam, case):
    got = RUN[fam](case)
    bad, fig = check(fam, case, got, expected(fam, case), truth(fam, case))
    _report(fam, case, fig)
    assert not bad, "\n".join(bad)
    _same_bytes(got, RUN[fam](case), f"{fam}-{case.name} run twice")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in DA_CASES if (c.Hs, c.Ws) == (c.Ht, c.Wt)],
                         ids=lambda c: c.name)
def test_da_packed_is_the_split_result(case):
    got = run_da_packed(case)
    bad, fig = check("da", case, got, expected("da", case), truth("da", case))
    _report("da", case, fig, "device packed")
    assert not bad, "\n".join(bad)
    _same_bytes(got, run_da(case), f"da-{case.name} packed against split")
    _same_bytes(got, run_da_packed(case), f"da-{case.name} packed run twice")
