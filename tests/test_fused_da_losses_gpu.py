"""The fused domain-adaptation losses pinned to tests/fused_da_losses.py through the public
entry points: tlod.da.idf.domain_losses (ef False / True: csrc/idf.hip, csrc/selftrain.hip),
tlod.da.idf.dam, separation and plain_distance (csrc/idf.hip), tlod.da.us_daf.us_daf_da_losses
and its packed form (csrc/us_daf.hip), tlod.da.pt_maf.masked_nll2, kd_kl_rows and kd_kl_rpn
(csrc/pt_maf.hip) and tlod.da.pa_atf.losses (csrc/pa_atf.hip).  The NLL's saved count, the KD's
saved normaliser and the separation's saved d are read from the autograd node, each checked
against what the entry point returned before it is used; no raw library call is needed.

For every case:

  exact      the whole US-DAF backward and the gates, masked_nll2's count, the IDF modulation
             a (1 + att) and the attention map's avg < thr, and every contract zero (cells off
             the map, an empty map, clamped focal rows, rows of weight 0 of the KD gradient,
             PA-ATF image gradients past the clamp and instance gradients at n = 2 label, the
             separation gradients under a zero attention and zero upstream gradients) equal the
             numpy restatement byte for byte;
  rounded    the US-DAF sigmoids, the per-image CE, dz_img, the focal / EFocal dz_ins, the KD
             loss, its normaliser and dstudent, the IDF avg (where kept), d, dist and both
             separation gradients and every PA-ATF gradient are within half a float32 ulp of
             the fp64 truth plus the kernel's derived double error;
  1 ulp      the focal / EFocal mean and the 14 PA-ATF terms are within 1 ulp of
             float32(fsum(terms) / n);
  bounded    masked_nll2's loss and dscore (fused_losses' ls2 bars) and the four US-DAF losses
             are within their derived bar of the fp64 truth;
  twice      a second run gives identical bytes; the packed US-DAF entry point gives the bytes
             of the split one.
No element is left out: each is compared as bytes or against a bar.

The cases and their inputs are built in numpy without a GPU and redrawn until no rounded-once
truth is within 2^-45 of a float32 tie, no focal p within 2^-45 of the clamp's midpoint and no
gate element loss within 16 u of 0.5; tests/test_fused_da_losses_cpu.py proves that, holds the
restatement and the truth to the torch compositions and to mpmath, and shows that every
plausible defect moves some expectation beyond its bar.

Measured on an MI355X (run with -s for every figure; worst over the cases).  For a rounded-once
quantity the bar is half a float32 ulp of the truth plus the kernel's double error, given here
in E = 2^-53 of the quantity's scale; the device's share of the bar is the rounding to float32
itself (the device gave float32(truth) wherever the share reads 1.00).  For a bounded quantity
both are in u = 2^-24 of the scale, with 2 ulp assumed for expf and logf.

  quantity                      bar (worst case)              device worst      case
  CE per image                  1/2 ulp + 8 E |t|             1.00 of the bar   efocal_r257
  dz_img                        1/2 ulp + 7.1 E |g|           0.95              focal_gamma_half
  focal / EFocal dz_ins         1/2 ulp + 70 E |g / R|        1.00              efocal_r513
  focal / EFocal mean           1 ulp                         0 ulp, every case
  US-DAF s_img, s_ins           1/2 ulp + 6.1 E               1.00              seam, edge1025
  US-DAF losses                 5.1 u * mean max(1, |e|)      0.86 u  (0.39)    packable
  masked_nll2 loss              7.3 u * mean max(1, |term|)   0.64 u  (0.98)    hw64_k8
  masked_nll2 dscore            8.4 u * |gout / count|        1.87 u  (0.66)    cap_full
  KD loss, sum w + 1            1/2 ulp + 281 E * scale       0.90              r1024
  KD dstudent                   1/2 ulp + 5834 E |g w|        1.00              r1023
  IDF att (avg where kept)      1/2 ulp + 19 E                1.00              p63_c15
  IDF d                         1/2 ulp + 14 E max(1, d)      1.00              p129_c33_zero_up
  IDF dist, plain dist          1/2 ulp + 28 E max(1, dist)   0.98              p65_c17
  IDF g_a, g_b                  1/2 ulp + 4.4 E * scale       1.00              p63_c15
  PA-ATF dz, image / CLUB       1/2 ulp + 7.1 E |g / n|       1.00              most_img, most_club
  PA-ATF dz, instance           1/2 ulp + 5.2 E |g / n|       1.00              most_ins
  PA-ATF 14 loss terms          1 ulp                         0 ulp, every case

Every exact piece matched byte for byte in every case (the US-DAF backward through both sweeps
and the pixel / instance seam, the subnormal sigmoid of -90 included), every case gave the same
bytes twice, and the packed US-DAF entry point the bytes of the split one.  (hw64_k8's loss
reads 0.98 of its bar in a one-cell map on a planted pair 104 apart: the truth is log1p(e^-104)
= 6.8e-46, the device's 0, the bar that term itself.)  The double cancellation p - 1.0 keeps 24
bits at a logit difference of 20 and none at 40 (p is 1.0, the gradient exactly 0); both are
inside the absolute term 5 E |g| and were left as they are.

One kernel defect was found: focal_gamma_half (gamma = 0.5, rows whose label leads by 40 and
104).  There 1.0 - p is 0 in double and domain_loss_bwd_kernel formed gamma * pow(0, -0.5) *
log(1.0) = inf * 0, a NaN gradient; the rows now take the exactly zero gradient the formula
gives for gamma >= 1 (include/tlod_idf.h says so), and gamma <= 0 is refused.

Libraries built with one defect each, one run each, the new tests and the old
test_{pt_maf,us_daf,idf,pa_atf}_ops_gpu.py / test_selftrain_gpu.py:
  masked_nll2_bwd without its grid stride    nll-cap_two_cells, nll-cap_full fail; old tests pass
  KD normaliser counting every row           the four kd-rpn_* cases fail; the old
                                             test_kd_kl_rpn_strided and test_kd_kl_switch_matches
                                             fail too
  kNear0 dropped from the US-DAF backward    all six us-* cases and the three packed ones fail;
                                             of the old tests test_saturation fails (a NaN)
  `<=` in the focal clamp (both kernels)     the five focal cases with clamp rows fail; old pass
  float expf in sigmoid_rn                   all six us-* cases and the three packed ones fail;
                                             old tests pass
  `n - label` for `n - 2 * label`            the three pa-* cases fail (dz ins); the old
                                             test_losses_against_the_fp64_composition fails too
  `avg <= thr` in the DAM                    all seven sep-* cases fail (att: the constant map is
                                             dropped); the old IDF tests pass
"""
import zlib
from collections import namedtuple

import numpy as np
import pytest

import fused_da_losses as D
from test_fused_losses_gpu import PAIRS, _bytes, ulps

f32 = np.float32
U = D.U
TIE = 2.0 ** -45
_INPUTS = {}


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _n32(rng, shape, scale=1.0):
    return (scale * rng.standard_normal(shape)).astype(np.float32)


def _up(a, idx):
    """Nudge the float32 elements a[idx] one step up (a redraw that keeps a planted value)."""
    a[idx] = np.nextafter(a[idx], f32(np.inf))


# ------------------------------------------------------------------ IDF / EFocal domain losses
DL = namedtuple("DL", "name n_img R label_img label_ins gamma ef gloss")
DL_CASES = [
    DL("focal_r1", 1, 1, 0, 1, 3.0, False, (1.0, 0.25)),
    DL("focal_r255", 2, 255, 1, 0, 1.0, False, (0.5, 2.0, 0.25)),
    DL("focal_r256", 3, 256, 0, 0, 5.0, False, (1.0, 0.0, 3.0, 0.25)),   # a zero upstream
    DL("focal_r257", 2, 257, 1, 1, 3.0, False, (0.5, 0.5, 0.25)),
    DL("focal_r513", 3, 513, 0, 1, 3.0, False, (0.5, 0.125, 1.5, 1.0)),
    DL("focal_gamma_half", 2, 257, 1, 0, 0.5, False, (0.5, 0.5, 0.25)),  # inf * 0 before the fix
    DL("efocal_r1", 1, 1, 1, 0, 3.0, True, (1.0, 0.25)),
    DL("efocal_r255", 2, 255, 0, 1, 1.0, True, (0.5, 2.0, 0.25)),
    DL("efocal_r256", 3, 256, 1, 1, 5.0, True, (1.0, 0.0, 3.0, 0.25)),
    DL("efocal_r257", 2, 257, 0, 0, 3.0, True, (0.5, 0.5, 0.25)),
    DL("efocal_r513", 3, 513, 1, 0, 3.0, True, (0.5, 0.125, 1.5, 1.0)),
]
# (label's logit, the other's): equal, signed zeros, the label ahead / behind by 20, 40, 104
DL_PAIRS = [(1.5, 1.5), (0.0, -0.0), (-0.0, 0.0), (19.75, -0.25), (-0.25, 19.75), (40.5, 0.5),
            (0.5, 40.5), (102.0, -2.0), (-2.0, 102.0)]


def clamp_rows():
    """(label's logit, the other's) rows around the focal clamp: three float32 neighbours of
    x = ln(1 / m - 1) on each side (m the midpoint below 1e-6f), and a row whose float32 p is
    1e-6f itself (not clamped: the compare is strict)."""
    m = D.clamp_midpoint()
    x0 = f32(np.log(1 / m - 1))
    xs = [x0]
    for _ in range(3):
        xs.append(np.nextafter(xs[-1], f32(100)))
    lo = x0
    for _ in range(3):
        lo = np.nextafter(lo, f32(0))
        xs.append(lo)
    rows = [(f32(0), x) for x in xs]
    # p = 1e-6f to within a quarter ulp: the label's logit takes up the fine part of x
    c = float(f32(1e-6))
    zo = f32(13.75)
    zl = f32(float(zo) - np.log(1 / c - 1))
    best = min((np.nextafter(zl, f32(-1)), zl, np.nextafter(zl, f32(1))),
               key=lambda v: abs(1 / (1 + np.exp(float(zo) - float(v))) - c))
    rows.append((best, zo))
    return rows


def dl_inputs(c):
    if c in _INPUTS:
        return _INPUTS[c]
    rng = _rng("dl" + c.name)
    z_img = _n32(rng, (c.n_img, 2), 2.0)
    z_ins = _n32(rng, (c.R, 2), 3.0)
    plants = list(DL_PAIRS) + ([] if c.ef else clamp_rows())
    shift = len(c.name)
    if c.n_img == 3:  # the image terms meet the saturated differences too
        for i in range(3):
            a, b = DL_PAIRS[3 + (i + shift) % 6]
            z_img[i, c.label_img], z_img[i, 1 - c.label_img] = a, b
    if c.R >= len(plants):
        for j, (a, b) in enumerate(plants):
            r = j if j % 2 else c.R - 1 - j  # both ends of the rows
            z_ins[r, c.label_ins], z_ins[r, 1 - c.label_ins] = a, b
    i = dict(z_img=z_img, label_img=c.label_img, z_ins=z_ins, label_ins=c.label_ins,
             gamma=c.gamma, ef=c.ef, gloss=c.gloss)
    for _ in range(50):
        bad_img, bad_ins = dl_tie_rows(i)
        if not (bad_img.size or bad_ins.size):
            break
        _up(z_img[:, 0], bad_img)
        _up(z_ins[:, 0], bad_ins)
    _INPUTS[c] = i
    return i


def dl_tie_rows(i):
    """Rows of z_img / z_ins with a rounded-once truth within 2^-45 of a float32 tie, or a
    focal p within 2^-45 of the clamp's midpoint."""
    t = D.domain_losses_truth(**i)
    n = i["z_img"].shape[0]
    g = np.asarray(i["gloss"], np.float64)
    img = (D.tie_margin(t["ce"][0]) < TIE) | ((D.tie_margin(t["dz_img"][0][:, 0]) < TIE)
                                              & (g[:n] != 0))
    ins = (D.tie_margin(t["dz_ins"][0][:, 0]) < TIE) & ~t["exact"]["dz_ins"][0][:, 0]
    if not i["ef"]:
        ins |= D.clamp_margin(i["z_ins"], i["label_ins"]) < TIE
    return np.flatnonzero(img), np.flatnonzero(ins)


def dl_check(c, got, exp, tru):
    bad, fig = [], {}
    n = c.n_img
    _bounded("ce", got["loss"][:n], tru["ce"], bad, fig)
    g, e = f32(got["loss"][n]), f32(tru["focal"])
    d = int(ulps(g, e)) if np.isfinite(g) and np.isfinite(e) else 1 << 30
    fig["focal (ulp)"] = (float(d), float(d))
    if d > 1:
        bad.append(f"focal: {g!r} is {d} ulp from the expected {e!r}")
    _bounded("dz_img", got["dz_img"], tru["dz_img"], bad, fig)
    _bounded("dz_ins", got["dz_ins"], tru["dz_ins"], bad, fig, tru["exact"]["dz_ins"])
    return bad, fig


def dl_caps(c, tru):
    return [(k,) + tru[k] for k in ("ce", "dz_img", "dz_ins")], []


def dl_run(c):
    from tlod.da.idf import domain_losses
    i = dl_inputs(c)
    zi, zn = _t(i["z_img"], True), _t(i["z_ins"], True)
    loss = domain_losses(zi, c.label_img, zn, c.label_ins, c.gamma, c.ef)
    (loss * _t(np.array(c.gloss, np.float32))).sum().backward()
    return {"loss": _np(loss), "dz_img": _np(zi.grad), "dz_ins": _np(zn.grad)}


# ------------------------------------------------------------------ US-DAF
US = namedtuple("US", "name Bs Hs Ws Bt Ht Wt ns nt gated gloss")
US_CASES = [
    US("one", 1, 1, 1, 1, 1, 1, 1, 0, False, (1.0, 0.5, 2.0, 0.25)),
    US("edge1025", 1, 25, 41, 2, 3, 5, 3, 1025, False, (1.0, 0.0, 0.5, 2.0)),  # a zero upstream
    US("edge1025_gated", 1, 25, 41, 2, 3, 5, 3, 1025, True, (1.0, 0.5, 0.5, 2.0)),
    # 262144 + 4 elements: the source's second sweep holds the pixel / instance seam; the
    # target (1025 pixels, then 4 x 1025) ends inside the first
    US("seam", 1, 512, 512, 1, 25, 41, 1, 1025, False, (3.0, 0.5, 0.25, 1.0)),
    US("packable", 1, 5, 7, 1, 5, 7, 3, 5, False, (1.0, 0.5, 2.0, 0.25)),
    US("packable_gated", 1, 5, 7, 1, 5, 7, 3, 5, True, (1.0, 0.5, 2.0, 0.25)),
]
# 0, signed zeros, and the saturations: float32 s is exactly 1 from 17.33 up and exactly 0 at
# -104, subnormal at -90; 1 - s is exactly 0, so both image clamps at -100, log(1e-10) and
# q < 1e-12 in the backward are all reached
US_LOGITS = [0.0, -0.0, 20.0, -20.0, 40.0, -40.0, 90.0, -90.0, 104.0, -104.0, 0.4375, -0.4375]
# (width, height): areas at and on each side of 400 and 10000
US_BOXES = [(20.0, 20.0), (20.0, 20.000002), (20.0, 19.999998), (100.0, 100.0),
            (100.0, 99.99999), (100.0, 100.00001), (5.0, 5.0), (300.0, 300.0)]


def us_inputs(c):
    if c in _INPUTS:
        return _INPUTS[c]
    rng = _rng("us" + c.name)
    z_imgs = [_n32(rng, (c.Bs, 1, c.Hs, c.Ws), 2.0), _n32(rng, (c.Bt, 1, c.Ht, c.Wt), 2.0)]
    z_inss = [_n32(rng, (c.ns, 4), 2.0), _n32(rng, (c.nt, 4), 2.0)]
    roiss = []
    for dom, n in enumerate((c.ns, c.nt)):
        zi = z_imgs[dom].reshape(-1)
        if zi.size >= 2 * len(US_LOGITS):
            zi[:len(US_LOGITS)] = US_LOGITS
            zi[-len(US_LOGITS):] = US_LOGITS[::-1]
        zn = z_inss[dom]
        if n >= len(US_LOGITS):
            for col in range(4):  # every column, both ends of the rows
                zn[:len(US_LOGITS), col] = np.roll(US_LOGITS, col)
                zn[-len(US_LOGITS):, col] = np.roll(US_LOGITS, -col)
        elif n:
            zn[0] = (20.0, -20.0, 0.0, -104.0) if dom == 0 else (-40.0, 90.0, -0.0, 104.0)
        r = np.zeros((n, 5), np.float32)
        r[:, 1:3] = rng.uniform(0, 200, (n, 2))
        wh = rng.uniform(5, 150, (n, 2)).astype(np.float32)
        for j in range(min(n, len(US_BOXES))):
            wh[(j * 7) % n] = US_BOXES[j]
        if n:
            r[:, 3:5] = r[:, 1:3] + wh
            # x2 - x1 must come back as the planted width: take whole coordinates there
            for j in range(min(n, len(US_BOXES))):
                k = (j * 7) % n
                r[k, 1:3] = np.floor(r[k, 1:3])
                r[k, 3:5] = r[k, 1:3] + np.array(US_BOXES[j], np.float32)
        roiss.append(r)
    gates = None
    if c.gated:
        gates = [(rng.random(n) < 0.5).astype(np.float32) for n in (c.ns, c.nt)]
    i = dict(z_imgs=z_imgs, z_inss=z_inss, roiss=roiss, gates_in=gates, gloss=c.gloss)
    for _ in range(50):
        bad = us_tie_elems(i)
        if not any(b.size for b in bad):
            break
        for dom in (0, 1):
            _up(z_imgs[dom].reshape(-1), bad[2 * dom])
            _up(z_inss[dom].reshape(-1), bad[2 * dom + 1])
    _INPUTS[c] = i
    return i


def us_tie_elems(i):
    """Per domain the flat indices of image / instance logits whose sigmoid is within 2^-45 of
    a float32 tie, or (column 0) whose element loss is within 16 u of the gate's 0.5."""
    t = D.us_daf_truth(**i)
    out = []
    for tag in "st":
        out.append(np.flatnonzero(D.tie_margin(t["s_img_" + tag][0]) < TIE))
        near = D.tie_margin(t["s_ins_" + tag][0]) < TIE
        near[:, 0] |= D.gate_margin(t["e0_" + tag]) < 16
        out.append(np.flatnonzero(near.ravel()))
    return out


US_EXACT = ("gate_s", "gate_t", "dz_img_s", "dz_img_t", "dz_ins_s", "dz_ins_t")
US_ROUNDED = ("s_img_s", "s_img_t", "s_ins_s", "s_ins_t")


def us_check(c, got, exp, tru):
    bad, fig = [], {}
    for name in US_ROUNDED:
        _bounded(name, got[name], tru[name], bad, fig)
    _bounded("loss", got["loss"], tru["loss"], bad, fig)
    for name in US_EXACT:
        _exact(name, got[name], exp[name], bad)
    return bad, fig


def us_caps(c, tru):
    return [(k,) + tru[k] for k in US_ROUNDED], [("loss",) + tru["loss"]]


def _us_out(da, s, gate, grads):
    import torch
    out = {"loss": _np(torch.stack(list(da)))}
    for name, x in zip(US_ROUNDED, s):
        out[name] = _np(x)
    out["gate_s"], out["gate_t"] = _np(gate[0]), _np(gate[1])
    for name, x in zip(US_EXACT[2:], grads):
        out[name] = x
    return out


def us_run(c):
    import torch
    from tlod.da.us_daf import us_daf_da_losses
    i = us_inputs(c)
    xs = [_t(i["z_imgs"][0], True), _t(i["z_imgs"][1], True), _t(i["z_inss"][0], True),
          _t(i["z_inss"][1], True)]
    go = None if i["gates_in"] is None else tuple(_t(g) for g in i["gates_in"])
    da, s, gate = us_daf_da_losses(*xs, _t(i["roiss"][0]), _t(i["roiss"][1]), go)
    (torch.stack(da) @ _t(np.array(c.gloss, np.float32))).backward()
    return _us_out(da, s, gate, [_np(xs[0].grad).ravel(), _np(xs[1].grad).ravel(),
                                 _np(xs[2].grad), _np(xs[3].grad)])


def us_run_packed(c):
    import torch
    from tlod.da.us_daf import us_daf_da_losses_packed
    i = us_inputs(c)
    zi = _t(np.concatenate(i["z_imgs"], 0), True)
    zn = _t(np.concatenate(i["z_inss"], 0), True)
    go = None if i["gates_in"] is None else tuple(_t(g) for g in i["gates_in"])
    da, s, gate = us_daf_da_losses_packed(zi, zn, _t(np.concatenate(i["roiss"], 0)), c.Bs, c.ns,
                                          go)
    (torch.stack(da) @ _t(np.array(c.gloss, np.float32))).backward()
    gi, gn = _np(zi.grad), _np(zn.grad)
    return _us_out(da, s, gate, [gi[:c.Bs].ravel(), gi[c.Bs:].ravel(), gn[:c.ns], gn[c.ns:]])


# ------------------------------------------------------------------ masked 2-way NLL
NLL = namedtuple("NLL", "name B H W K maps")
NLL_CASES = [
    NLL("hw1", 1, 1, 1, 1, "full"),
    NLL("hw63", 3, 7, 9, 1, "mixed"),
    NLL("hw64_k8", 1, 8, 8, 8, "mixed"),
    NLL("hw65", 3, 5, 13, 1, "mixed"),
    NLL("hw1023", 1, 33, 31, 1, "last"),
    NLL("hw1024", 3, 32, 32, 1, "random"),
    NLL("hw1025_k8", 1, 25, 41, 8, "mixed"),
    NLL("hw2049", 3, 3, 683, 1, "random"),
    # 16385 cells: one past the backward's 64 x 256 grid, so cell 16384 is the second sweep
    NLL("cap_two_cells", 1, 113, 145, 1, "cap"),
    NLL("cap_full", 1, 113, 145, 1, "full"),
]
KINDS = ("random", "empty", "first", "last", "full")


def _map(kind, HW, rng):
    m = np.zeros(HW, np.float32)
    if kind == "random":
        m[rng.random(HW) < 0.4] = 1
        m[[0, HW - 1]] = 1
    elif kind == "first":
        m[0] = 1
    elif kind == "last":
        m[HW - 1] = 1
    elif kind == "full":
        m[:] = 1
    elif kind == "cap":
        m[[16383, 16384]] = 1
    return m


def nll_inputs(c):
    if c in _INPUTS:
        return _INPUTS[c]
    rng = _rng("nll" + c.name)
    HW = c.H * c.W
    need = np.array([(b + len(c.name)) % 2 for b in range(c.B)], np.float32)
    scores, maps, shared = [], [], []
    for k in range(c.K):
        if k == 1:  # one score tensor in two pairs
            scores.append(scores[0])
            shared.append(0)
        else:
            scores.append(_n32(rng, (c.B, 2, c.H, c.W), 3.0))
            shared.append(k)
        mp = np.stack([_map(KINDS[(k + b + len(c.name)) % 5] if c.maps == "mixed" else c.maps,
                            HW, rng) for b in range(c.B)]).reshape(c.B, c.H, c.W)
        maps.append(mp)
    for k in range(c.K):  # the planted pairs on the first kept cells of pair k (k = 1: pair 0's)
        if shared[k] != k:
            continue
        for b in range(c.B):
            kept = np.flatnonzero(maps[k][b].ravel() == 1)
            if c.maps == "cap":
                # cell 16384 (the second sweep) decided and right by 20: its gradient is
                # 2e-9 of the other cell's, far below what a max-norm check can see
                lab = int(need[b])
                sc = scores[k][b].reshape(2, HW)
                sc[lab, 16384], sc[1 - lab, 16384] = 19.75, -0.25
                sc[lab, 16383], sc[1 - lab, 16383] = -0.5, 0.25
                continue
            for j, q in enumerate(kept[:len(PAIRS)]):
                a0, a1 = PAIRS[(j + k + b) % len(PAIRS)]
                scores[k][b].reshape(2, HW)[:, q] = a0, a1
    gout = 0.25 * (1 + np.arange(c.K * c.B, dtype=np.float32)).reshape(c.K, c.B)
    if c.K * c.B > 1:
        gout[-1, -1] = 0.0
    _INPUTS[c] = dict(scores=scores, maps=maps, need=need, gout=gout)
    return _INPUTS[c]


def nll_check(c, got, exp, tru):
    bad, fig = [], {}
    _exact("count", got["count"], exp["count"], bad)
    _bounded("loss", got["loss"], tru["loss"], bad, fig)
    zero = np.zeros(tru["zeros"].shape, np.float32)
    _bounded("dscore", got["dscore"], tru["dscore"], bad, fig, (tru["zeros"], zero))
    return bad, fig


def nll_caps(c, tru):
    return [], [("loss",) + tru["loss"], ("dscore",) + tru["dscore"]]


def nll_run(c):
    import torch
    from tlod.da.pt_maf import masked_nll2
    i = nll_inputs(c)
    base = []
    for k, s in enumerate(i["scores"]):
        base.append(base[0] if k == 1 else _t(s))
    # pair 1 reads pair 0's storage through a leaf of its own, and so has its own gradient
    leaves = [s.detach().requires_grad_(True) for s in base]
    loss = masked_nll2(_t(i["need"]), [(s, _t(m)) for s, m in zip(leaves, i["maps"])])
    out = loss.grad_fn.saved_tensors[1]  # (2, K, B): loss, count
    assert out.shape == (2, c.K, c.B) and torch.equal(out[0], loss.detach())
    count = out[1]
    (loss * _t(i["gout"])).sum().backward()
    HW = c.H * c.W
    return {"loss": _np(loss), "count": _np(count),
            "dscore": np.stack([_np(s.grad).reshape(c.B, 2, HW) for s in leaves])}


# ------------------------------------------------------------------ KD KL
# rows: (R, C) scores with a weight per row; rpn: (1, 2, A*H, W) scores, g (H, W) shared by
# the A anchors (R = A H W rows of stride 1, class stride R, wmod = H W)
KD = namedtuple("KD", "name form R C A H W T weights mag gout")
KD_CASES = [
    KD("r1", "rows", 1, 2, 0, 0, 0, 1.0, "ones", 2.0, 1.0),
    KD("r1023", "rows", 1023, 9, 0, 0, 0, 3.0, "binary0", 2.0, 0.5),   # w[0] = 0
    KD("r1024", "rows", 1024, 21, 0, 0, 0, 1.0, "frac", 2.0, 2.0),
    KD("r1025_mag30", "rows", 1025, 9, 0, 0, 0, 3.0, "binary", 30.0, 0.5),
    KD("r2049_mag100", "rows", 2049, 21, 0, 0, 0, 3.0, "frac", 100.0, 1.0),
    KD("equal", "rows", 1025, 9, 0, 0, 0, 3.0, "frac", 2.0, 1.0),      # student = teacher
    # one row past the backward's 1024 x 256 grid; its weight is 1
    KD("cap", "rows", 262145, 2, 0, 0, 0, 3.0, "binary", 2.0, 1.0),
    KD("rpn_3_5_7", "rpn", 105, 2, 3, 5, 7, 1.0, "binary0", 2.0, 1.0),
    KD("rpn_9_12_20", "rpn", 2160, 2, 9, 12, 20, 3.0, "frac", 2.0, 0.5),
    KD("rpn_5_5_41", "rpn", 1025, 2, 5, 5, 41, 3.0, "binary", 2.0, 1.0),  # wmod = 205 < 1025
    # one weight of 2^-19: counted once per row instead of once it moves the loss by 1.5e-5
    KD("rpn_one_small_weight", "rpn", 2160, 2, 9, 12, 20, 3.0, "one_small", 2.0, 1.0),
]


def kd_inputs(c):
    if c in _INPUTS:
        return _INPUTS[c]
    rng = _rng("kd" + c.name)
    R, C = c.R, c.C
    teacher = _n32(rng, (R, C), c.mag)
    student = (teacher + _n32(rng, (R, C), 0.25 * c.mag)).astype(np.float32)
    if c.name == "equal":
        student = teacher.copy()
    elif R >= 64:
        student[1] = teacher[1]                                   # an equal row
        student[2] = teacher[2]
        student[2, C - 1] = np.nextafter(teacher[2, C - 1], f32(np.inf))  # one ulp, one class
        student[3] = teacher[3]
        student[3, 0] = np.nextafter(teacher[3, 0], f32(-np.inf))
        # the teacher puts e^-104 on the student's best class (T = 3: 312 apart)
        k = int(np.argmax(student[4]))
        teacher[4] = 0.0
        teacher[4, k] = -104.0 * c.T
        student[R - 1], teacher[R - 1] = student[4], teacher[4]
    wmod = c.H * c.W if c.form == "rpn" else R
    if c.weights == "ones":
        w = np.ones(wmod, np.float32)
    elif c.weights in ("binary", "binary0"):
        w = (rng.random(wmod) < 0.5).astype(np.float32)
        w[:min(5, wmod)] = 1.0
        w[wmod - 1] = 1.0
        if c.weights == "binary0":
            w[0] = 0.0
    elif c.weights == "frac":
        w = rng.random(wmod).astype(np.float32)
        w[rng.random(wmod) < 0.2] = 0.0
        w[:min(5, wmod)] = rng.random(min(5, wmod)).astype(np.float32) + f32(0.25)
    else:
        w = np.zeros(wmod, np.float32)
        w[wmod // 2] = 2.0 ** -19
    if c.form == "rpn":  # row r = (a, h, w), class c: element c * R + r of (1, 2, A*H, W)
        student = np.ascontiguousarray(student.T).reshape(1, 2, c.A * c.H, c.W)
        teacher = np.ascontiguousarray(teacher.T).reshape(1, 2, c.A * c.H, c.W)
        lay = dict(R=R, C=2, rs=1, cs=R, wmod=wmod)
    else:
        lay = dict(R=R, C=C, rs=C, cs=1, wmod=wmod)
    i = dict(student=student, teacher=teacher, weight=w, T=c.T, gout=c.gout, **lay)
    for _ in range(50):
        t = D.kd_kl_truth(**i)
        bad = np.flatnonzero((D.tie_margin(t["dstudent"][0]) < TIE) & ~t["zeros"])
        if not bad.size and D.tie_margin(t["out"][0]).min() >= TIE:
            break
        _up(student.reshape(-1), bad if bad.size else np.array([5 * C]))
    _INPUTS[c] = i
    return i


def kd_check(c, got, exp, tru):
    bad, fig = [], {}
    _bounded("out", got["out"], tru["out"], bad, fig)
    zero = np.zeros(tru["zeros"].shape, np.float32)
    _bounded("dstudent", got["dstudent"], tru["dstudent"], bad, fig, (tru["zeros"], zero))
    return bad, fig


def kd_caps(c, tru):
    return [("out",) + tru["out"], ("dstudent",) + tru["dstudent"]], []


def kd_run(c):
    import torch
    from tlod.da.pt_maf import kd_kl_rows, kd_kl_rpn
    i = kd_inputs(c)
    s = _t(i["student"], True)
    if c.form == "rpn":
        loss = kd_kl_rpn(s, _t(i["teacher"]), _t(i["weight"].reshape(c.H, c.W)), c.T)
    else:
        loss = kd_kl_rows(s, _t(i["teacher"]), _t(i["weight"]), c.T)
    out = loss.grad_fn.saved_tensors[3]  # [loss, sum w + 1]
    assert out.shape == (2,) and torch.equal(out[0], loss.detach())
    (loss * c.gout).backward()
    return {"out": _np(out), "dstudent": _np(s.grad).ravel()}


# ------------------------------------------------------------------ PA-ATF: the 14 terms
# n: six image terms, two instance terms, six CLUB terms; in each case the largest n (what the
# backward's grid is sized by) belongs to one term only.  ones: per instance term
PA = namedtuple("PA", "name n img_labels ones club_labels gloss_zero")
PA_CASES = [
    PA("most_img", (1, 255, 256, 257, 1025, 63, 256, 257, 1, 255, 256, 257, 300, 5),
       (0, 1, 0, 1, 1, 0), (128, 256), (1, 0, 1, 0, 1, 0), 3),        # n / 2 and n - 1 ones
    PA("most_ins", (257, 1, 255, 256, 64, 65, 1025, 1, 257, 1, 255, 256, 33, 300),
       (1, 0, 1, 0, 0, 1), (1, 1), (0, 1, 0, 1, 0, 1), 7),            # 1 and n ones
    PA("most_club", (256, 257, 1, 255, 300, 12, 255, 256, 1025, 256, 1, 257, 255, 64),
       (0, 0, 1, 1, 0, 1), (0, 256), (1, 1, 0, 0, 1, 0), 10),         # 0 and n ones
]
# on each side of the backward's switch and of the forward's clamp at 100, and far past it
PA_LOGITS = [99.5, -99.5, 100.5, -100.5, 745.0, -745.0, 0.0, -0.0, 20.0, -20.0, 40.0, -40.0]


def pa_inputs(c):
    if c in _INPUTS:
        return _INPUTS[c]
    rng = _rng("pa" + c.name)
    z = []
    for t, n in enumerate(c.n):
        if t < D.PA_IMG + D.PA_INS:
            x = _n32(rng, (n, 1) if t >= D.PA_IMG else (n,), 2.0)
            if n >= 2 * len(PA_LOGITS):
                x.reshape(-1)[:len(PA_LOGITS)] = PA_LOGITS
                x.reshape(-1)[-len(PA_LOGITS):] = PA_LOGITS[::-1]
        else:
            x = _n32(rng, (n, 2), 2.0)
            lab = c.club_labels[t - D.PA_IMG - D.PA_INS]
            if n >= len(DL_PAIRS):
                for j, (a, b) in enumerate(DL_PAIRS):
                    r = j if j % 2 else n - 1 - j
                    x[r, lab], x[r, 1 - lab] = a, b
        z.append(x)
    gloss = 0.25 * (1 + np.arange(D.PA_TERMS, dtype=np.float32))
    gloss[c.gloss_zero] = 0.0
    label = list(c.img_labels) + list(c.ones) + list(c.club_labels)
    i = dict(z=z, n=list(c.n), label=label, gloss=gloss)
    for _ in range(50):
        t = D.pa_atf_truth(**i)
        clean = True
        for k in range(D.PA_TERMS):
            v, _, _ = t["dz"][k]
            bad = np.flatnonzero(((D.tie_margin(v) < TIE) & ~t["exact"][k][0]).reshape(
                c.n[k], -1).any(1))
            if bad.size:
                clean = False
                _up(z[k].reshape(c.n[k], -1)[:, 0], bad)
        if clean:
            break
    _INPUTS[c] = i
    return i


def pa_check(c, got, exp, tru):
    bad, fig = [], {}
    for t in range(D.PA_TERMS):
        g, e = f32(got["loss"][t]), f32(tru["loss"][t])
        d = int(ulps(g, e)) if np.isfinite(g) and np.isfinite(e) else 1 << 30
        kind = "img" if t < D.PA_IMG else ("ins" if t < D.PA_IMG + D.PA_INS else "club")
        fig[f"loss {kind} (ulp)"] = max(fig.get(f"loss {kind} (ulp)", (0.0, 0.0)),
                                         (float(d), float(d)))
        if d > 1:
            bad.append(f"loss[{t}]: {g!r} is {d} ulp from the expected {e!r}")
        sub = {}
        _bounded(f"dz {kind}", got["dz"][t], tru["dz"][t], bad, sub, tru["exact"][t])
        fig[f"dz {kind}"] = max(fig.get(f"dz {kind}", (0.0, 0.0)), sub[f"dz {kind}"],
                                key=lambda v: v[1])
    return bad, fig


def pa_caps(c, tru):
    return [(f"dz[{t}]",) + tru["dz"][t] for t in range(D.PA_TERMS)], []


def pa_run(c):
    from tlod.da.pa_atf import losses
    i = pa_inputs(c)
    z = [_t(x, True) for x in i["z"]]
    a, b = D.PA_IMG, D.PA_IMG + D.PA_INS
    loss = losses(z[:a], list(c.img_labels), z[a:b], list(c.ones), z[b:], list(c.club_labels))
    (loss * _t(i["gloss"])).sum().backward()
    return {"loss": _np(loss), "dz": [_np(x.grad) for x in z]}


# ------------------------------------------------------------------ IDF: DAM and separation
# mode: "mod" the three outputs and all three upstream gradients; "dist": only the distance
# carries a gradient (the backward without the modulation terms); "zero_up": zero upstream
# gradients on the modulated maps, so a zero attention gives exactly zero gradients
SEP = namedtuple("SEP", "name C H W mode")
SEP_CASES = [
    SEP("p1_c1", 1, 1, 1, "mod"),
    SEP("p63_c15", 15, 7, 9, "mod"),
    SEP("p64_c16", 16, 8, 8, "mod"),
    SEP("p65_c17", 17, 5, 13, "mod"),
    SEP("p129_c33", 33, 3, 43, "mod"),
    SEP("p65_c17_dist_only", 17, 5, 13, "dist"),
    SEP("p129_c33_zero_up", 33, 3, 43, "zero_up"),
]


def sep_inputs(c):
    if c in _INPUTS:
        return _INPUTS[c]
    rng = _rng("sep" + c.name)
    N, C, P = 2, c.C, c.H * c.W
    x = _n32(rng, (N, C, P), 2.0)
    x[1] = _n32(rng, (C, 1), 2.0)  # a constant map: every avg equals the threshold, all kept
    a, b = _n32(rng, (N, C, P)), _n32(rng, (N, C, P))
    att_a = rng.uniform(0.3, 0.7, (N, P)).astype(np.float32)
    att_b = rng.uniform(0.3, 0.7, (N, P)).astype(np.float32)
    att_a[rng.random((N, P)) < 0.3] = 0.0
    att_b[rng.random((N, P)) < 0.3] = 0.0
    if P >= 63:
        att_b[:, 0] = (0.5, 0.40625)
        att_b[:, 1], att_b[:, 2] = 0.625, 0.0
        b[:, :, 1] = a[:, :, 1]                       # a == b: d = sqrt(C) 1e-6
        for k in range(5):                            # (a - b) w near -1e-6: e crosses zero
            b[:, k, 0] = a[:, k, 0] + (f32(1e-6) / att_b[:, 0]) * f32(1 + (k - 2) * 1e-3)
    g_a, g_b = _n32(rng, (N, C, P)), _n32(rng, (N, C, P))
    if c.mode == "zero_up":
        g_a[:], g_b[:] = 0.0, 0.0
    g_d = np.array([1.5, 0.25], np.float32)
    i = dict(x=x, a=a, b=b, att_a=att_a, att_b=att_b, g_a_out=None if c.mode == "dist" else g_a,
             g_b_out=None if c.mode == "dist" else g_b, g_dist=g_d)
    for _ in range(50):
        bad = sep_tie_elems(i)
        if not any(v.size for v in bad):
            break
        _up(x.reshape(-1), bad[0])
        _up(a.reshape(-1), bad[1])
    _INPUTS[c] = i
    return i


def _sep_args(i, plain=False):
    if plain:
        return dict(a=i["a"], b=i["b"], att_a=None, att_b=None, g_a_out=None, g_b_out=None,
                    g_dist=None)
    return {k: i[k] for k in ("a", "b", "att_a", "att_b", "g_a_out", "g_b_out", "g_dist")}


def sep_tie_elems(i):
    """Flat indices into x and into a of elements behind a rounded-once truth within 2^-45 of
    a float32 tie (avg, thr; d, dist, the plain dist, g_a, g_b)."""
    N, C, P = i["x"].shape
    t = D.dam_truth(i["x"])
    px = (D.tie_margin(t["avg"][0]) < TIE) | (D.tie_margin(t["thr"][0]) < TIE)[:, None]
    s, sp = D.separation_truth(**_sep_args(i)), D.separation_truth(**_sep_args(i, True))
    pa = (D.tie_margin(s["d"][0]) < TIE) | (D.tie_margin(sp["d"][0]) < TIE)
    pa |= ((D.tie_margin(s["dist"][0]) < TIE) | (D.tie_margin(sp["dist"][0]) < TIE))[:, None]
    el = ((D.tie_margin(s["g_a"][0]) < TIE) | (D.tie_margin(s["g_b"][0]) < TIE)) & ~s["zeros"]
    el[:, C - 1, :] |= pa  # a pixel-level tie: move the pixel's last channel
    first = np.zeros((N, C, P), bool)
    first[:, C - 1, :] = px
    return np.flatnonzero(first.ravel()), np.flatnonzero(el.ravel())


def sep_expected(x, **kw):
    out = D.separation(**kw)
    out["att"] = D.dam(x)
    out["plain_dist"] = D.separation(kw["a"], kw["b"], None, None, None, None, None)["dist"]
    return out


def sep_truth(x, **kw):
    out = D.separation_truth(**kw)
    out["plain_dist"] = D.separation_truth(kw["a"], kw["b"], None, None, None, None,
                                           None)["dist"]
    out.update(D.dam_truth(x))
    return out


SEP_ROUNDED = ("d", "dist", "plain_dist", "g_a", "g_b")


def sep_check(c, got, exp, tru):
    bad, fig = [], {}
    for name in ("att", "a_out", "b_out"):
        _exact(name, got[name], exp[name], bad)
    # att is avg (rounded once) where it is kept: the bytes above, and the bar here
    avg, bavg, _ = tru["avg"]
    kept = np.asarray(exp["att"]) != 0
    _bounded("att", got["att"], (np.where(kept, avg, 0.0), np.where(kept, bavg, 0.0), 1.0), bad,
             fig)
    zero = np.zeros(tru["zeros"].shape, np.float32)
    for name in SEP_ROUNDED:
        _bounded(name, got[name], tru[name], bad, fig,
                 (tru["zeros"], zero) if name in ("g_a", "g_b") else None)
    return bad, fig


def sep_caps(c, tru):
    return [(k,) + tru[k] for k in SEP_ROUNDED + ("avg", "thr")], []


def sep_run(c):
    import torch
    from tlod.da.idf import dam, plain_distance, separation
    i = sep_inputs(c)
    N, C, P = i["x"].shape
    r4 = lambda v: _t(v.reshape(N, C, c.H, c.W))
    r3 = lambda v: _t(v.reshape(N, c.H, c.W))
    a, b = r4(i["a"]).requires_grad_(True), r4(i["b"]).requires_grad_(True)
    ao, bo, dist = separation(a, b, r3(i["att_a"]), r3(i["att_b"]))
    saved = dist.grad_fn.saved_tensors  # a, b, att_a, att_b, d
    d = saved[4]
    assert len(saved) == 5 and d.shape == (N, c.H, c.W)
    assert torch.allclose(d.double().mean((1, 2)), dist.double(), rtol=1e-6, atol=0)
    loss = (dist * _t(i["g_dist"])).sum()
    if c.mode != "dist":
        loss = loss + (ao * r4(i["g_a_out"])).sum() + (bo * r4(i["g_b_out"])).sum()
    loss.backward()
    flat = lambda v, k: _np(v).reshape(N, k, P) if k else _np(v).reshape(N, P)
    return {"att": flat(dam(r4(i["x"])), 0), "a_out": flat(ao, C), "b_out": flat(bo, C),
            "d": flat(d, 0), "dist": _np(dist), "plain_dist": _np(plain_distance(a, b)),
            "g_a": flat(a.grad, C), "g_b": flat(b.grad, C)}


# ------------------------------------------------------------------ what is compared, and how
Family =namedtuple("Family", "cases inputs restate truth check caps run")
FAMILIES = {
    "dl": Family(DL_CASES, dl_inputs, D.domain_losses, D.domain_losses_truth, dl_check, dl_caps,
                 dl_run),
    "us": Family(US_CASES, us_inputs, D.us_daf, D.us_daf_truth, us_check, us_caps, us_run),
    "nll": Family(NLL_CASES, nll_inputs, D.masked_nll2, D.masked_nll2_truth, nll_check, nll_caps,
                  nll_run),
    "kd": Family(KD_CASES, kd_inputs, D.kd_kl, D.kd_kl_truth, kd_check, kd_caps, kd_run),
    "pa": Family(PA_CASES, pa_inputs, D.pa_atf, D.pa_atf_truth, pa_check, pa_caps, pa_run),
    "sep": Family(SEP_CASES, sep_inputs, sep_expected, sep_truth, sep_check, sep_caps, sep_run),
}
ALL = [(fam, c) for fam, spec in FAMILIES.items() for c in spec.cases]
ALL_IDS = [f"{fam}-{c.name}" for fam, c in ALL]


def expected(fam, case, **kw):
    return FAMILIES[fam].restate(**FAMILIES[fam].inputs(case), **kw)


def truth(fam, case):
    return FAMILIES[fam].truth(**FAMILIES[fam].inputs(case))


def check(fam, case, got, exp, tru):
    """got (from the device, or from a restatement with a defect put in) against the
    restatement exp and the truth tru: (violations, figures); figures maps each compared
    output to (worst error in u of its scale, worst error / bar)."""
    return FAMILIES[fam].check(case, got, exp, tru)


def _exact(name, got, exp, bad):
    g, e = np.asarray(got, np.float32), np.asarray(exp, np.float32)
    if g.shape != e.shape:
        g = g.reshape(e.shape) if g.size == e.size else g
    if g.shape != e.shape or _bytes(g) != _bytes(e):
        n = int(np.count_nonzero(g.ravel().view(np.int32) != e.ravel().view(np.int32))) \
            if g.shape == e.shape else -1
        bad.append(f"{name}: {n} of {e.size} elements differ from the restatement")


def _bounded(name, got, tru, bad, fig, exact=None):
    """|got - truth| <= bar element by element; the elements of the mask exact[0] are compared
    with the bytes exact[1] instead."""
    t, bar, scale = (np.asarray(x, np.float64) for x in tru)
    g32 = np.asarray(got, np.float32).reshape(t.shape)
    g = g32.astype(np.float64)
    bar, scale = np.broadcast_to(bar, t.shape), np.broadcast_to(scale, t.shape)
    held = np.zeros(t.shape, bool) if exact is None else exact[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(g - t)
        err = np.where(np.isfinite(err), err, np.inf)
        err = np.where(held, 0.0, err)
        over = err > bar
        inu = np.where(scale > 0, err / (U * np.where(scale > 0, scale, 1)), 0.0)
        ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1), 0.0)
    fig[name] = (float(inu.max()) if inu.size else 0.0, float(ratio.max()) if ratio.size else 0.0)
    if over.any():
        i = int(np.argmax(np.where(over, err / np.maximum(bar, 1e-300), 0)))
        bad.append(f"{name}: {int(over.sum())} of {t.size} beyond the bar, worst at {i}: "
                   f"got {g.ravel()[i]!r} truth {t.ravel()[i]!r} bar {bar.ravel()[i]:.3e}")
    if held.any() and _bytes(g32[held]) != _bytes(np.asarray(exact[1], np.float32)[held]):
        n = int(np.count_nonzero(g32[held].view(np.int32)
                                 != np.asarray(exact[1], np.float32)[held].view(np.int32)))
        bad.append(f"{name}: {n} of {int(held.sum())} contract zeros differ")


# ------------------------------------------------------------------ on the device
dev = "cuda"


def _t(a, grad=False):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t.requires_grad_(True) if grad else t


def _np(t):
    return t.detach().cpu().numpy()


def _same_bytes(a, b, what):
    assert a.keys() == b.keys()
    flat = lambda v: np.concatenate([np.ravel(x) for x in v]) if isinstance(v, list) else v
    for k in a:
        assert _bytes(flat(a[k])) == _bytes(flat(b[k])), f"{what}: {k} differs"


def _report(fam, case, fig, what="device"):
    for name, (inu, ratio) in sorted(fig.items()):
        print(f"FIGURE {what} {fam}-{case.name} {name}: {inu:.4f} u of scale, "
              f"{ratio:.3f} of the bar")


@pytest.mark.gpu
@pytest.mark.parametrize("fam,case", ALL, ids=ALL_IDS)
def test_device_against_restatement_and_truth(fam, case):
    got = FAMILIES[fam].run(case)
    bad, fig = check(fam, case, got, expected(fam, case), truth(fam, case))
    _report(fam, case, fig)
    assert not bad, "\n".join(bad)
    _same_bytes(got, FAMILIES[fam].run(case), f"{fam}-{case.name} run twice")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in US_CASES if (c.Hs, c.Ws) == (c.Ht, c.Wt)],
                         ids=lambda c: c.name)
def test_us_daf_packed_is_the_split_result(case):
    got = us_run_packed(case)
    bad, fig = check("us", case, got, expected("us", case), truth("us", case))
    _report("us", case, fig, "device packed")
    assert not bad, "\n".join(bad)
    _same_bytes(got, us_run(case), f"us-{case.name} packed against split")
    _same_bytes(got, us_run_packed(case), f"us-{case.name} packed run twice")


@pytest.mark.gpu
@pytest.mark.parametrize("gamma", [0.0, -0.5])
def test_focal_refuses_a_gamma_that_is_not_positive(gamma):
    """include/tlod_idf.h: gamma > 0; the forward is refused before anything is launched, and
    so is the backward called on its own."""
    import torch
    from tlod import _lib
    from tlod.da.idf import domain_losses
    z = _t(np.array([[0.5, -0.5], [40.0, 0.0]], np.float32), True)
    with pytest.raises(RuntimeError, match="gamma must be positive"):
        domain_losses(z, 0, z, 0, gamma)
    zi, g, out = z.detach(), torch.ones(3, device=dev), torch.full((2, 2), 7.0, device=dev)
    st = _lib.lib().tlod_idf_domain_loss_bwd_f32(
        _lib.ptr(zi), 2, 0, _lib.ptr(zi), 2, 0, float(gamma), _lib.ptr(g), _lib.ptr(out),
        _lib.ptr(out), _lib.stream_of(zi))
    assert st != 0 and b"gamma must be positive" in _lib.lib().tlod_last_error()
    assert bool((out == 7.0).all())  # nothing was written
