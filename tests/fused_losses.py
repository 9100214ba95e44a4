"""The fused RPN, RCNN and DAF losses of csrc/losses.hip restated in numpy float32 operation by
operation, and the fp64 truth (with a derived error bar per element) they are measured
against.  u = 2^-24 throughout, half a float32 ulp of a value in [1, 2).

Exact pieces: plain IEEE float32 operations, which the device (built without contraction)
must equal bit for bit (tests/test_fused_losses_gpu.py):

  smooth_l1     the element loss out_w * l and its derivative out_w * (quad ? s2*d : sign(d))
                * in_w, with 1.f/s2 and 0.5f/s2 as float32 divisions and s2 = sigma * sigma
                rounded to float32;
  rpn           dbbox = (gloss[1] / B) * dp, count = max(kept, 1), the row -> (image, offset,
                class plane) map, exact zeros at ignored anchors, at images B..B_total-1 and
                everywhere when no anchor is kept;
  rcnn          box_sel, dbox = dp * (gloss[1] / R) at the label's four columns and 0.0
                elsewhere, exact zeros in rows R..R_total-1;
  da            ins_label(r) = need[r // 256] while r // 256 < B, else 1.

Loss scalars are a double sum of float32 terms, divided, rounded once: loss_scalar restates
them as float32(math.fsum(terms) / denom).  fsum is the exactly rounded sum, the device adds in
a fixed tree; the two quotients can differ only where the exact quotient lies within about
N * 2^-53 (relative) of a float32 rounding tie, so equality is expected and 1 ulp allowed.  For
the smooth-L1 losses the terms themselves are exact, so that is the whole difference.

Transcendental pieces (LogSoftmax2, the C-way softmax with its sequential float32 z, the BCE
term and gradient, the consistency mean) go through expf / logf.  They are restated here with
numpy's float32 exp / log for the CPU half only; the device is compared with the fp64 truth.

The bars.  Every truth function returns, next to each fp64 value, a first-order bound on what
a float32 evaluation in the kernel's order can be off by, assuming expf and logf are within
ULP_EXP = ULP_LOG = 2 ulp (a relative 4 u; the upper end of what the HIP math API reference
states for ocml: 1 ulp for expf and logf, and well inside OpenCL's 3 ulp, which ocml is built
to).  One percent is added for the second-order terms and 2^-126 where a result may underflow.
Rounding errors of subtractions of inputs (x - m, 1 - x) are not bounded but computed: the
truth knows the operands.  Adding a term e >= 0 to a partial sum S errs by at most
min(e, u * (S + e)).  With t = -|a - b|, e = exp(t), s = 1 + e, lz = log(s):

  ls2       err(s) <= e*dt + 4u*e + min(e, u*s); err(lz) <= err(s)/s + 4u*lz;
            err(ls_c) <= dt_c + err(lz) + u*|ls_c|             (at most 8.2 u + 2 u |ls|)
  p = exp(ls)                 p * (err(ls) + 4u)                (at most 12.2 u, about 5.5 u)
  score gradients g*(p - y)   |g| * (err(p) + 3u*|p - y|)       (g = gloss / count; <= 15.5 u)
  CE / NLL loss               mean err(term) + u*|loss|
  C-way z                     zeta = (sum e_k*(dt_k + 4u) + sum min(e_k, u*S_k)) / z, without
                              the 4u where t_k = 0: expf(0) is exactly 1
  cls_prob                    (4u + zeta + u) * max(p, 2^-20), measured from the fp64 softmax
                              of the kernel's exponents fl32(x_c - m) (dt_c = 0 in zeta too)
  C-way CE term               dt_lab + zeta + 4u*|lz| + u*|term|
  BCE term T                  dx/(1 - x) + 4u*|T|               (dx = err of 1 - x; y = 0 only)
  BCE gradient                4u relative: x - y, 1 - x, the product, the quotient
  consistency mean c          mean err(p) + u*c
  consistency loss            sum (2|e|*(err(c) + u|e|) + u*e^2) + u*loss,  e = x - c
  dins                        7u*|gb*bce| + 3u*|gm*2(x - c)| + |2 gm| * err(c)

Each is capped at CAP = 16 u times its scale (the element for cls_prob above 2^-20,
max(1, |term|) for loss terms, |g| for score gradients): the worst case of the C - 1 additions
of z alone is (C - 1) u, over the cap for C = 21, and a kernel that needs it is worth a look.
dins carries |2 gm| * err(c) on top of its scale |gb*bce| + |gm*2(x - c)|: at x = c the scale
shrinks to |gb*bce| >= |gloss| / n while even a correctly rounded c is off by u*c / 2.

Everything a defect could plausibly touch goes through a module-level name (cut_test, sign,
kept_count, box_denom, plane_stride, rows_visited, dead_rows, box_index, dbox_class, lse,
MINIBATCH, past_blocks_label, need_at, cons_channel, cons_for, LOG_CLAMP, GRAD_FLOOR), so
tests/test_fused_losses_cpu.py can swap one for a defective version.

No torch and no tlod at import.
"""
import math

import numpy as np

from fused_optim import TINY, Watch  # noqa: F401  (one Watch for both restatements)
import fused_optim as _fo

f32 = np.float32
U = 2.0 ** -24
ULP_EXP = ULP_LOG = 2
XE, XL = 2 * ULP_EXP * U, 2 * ULP_LOG * U  # relative error of expf, logf
CAP = 16 * U
SLACK = 1.01
PFLOOR = 2.0 ** -20
MINIBATCH = 256
LOG_CLAMP = f32(-100.0)
GRAD_FLOOR = f32(1e-12)


def _w(x):
    return _fo._w(x)


def _a(x):
    return np.ascontiguousarray(x, dtype=np.float32)


# ------------------------------------------------------------------ exact pieces
def cut_test(ad, cut):
    return ad < cut


def sign(d):
    return np.where(d > 0, f32(1), np.where(d < 0, f32(-1), f32(0))).astype(np.float32)


def sigma2(sigma):
    return f32(sigma) * f32(sigma)


def smooth_l1(pred, tgt, in_w, out_w, s2):
    """(out_w * l, dpred) of smooth_l1 of csrc/losses.hip, elementwise."""
    pred, tgt, in_w, out_w, s2 = _a(pred), _a(tgt), _a(in_w), _a(out_w), f32(s2)
    d = _w(in_w * _w(pred - tgt))
    ad = np.abs(d)
    quad = cut_test(ad, f32(1) / s2)
    lq = _w(np.where(quad, d * d, f32(0))) * _w(s2 * f32(0.5))
    ll = ad - _w(f32(0.5) / s2)
    l = _w(np.where(quad, lq, ll))
    inner = _w(np.where(quad, s2 * d, sign(d)))
    return _w(out_w * l), _w(_w(out_w * inner) * in_w)


def loss_scalar(terms, denom):
    with np.errstate(divide="ignore", invalid="ignore"):
        return f32(np.float64(math.fsum(float(t) for t in np.ravel(terms))) / np.float64(denom))


def kept_count(kept):
    return max(kept, 1)


def box_denom(n, n_total):
    """What the box loss and its gradient are divided by: the B images (R rows) of the loss."""
    return n


def plane_stride(A, H, W):
    """Distance between the two class planes of an anchor in RPN_cls_score (B, 2A, H, W)."""
    return A * H * W


def rpn_row_map(r, A, H, W):
    """Row r of the (B*A*H*W, 2) score view -> (image, in-image offset, index of class 0,
    index of class 1) in the raw (B, 2A, H, W) tensor."""
    ahw = A * H * W
    b = r // ahw
    q = r - b * ahw
    i0 = b * 2 * ahw + q
    return b, q, i0, i0 + plane_stride(A, H, W)


def rows_visited(rows):
    """The rows the forward's four-in-flight loop reaches: all of them."""
    return np.arange(rows)


def dead_rows(n):
    """Gradient of the n elements that take no part in the loss."""
    return np.zeros(n, dtype=np.float32)


def box_index(r, lab, C, agnostic):
    """Flat offset in bbox_pred of the four values the forward gathers for row r."""
    return r * 4 if agnostic else r * 4 * C + 4 * lab


def dbox_class(lab, C, agnostic):
    """The class whose four columns of row r take the box gradient."""
    return np.zeros_like(lab) if agnostic else lab


def need_at(need, i):
    return need[i]


def past_blocks_label():
    return f32(1)


def ins_label(r, need, B):
    """InstanceLabelResizeLayer: need[r // 256] while that block has an image, else 1."""
    r = np.asarray(r)
    i = r // MINIBATCH
    need = _a(need)
    inside = need_at(need, np.minimum(i, B - 1)) if B > 0 else np.zeros(r.shape, np.float32)
    return np.where(i < B, inside, past_blocks_label()).astype(np.float32)


def cons_channel(dom):
    """The softmax channel averaged for the consistency target: 1 (source), 0 (target)."""
    return 1 if dom == 0 else 0


def cons_for(dom, cons):
    return cons[dom]


# ------------------------------------------------------------------ transcendental pieces
def log_softmax2(a, b):
    a, b = _a(a), _a(b)
    m = np.maximum(a, b)
    ta, tb = _w(a - m), _w(b - m)
    lz = _w(np.log(_w(_w(np.exp(ta)) + _w(np.exp(tb)))))
    return _w(ta - lz), _w(tb - lz)


def lse(s):
    """(m, z, log z) per row of s (R, C): the running fmaxf, the sequential float32 z."""
    m = s[:, 0].copy()
    for c in range(1, s.shape[1]):
        m = np.maximum(m, s[:, c])
    z = np.zeros(s.shape[0], dtype=np.float32)
    for c in range(s.shape[1]):
        z = _w(z + _w(np.exp(_w(s[:, c] - m))))
    with np.errstate(divide="ignore"):
        return m, z, np.log(z)


def bce_term(x, y):
    with np.errstate(divide="ignore"):  # log(0) = -inf is clamped at once
        lx = np.maximum(np.log(x), LOG_CLAMP)
        l1x = np.maximum(np.log(_w(f32(1) - x)), LOG_CLAMP)
    with np.errstate(invalid="ignore"):
        return _w(_w((y - f32(1)) * l1x) - _w(y * lx))


def bce_grad(x, y):
    with np.errstate(invalid="ignore", divide="ignore"):
        return _w(_w(x - y) / np.maximum(_w(_w(f32(1) - x) * x), GRAD_FLOOR))


# ------------------------------------------------------------------ the three families
def rpn(score, labels, bbox, tgt, inw, outw, B, B_total, A, H, W, sigma, gloss):
    """Forward and backward of rpn_losses.  Returns loss_cls, loss_box, count, dscore, dbbox
    (the gradients flat, in the layout of score / bbox)."""
    score, bbox, lab = _a(score).ravel(), _a(bbox).ravel(), _a(labels).ravel()
    ahw = A * H * W
    rows, lne = B * ahw, B * ahw * 4
    s2 = sigma2(sigma)
    vis = rows_visited(rows)
    kept = vis[lab[vis] != -1]
    _, _, i0, i1 = rpn_row_map(kept, A, H, W)
    l0, l1 = log_softmax2(score[i0], score[i1])
    terms = -np.where(lab[kept].astype(np.int64) == 1, l1, l0)
    count = kept_count(len(kept))
    lb, _ = smooth_l1(bbox[:lne], _a(tgt).ravel(), _a(inw).ravel(), _a(outw).ravel(), s2)
    out = {"loss_cls": loss_scalar(terms, count), "count": f32(count),
           "loss_box": loss_scalar(lb, box_denom(B, B_total))}
    g = _a(gloss)
    with np.errstate(divide="ignore", invalid="ignore"):
        gc, gb = _w(g[0] / f32(count)), _w(g[1] / f32(box_denom(B, B_total)))
    dscore = dead_rows(B_total * 2 * ahw)
    keptb = np.flatnonzero(lab != -1)  # the backward goes over every row
    _, _, i0, i1 = rpn_row_map(keptb, A, H, W)
    l0, l1 = log_softmax2(score[i0], score[i1])
    one = lab[keptb].astype(np.int64) == 1
    with np.errstate(invalid="ignore"):
        dscore[i0] = _w(gc * _w(_w(np.exp(l0)) - np.where(one, f32(0), f32(1))))
        dscore[i1] = _w(gc * _w(_w(np.exp(l1)) - np.where(one, f32(1), f32(0))))
        _, dp = smooth_l1(bbox[:lne], _a(tgt).ravel(), _a(inw).ravel(), _a(outw).ravel(), s2)
        dbbox = gb * dead_rows(B_total * 4 * ahw)
        dbbox[:lne] = _w(gb * dp)
    out.update(dscore=dscore, dbbox=dbbox)
    return out


def rcnn(cls, box, labels, tgt, inw, outw, R, R_total, C, agnostic, sigma, gloss):
    """Forward and backward of rcnn_losses: prob, box_sel, loss_cls, loss_box, dcls, dbox."""
    cls, box = _a(cls).reshape(R_total, C), _a(box)
    bw = 4 if agnostic else 4 * C
    lab = np.asarray(labels, dtype=np.int64).ravel()
    lab = np.where((lab < 0) | (lab >= C), 0, lab)
    tgt, inw, outw = (_a(x).reshape(R, 4) for x in (tgt, inw, outw))
    s2 = sigma2(sigma)
    s = cls[:R]
    r = np.arange(R)
    m, z, lz = lse(s)
    with np.errstate(invalid="ignore", divide="ignore"):
        prob = _w(_w(np.exp(_w(s - m[:, None]))) / z[:, None])
        terms = -_w(_w(s[r, lab] - m) - lz)
    sel = box.ravel()[box_index(r, lab, C, agnostic)[:, None] + np.arange(4)]
    lb, _ = smooth_l1(sel, tgt, inw, outw, s2)
    out = {"prob": prob, "box_sel": sel, "loss_cls": loss_scalar(terms, box_denom(R, R_total)),
           "loss_box": loss_scalar(lb, box_denom(R, R_total))}
    g = _a(gloss)
    gc, gb = _w(g[0] / f32(box_denom(R, R_total))), _w(g[1] / f32(box_denom(R, R_total)))
    dcls = dead_rows(R_total * C).reshape(R_total, C)
    onehot = (np.arange(C)[None, :] == lab[:, None]).astype(np.float32)
    with np.errstate(invalid="ignore"):
        dcls[:R] = _w(gc * _w(prob - onehot))
    dbox = dead_rows(R_total * bw).reshape(R_total, bw)
    dbox[:R] = 0.0
    cols = 4 * dbox_class(lab, C, agnostic)[:, None] + np.arange(4)
    ok = cols[:, 0] < bw
    at = box.reshape(R_total, bw)[r[ok, None], cols[ok]]
    _, dp = smooth_l1(at, tgt[ok], inw[ok], outw[ok], s2)
    dbox[r[ok, None], cols[ok]] = _w(dp * gb)
    out.update(dcls=dcls, dbox=dbox)
    return out


def da(scores, needs, inss, gloss):
    """Forward and backward of daf_da_losses.  scores / needs / inss: (source, target);
    gloss in the kernel's order [img_s, ins_s, cst_s, img_t, ins_t, cst_t].  Returns loss (6,
    same order), cons (2), dscore_s, dscore_t, dins_s, dins_t."""
    g = _a(gloss)
    loss, cons, fwd = np.zeros(6, np.float32), np.zeros(2, np.float32), []
    for dom in (0, 1):
        sc, need, x = _a(scores[dom]), _a(needs[dom]).ravel(), _a(inss[dom]).ravel()
        B, _, H, W = sc.shape
        npix, n = B * H * W, x.size
        b = np.arange(npix) // (H * W)
        s0, s1 = sc[:, 0].ravel(), sc[:, 1].ravel()
        l0, l1 = log_softmax2(s0, s1)
        one = need_at(need, b).astype(np.int64) == 1
        cons[dom] = loss_scalar(_w(np.exp((l0, l1)[cons_channel(dom)])), npix)
        y = ins_label(np.arange(n), need, B)
        e = _w(x - cons[dom])
        loss[3 * dom + 0] = loss_scalar(-np.where(one, l1, l0), npix)
        loss[3 * dom + 1] = loss_scalar(bce_term(x, y), max(n, 1))
        loss[3 * dom + 2] = loss_scalar(_w(e * e), 1)
        fwd.append((sc, x, y, l0, l1, one, npix, n))
    out = {"loss": loss, "cons": cons}
    for dom, (sc, x, y, l0, l1, one, npix, n) in enumerate(fwd):
        gi = _w(g[3 * dom] / f32(npix))
        gb = _w(g[3 * dom + 1] / f32(max(n, 1)))
        gm2 = _w(g[3 * dom + 2] * f32(2))
        c = cons_for(dom, cons)
        ds = np.empty(sc.shape, np.float32)
        shp = ds[:, 0].shape
        ds[:, 0] = _w(gi * _w(_w(np.exp(l0)) - np.where(one, f32(0), f32(1)))).reshape(shp)
        ds[:, 1] = _w(gi * _w(_w(np.exp(l1)) - np.where(one, f32(1), f32(0)))).reshape(shp)
        with np.errstate(invalid="ignore"):
            di = _w(_w(gb * bce_grad(x, y)) + _w(gm2 * _w(x - c)))
        out["dscore_" + "st"[dom]], out["dins_" + "st"[dom]] = ds, di
    return out


# ------------------------------------------------------------------ the fp64 truth
def _d(x):
    return np.asarray(x, dtype=np.float64)


def _sub_err(a, b):
    """|fl32(a - b) - (a - b)| for float32 operands held as float64."""
    return np.abs(_d(a.astype(np.float32) - b.astype(np.float32)) - (a - b))


def ls2_truth(a, b):
    """fp64 2-way log-softmax of float32 logits: ((ls0, ls1), (p0, p1)) and their bars."""
    a, b = _d(a), _d(b)
    m = np.maximum(a, b)
    ta, tb = a - m, b - m
    dta, dtb = _sub_err(a, m), _sub_err(b, m)
    t = np.minimum(ta, tb)
    e = np.exp(t)
    s, lz = 1 + e, np.log1p(e)
    err_lz = (e * (dta + dtb) + XE * e + np.minimum(e, U * s)) / s + XL * lz
    ls = (ta - lz, tb - lz)
    bls = tuple(SLACK * (dt + err_lz + U * np.abs(l)) for dt, l in zip((dta, dtb), ls))
    p = tuple(np.exp(l) for l in ls)
    bp = tuple(SLACK * q * (bl + XE) + TINY for q, bl in zip(p, bls))
    return ls, bls, p, bp


def smooth_l1_truth(pred, tgt, in_w, out_w, s2):
    pred, tgt, in_w, out_w, s2 = _d(pred), _d(tgt), _d(in_w), _d(out_w), float(s2)
    d = in_w * (pred - tgt)
    ad = np.abs(d)
    quad = ad < 1.0 / s2
    l = np.where(quad, d * d * (s2 / 2), ad - 0.5 / s2)
    return out_w * l, out_w * np.where(quad, s2 * d, np.sign(d)) * in_w


def _mean_bar(value, term_bars, denom, scale):
    """Bar of a double sum of float32 terms, divided and rounded once; capped at CAP * scale."""
    return min(SLACK * (float(np.sum(term_bars)) / denom + U * abs(value)), CAP * scale)


def _mean_scale(terms, denom):
    """max(1, |term|) averaged over the terms (1 when there are none)."""
    return float(np.maximum(1, np.abs(terms)).sum()) / denom if np.size(terms) else 1.0


def rpn_truth(score, labels, bbox, tgt, inw, outw, B, B_total, A, H, W, sigma, gloss):
    """name -> (fp64 value, bar, scale).  loss_box and dbbox carry the bar of the restatement
    (the device is held to the restatement itself)."""
    score, bbox, lab = _d(score).ravel(), _d(bbox).ravel(), _d(labels).ravel()
    ahw = A * H * W
    rows, lne = B * ahw, B * ahw * 4
    s2 = float(sigma2(sigma))
    g = _d(_a(gloss))
    r = np.arange(rows)
    b = r // ahw
    i0 = b * 2 * ahw + (r - b * ahw)
    i1 = i0 + ahw
    kept = lab != -1
    one = lab.astype(np.int64) == 1
    ls, bls, p, bp = ls2_truth(score[i0], score[i1])
    nk = int(kept.sum())
    count = max(nk, 1)
    terms = -np.where(one, ls[1], ls[0])[kept]
    tb = np.minimum(np.where(one, bls[1], bls[0])[kept], CAP * np.maximum(1, np.abs(terms)))
    lc = terms.sum() / count
    gc = g[0] / count
    ds, bds = np.zeros(B_total * 2 * ahw), np.zeros(B_total * 2 * ahw)
    for idx, k, y in ((i0, 0, np.where(one, 0.0, 1.0)), (i1, 1, np.where(one, 1.0, 0.0))):
        ds[idx[kept]] = (gc * (p[k] - y))[kept]
        bds[idx[kept]] = (abs(gc) * np.minimum(SLACK * (bp[k] + 3 * U * np.abs(p[k] - y)),
                                               CAP))[kept]
    lt, dp = smooth_l1_truth(bbox[:lne], _d(tgt).ravel(), _d(inw).ravel(), _d(outw).ravel(), s2)
    db = np.zeros(B_total * 4 * ahw)
    db[:lne] = g[1] / B * dp
    sc = _mean_scale(terms, count)
    return {"loss_cls": (lc, _mean_bar(lc, tb, count, sc), sc), "count": (float(count), 0.0, 1.0),
            "dscore": (ds, bds, abs(gc)),
            "loss_box": (lt.sum() / B, 6 * U * np.abs(lt).sum() / B, np.abs(lt).sum() / B),
            "dbbox": (db, 6 * U * np.abs(db), np.abs(db))}


def rcnn_truth(cls, box, labels, tgt, inw, outw, R, R_total, C, agnostic, sigma, gloss):
    cls = _d(cls).reshape(R_total, C)
    bw = 4 if agnostic else 4 * C
    box = _d(box).reshape(R_total, bw)
    lab = np.asarray(labels, dtype=np.int64).ravel()
    lab = np.where((lab < 0) | (lab >= C), 0, lab)
    tgt, inw, outw = (_d(x).reshape(R, 4) for x in (tgt, inw, outw))
    s2 = float(sigma2(sigma))
    g = _d(_a(gloss))
    s = cls[:R]
    r = np.arange(R)
    m = s.max(1, keepdims=True)
    t = s - m
    dt = _sub_err(s, np.broadcast_to(m, s.shape))
    e = np.exp(t)
    S = np.cumsum(e, 1)
    z = S[:, -1:]
    add = np.minimum(e, U * S)
    add[:, 0] = 0.0  # 0 + e is exact
    xe = np.where(t == 0, 0.0, XE)  # expf(0) is exactly 1: the largest term carries no error
    zeta = ((e * (dt + xe)).sum(1, keepdims=True) + add.sum(1, keepdims=True)) / z
    p = e / z
    # cls_prob is measured from the kernel's own exponents t32 = fl32(s - m), an exact piece:
    # at t in [-16, -8) that one rounding alone is worth up to 8 u of the element, which no
    # float32 evaluation can avoid and a bar of 16 u of the element could not carry
    e32 = np.exp(_d(s.astype(np.float32) - m.astype(np.float32)))
    S32 = np.cumsum(e32, 1)
    add32 = np.minimum(e32, U * S32)
    add32[:, 0] = 0.0
    pk = e32 / S32[:, -1:]
    zeta32 = ((xe * e32).sum(1, keepdims=True) + add32.sum(1, keepdims=True)) / S32[:, -1:]
    bpk = np.minimum(SLACK * (xe + zeta32 + U), CAP) * np.maximum(pk, PFLOOR) + TINY
    shift = SLACK * p * (dt + (e * dt).sum(1, keepdims=True) / z) + TINY  # |pk - p| at most
    bp = bpk + shift
    lz = np.log(z[:, 0])
    terms = -(t[r, lab] - lz)
    tb = np.minimum(SLACK * (dt[r, lab] + zeta[:, 0] + XL * np.abs(lz) + U * np.abs(terms)),
                    CAP * np.maximum(1, np.abs(terms)))
    lc = terms.sum() / R
    gc, gb = g[0] / R, g[1] / R
    onehot = (np.arange(C)[None, :] == lab[:, None]).astype(np.float64)
    dcls, bdc = np.zeros((R_total, C)), np.zeros((R_total, C))
    dcls[:R] = gc * (p - onehot)
    bdc[:R] = abs(gc) * np.minimum(bp + SLACK * 3 * U * np.abs(p - onehot), CAP)
    cols = 4 * (np.zeros_like(lab) if agnostic else lab)[:, None] + np.arange(4)
    sel = box[r[:, None], cols]
    lt, dp = smooth_l1_truth(sel, tgt, inw, outw, s2)
    dbox = np.zeros((R_total, bw))
    dbox[r[:, None], cols] = dp * gb
    sc = _mean_scale(terms, R)
    return {"prob": (pk, bpk, np.maximum(pk, PFLOOR)), "prob_pure": (p, shift, p),
            "loss_cls": (lc, _mean_bar(lc, tb, R, sc), sc), "dcls": (dcls, bdc, abs(gc)),
            "box_sel": (sel, np.zeros_like(sel), 1.0),
            "loss_box": (lt.sum() / R, 6 * U * np.abs(lt).sum() / R, np.abs(lt).sum() / R),
            "dbox": (dbox, 6 * U * np.abs(dbox), np.abs(dbox))}


def da_truth(scores, needs, inss, gloss):
    g = _d(_a(gloss))
    loss, bloss, sloss, cons, bcons, out = (np.zeros(6), np.zeros(6), np.ones(6), np.zeros(2),
                                            np.zeros(2), {})
    floor, clamp = float(GRAD_FLOOR), float(LOG_CLAMP)
    for dom in (0, 1):
        sc, need, x = _d(scores[dom]), _d(needs[dom]).ravel(), _d(inss[dom]).ravel()
        B, _, H, W = sc.shape
        npix, n = B * H * W, x.size
        lab1 = (need.astype(np.int64) == 1)[:, None, None] & np.ones((B, H, W), bool)
        ls, bls, p, bp = ls2_truth(sc[:, 0], sc[:, 1])
        ch = 1 if dom == 0 else 0
        c = p[ch].sum() / npix
        bc = _mean_bar(c, bp[ch], npix, 1.0)
        terms = -np.where(lab1, ls[1], ls[0])
        tb = np.minimum(np.where(lab1, bls[1], bls[0]), CAP * np.maximum(1, np.abs(terms)))
        li = terms.sum() / npix
        blk = np.arange(n) // 256
        y = np.where(blk < B, need[np.minimum(blk, B - 1)], 1.0)
        om = 1 - x
        dom_ = _sub_err(np.ones_like(x), x)
        with np.errstate(divide="ignore", invalid="ignore"):
            lx, l1x = np.maximum(np.log(x), clamp), np.maximum(np.log(om), clamp)
            T = np.where(y == 1, -lx, -l1x)  # (y - 1) * l1x - y * lx for y in {0, 1}
            bT = SLACK * (np.where((y == 0) & (om > 0), dom_ / np.where(om > 0, om, 1), 0.0)
                          + XL * np.abs(T))
            bT = np.where(np.abs(T) == -clamp, 0.0, np.minimum(bT, CAP * np.maximum(1, np.abs(T))))
        lb = T.sum() / max(n, 1)
        e = x - c
        lm = (e * e).sum()
        sm = float(np.maximum(1, e * e).sum())
        bm = min(SLACK * ((2 * np.abs(e) * (bc + U * np.abs(e)) + U * e * e).sum() + U * lm),
                 CAP * sm)
        si, sb = _mean_scale(terms, npix), _mean_scale(T, max(n, 1))
        loss[3 * dom:3 * dom + 3] = li, lb, lm
        sloss[3 * dom:3 * dom + 3] = si, sb, max(sm, 1.0)
        bloss[3 * dom:3 * dom + 3] = (_mean_bar(li, tb, npix, si),
                                      _mean_bar(lb, bT, max(n, 1), sb) if n else 0.0, bm)
        cons[dom], bcons[dom] = c, bc
        gi, gb, gm = g[3 * dom] / npix, g[3 * dom + 1] / max(n, 1), g[3 * dom + 2]
        ds, bds = np.zeros(sc.shape), np.zeros(sc.shape)
        for k, yk in ((0, np.where(lab1, 0.0, 1.0)), (1, np.where(lab1, 1.0, 0.0))):
            ds[:, k] = gi * (p[k] - yk)
            bds[:, k] = abs(gi) * np.minimum(SLACK * (bp[k] + 3 * U * np.abs(p[k] - yk)), CAP)
        t1 = gb * (x - y) / np.maximum(om * x, floor)
        t2 = gm * 2 * e
        bdi = SLACK * (7 * U * np.abs(t1) + 3 * U * np.abs(t2)) + abs(2 * gm) * bc
        out["dscore_" + "st"[dom]] = (ds, bds, abs(gi))
        out["dins_" + "st"[dom]] = (t1 + t2, bdi, np.abs(t1) + np.abs(t2) + abs(2 * gm))
    out["loss"], out["cons"] = (loss, bloss, sloss), (cons, bcons, 1.0)
    return out
