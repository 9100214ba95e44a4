"""The fused domain-adaptation losses restated in numpy, and the fp64 truth (with a derived
error bar per element) they are measured against: the IDF / EFocal domain losses
(csrc/idf.hip, csrc/selftrain.hip), the IDF attention map and separation kernels (csrc/idf.hip),
the US-DAF losses (csrc/us_daf.hip), the masked two-way NLL and the KD KL loss of PT-MAF
(csrc/pt_maf.hip) and the 14 PA-ATF terms (csrc/pa_atf.hip).  u = 2^-24 (fused_losses.U),
E = 2^-53 (double's rounding unit).

Three classes of expectation, by what the kernel text does.

Exact: plain IEEE float32 operations, compiled without contraction, so the device must give
the bytes of the numpy float32 restatement.
  us_daf_loss_bwd_kernel   everything, given the saved s and gate: gi = gloss / npix and
                gn = gloss / (4.f * max(n, 1)) as float32 divisions, q = p * (1 - p),
                (gi * (p - y)) * (q / fmaxf(q, 1e-12f)), de = -(y / (s + NEAR_0) - (1 - y) /
                ((1 - s) + NEAR_0)) and ((gn * w) * de) * (s * (1 - s)) with w the gate in
                column 0 and 1 elsewhere, y the domain label in column 0 and the RoI's scale
                label (scale_labels: area = (x2 - x1) * (y2 - y1), <= 400 / between / >= 10000)
                in columns 1..3.  s is rounded once (below) and tie-free in every case, so the
                restatement starts from float32(truth) and the gradients are compared as bytes;
  us_daf gate   e[0] > 0.5f, or the override: every case keeps e[0] 16 u or more from 0.5;
  masked_nll2   count (an integer sum), g = gout / count, +0.0 in every cell off the map, in
                every cell of an empty map, and the loss 0 of an empty map;
  focal         rows whose float32 softmax[label] is below 1e-6f: dz = (+0.0, -0.0) at (label,
                other), and the forward term -(1 - c)^gamma log c with c = (double)1e-6f;
  IDF           the modulation a * (1.f + att) (one add, one multiply); att = avg < thr ? 0 : avg
                given the rounded-once, tie-free avg and thr (a constant map has avg == thr in
                every pixel and keeps them all); g_a = g_b = +0.0 where the attention and the
                upstream gradients of the modulated maps are zero;
  PA-ATF        image gradients past the switch softplus(u) < 100: g * (+-0.0); an instance
                term with n == 2 label: g * 0 in every row.

Rounded once: evaluated in double from the float32 inputs and cast, so the expectation is
float32(truth), the truth in float64 from stable forms (log1p, and with x = z_other - z_label:
P = 1 / (1 + e^x), 1 - P = 1 / (1 + e^-x), log P = -log1p(e^x)).  The bar is half a float32 ulp
of the truth plus a first-order bound on the kernel's double error in its own order, with
exp, log, log1p and pow taken as 1 ulp (2 E relative):
  us_daf s      1 / (1 + exp(-z)): 6 E |s| (exp, the add, the quotient);
  CE (image)    x + log1p(exp(-x)) or log1p(exp(x)): 8 E |t|;
  dz_img        g (p - 1.0): p carries 4 E p absolute, the difference is exact or rounds once:
                |g| 5 E + 2 E |t|.  The 5 E |g| is absolute: at x = -20 the kernel's p - 1.0
                = -2.06e-9 keeps 53 - 29 = 24 bits, at x = -40 (4.2e-18 < E) p is 1.0 and the
                gradient exactly 0: no bit, and inside the bar;
  focal dz_ins  (g / R) (gamma q^(gamma-1) log p - q^gamma / p) p q, q = 1.0 - p: both terms
                have one sign; q carries rho = (4 E p + E q) / q relative, log p near 1 the
                same, and the terms go as q^gamma and q^(gamma+1):
                |t| ((gamma + 2) 5 E / q + 16 E), which stays below 12 (gamma + 2) E |g / R|.
                Where q is 0 in double (the label leads by 37 or more) the kernel gives 0; the
                truth there is below |g / R| e^-37 and the same bound covers it;
  EFocal dz_ins (g / R) e^(-gamma p) (gamma log p - 1 / p) p (1 - p): |t| (5 E / q + (16 + 4
                gamma) E).  No clamp: at x = 104 p = 6.8e-46 in double, log p = -104 and the
                gradient -(g / R) (include/tlod_selftrain.h: evaluated in double, no clamp; the
                float32 softmax of tests/ref_selftrain.py would give inf there).  Rows beyond
                that, where p underflows in double, are not in the header and not tested.
  KD KL         kl_row in double: z = s / T, l = (z - max z) - log sum exp(z - max z), KL = sum
                e^l1 (l1 - l2); out[0] = sum w KL / (sum w + 1), out[1] = sum w + 1 over the
                wmod weights (each once), dstudent = gout / (float)out[1] / T * w * e^l1_j ((l1_j
                - l2_j) - KL), +0.0 in rows of weight 0.  The truth (kd_kl_truth, np.longdouble)
                never forms the cancelling differences: KL = sum p1 (e^u - 1 - u) with u = log p2
                - log p1 from the differences s - t, and (l1_j - l2_j) - KL = sum_{c != j} p1_c
                (delta_j - delta_c).  The kernel's error is bounded per row from err(l_c) =
                a_c + zeta + 2 E |log Z| + E |l_c| (a_c: the two quotients and the subtraction,
                0 at the row's best class; zeta: the relative error of Z); (l1 - l2) - kl cancels
                in double, so the gradient's bound is absolute: |g w| p1_j (err(l1) + err(l2) +
                err(KL)), a few hundred E at logits of magnitude 100, inside the cap.
  IDF avg, thr  mean_c 1 / (1 + exp(-x)) over 16 channel slices, each quotient 4 E: (C / 16 + 24) E
                avg; thr the double mean of the float32 avg: (P / 64 + 12) E thr;
  IDF d, dist   e = (a - b) w + 1e-6 (the double 1e-6): a - b is exact, the product and the sum
                round, so e carries E (|(a - b) w| + |e|) absolute, which matters where the two
                cancel (|a - b| w near 1e-6); d = sqrt(sum e^2): err(ss) / (2 d) + E d; dist the
                double mean of the double d.  Both are loss terms: scale max(1, value);
  IDF g_a, g_b  g_a_out (1 + att_b) +- k e with k = g_dist / P * w / (double)(float)d, 0 where d
                is 0: the truth divides by the same float32 d.  3 E (|g_a_out (1 + att_b)| +
                |k e|) for the sum, which may cancel, plus |k| err(e) + 5 E |k e|;
  PA-ATF dz     image: g * +-1 / (1 + exp(-u)), 6 E |t|; instance: g (n - 2 label) / n * x (1 - x)
                with x = 1 / (1 + exp(-z)): 1.0 - x cancels, 12 E |t| + 5 E |g (n - 2 label) / n|
                x^2 absolute; CLUB: as dz_img.
Loss scalars (the focal / EFocal mean and the 14 PA-ATF terms: double sums, divided, cast):
float32(fsum(terms) / n) as fused_losses.loss_scalar, equality expected, 1 ulp allowed.  The
PA-ATF image terms are min(softplus(u), 100): 99.5 at a logit of 99.5, the clamp from 100 on.

Bounded float32: masked_nll2 forward and backward use LogSoftmax2, expf and logf exactly as
losses.hip: fused_losses.ls2_truth and its bars, unchanged.  The US-DAF forward element losses
start from the exact s: -max(logf(s), -100) or -max(logf(1 - s), -100) (image; (y - 1) * l1s -
y * ls is exactly one of the two for y in {0, 1}), -logf(s + NEAR_0) or -logf((1 - s) + NEAR_0)
(instance).  The truth takes the log of the float32 operand the kernel forms, so the bar of an
element is XL |e| (logf within 2 ulp), 0 where the clamp is in force; a loss is the double mean,
rounded once: mean bar + u |loss|.

Caps (asserted on the CPU for every case): a rounded-once bar never exceeds half an ulp of the
truth plus 2^-40 times its scale (the upstream gradient over the denominator for a gradient,
max(1, |term|) for a loss term); a bounded bar never exceeds fused_losses.CAP times its scale.

Ties: a rounded-once value is only determined when the truth is not within 2^-45 (relative) of
a float32 rounding tie; the focal clamp when p is not within 2^-45 of the midpoint below
1e-6f; the gate when e[0] is 16 u from 0.5.  tie_margin / clamp_margin / gate_margin measure
these and the case builders redraw until every element passes.

Everything a defect could plausibly touch goes through a module-level name (clamp_test,
P_FLOOR, NEAR_0, LOG_CLAMP, GRAD_FLOOR, gate_test, ins_denom, gate_column, scale_labels,
label_column, near0_bwd, cells_visited, sweep_rows, nll_count, on_map, other_logit, focal_q0,
kd_norm_rows, kd_norm_plus, kd_weight_index, kd_fwd_rows, kd_bwd_rows,
kd_temperature_in_gradient, PA_CLAMP, pa_switch, pa_ins_factor, pa_ins_zeros, pa_club_other,
dam_drop, dam_thr_images, modulate, sep_sign_b, sep_mean_over, SEP_EPS), so
tests/test_fused_da_losses_cpu.py can swap one for a defective version.

No torch and no tlod at import.
"""
import math

import numpy as np

import fused_losses as L
from fused_losses import SLACK, U, XL, CAP, loss_scalar, ls2_truth  # noqa: F401
from fused_optim import TINY, Watch  # noqa: F401

f32 = np.float32
E = 2.0 ** -53
RCAP = 2.0 ** -40
P_FLOOR = f32(1e-6)
NEAR_0 = f32(1e-10)
LOG_CLAMP = f32(-100.0)
GRAD_FLOOR = f32(1e-12)

_a, _d, _w = L._a, L._d, L._w


# ------------------------------------------------------------------ float32 spacing, ties
def half_ulp32(t):
    """Half the float32 spacing at |t| (float64), 2^-150 at and below the subnormals."""
    t = np.abs(_d(t))
    _, e = np.frexp(t)  # |t| in [2^(e-1), 2^e): the spacing there is 2^(e-24)
    return np.ldexp(0.5, np.where(t > 0, np.maximum(e - 24, -149), -149))


def tie_margin(t):
    """Distance of t from the nearest float32 rounding tie, relative to |t| (inf at 0)."""
    t = np.abs(_d(t))
    ulp = 2 * half_ulp32(t)
    frac = t / ulp - np.floor(t / ulp)  # exact: a division by a power of two
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(t > 0, np.abs(frac - 0.5) * ulp / np.where(t > 0, t, 1), np.inf)


def rounded(t, dbl_err):
    """Bar of a value evaluated in double (error <= dbl_err) and cast to float32."""
    return half_ulp32(t) + SLACK * dbl_err




# ------------------------------------------------------------------ IDF / EFocal domain losses
def clamp_test(p32, floor):
    return p32 < floor


def other_logit(label):
    return 1 - label


def focal_q0(q):
    """Rows whose 1.0 - p is 0 in double take an exactly zero gradient.  The kernel guards
    them for gamma < 1 only (q > 0.0 || gamma >= 1.0); for gamma >= 1 its formula gives 0 there
    by itself, so a kernel that zeroed them for every gamma would compute the same values and
    no case could, or need, tell the two apart."""
    return q == 0.0


def domain_losses(z_img, label_img, z_ins, label_ins, gamma, ef, gloss):
    """domain_loss_fwd / _bwd_kernel (ef: the _ef_ pair of selftrain.hip) in float64, in the
    kernel's own order, cast as the kernel casts: loss (n_img + 1), dz_img, dz_ins."""
    g = _d(_a(gloss))
    gamma = float(f32(gamma))
    zi, zn = _d(_a(z_img)).reshape(-1, 2), _d(_a(z_ins)).reshape(-1, 2)
    n, R = len(zi), len(zn)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        zl, zo = zi[:, label_img], zi[:, other_logit(label_img)]
        x = zo - zl
        ce = np.where(x > 0, x + np.log1p(np.exp(-x)), np.log1p(np.exp(x)))
        gg = g[:n] * (1.0 / (1.0 + np.exp(zo - zl)) - 1.0)
        dz_img = np.empty((n, 2), np.float32)
        dz_img[:, label_img], dz_img[:, other_logit(label_img)] = gg, -gg
        zl, zo = zn[:, label_ins], zn[:, other_logit(label_ins)]
        p = 1.0 / (1.0 + np.exp(zo - zl))
        if ef:
            terms = -np.exp(-gamma * p) * np.log(p)
            gi = g[n] / R * (np.exp(-gamma * p) * (gamma * np.log(p) - 1.0 / p)) * p * (1.0 - p)
        else:
            cl = clamp_test(p.astype(np.float32), P_FLOOR)
            P = np.where(cl, np.float64(P_FLOOR), p)
            terms = -(1.0 - P) ** gamma * np.log(P)
            q = 1.0 - p
            dLdP = gamma * q ** (gamma - 1.0) * np.log(p) - q ** gamma / p
            gi = np.where(cl | (focal_q0(q) & (gamma < 1.0)), 0.0, g[n] / R * dLdP * p * q)
        dz_ins = np.empty((R, 2), np.float32)
        dz_ins[:, label_ins], dz_ins[:, other_logit(label_ins)] = gi, -gi
        loss = np.concatenate([ce, [math.fsum(terms) / R if np.isfinite(terms).all()
                                    else np.nan]]).astype(np.float32)
    return {"loss": loss, "dz_img": dz_img, "dz_ins": dz_ins}


def _x(z, label):
    z = _d(_a(z)).reshape(-1, 2)
    return z[:, 1 - label] - z[:, label]  # exact in double for the magnitudes used


def _pq(x):
    """P, 1 - P and log P of a row whose other logit leads the label's by x."""
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(x)), 1.0 / (1.0 + np.exp(-x)), -np.logaddexp(0.0, x)


def clamp_midpoint():
    """(float)p < 1e-6f holds exactly when the double p lies below this."""
    return (float(f32(1e-6)) + float(np.nextafter(f32(1e-6), f32(0)))) / 2


def clamp_margin(z, label):
    p, _, _ = _pq(_x(z, label))
    return np.abs(p - clamp_midpoint()) / clamp_midpoint()


def domain_losses_truth(z_img, label_img, z_ins, label_ins, gamma, ef, gloss):
    """name -> (fp64 truth, bar, scale) for ce (n_img), dz_img, dz_ins; "focal": the float32
    the mean is expected to be; "terms"; "exact": the mask of dz_ins elements that are contract
    zeros, and their bytes."""
    g = _d(_a(gloss))
    gamma = float(f32(gamma))
    n, R = np.size(z_img) // 2, np.size(z_ins) // 2
    x = _x(z_img, label_img) if n else np.zeros(0)
    ce = np.logaddexp(0.0, x)
    with np.errstate(over="ignore"):
        t = g[:n] * (-1.0 / (1.0 + np.exp(-x)))  # g (p - 1)
    bar = rounded(t, np.abs(g[:n]) * 5 * E + 2 * E * np.abs(t))
    dz_img, b_img, s_img = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 2))
    dz_img[:, label_img], dz_img[:, 1 - label_img] = t, -t
    b_img[:], s_img[:] = bar[:, None], np.abs(g[:n])[:, None]

    p, q, lp = _pq(_x(z_ins, label_ins))
    gr = g[n] / R
    if ef:
        clamped = np.zeros(R, bool)
        terms = -np.exp(-gamma * p) * lp
        t = gr * np.exp(-gamma * p) * (gamma * p * lp - 1.0) * q
        rel = 5 * E / q + (16 + 4 * gamma) * E
    else:
        clamped = p.astype(np.float32) < f32(1e-6)
        c = float(f32(1e-6))
        terms = np.where(clamped, -(1 - c) ** gamma * math.log(c), -q ** gamma * lp)
        t = np.where(clamped, 0.0, gr * (gamma * q ** gamma * p * lp - q ** (gamma + 1)))
        rel = (gamma + 2) * 5 * E / q + 16 * E
    bar = np.where(clamped, 0.0, rounded(t, np.abs(t) * rel))
    dz_ins, b_ins = np.zeros((R, 2)), np.zeros((R, 2))
    dz_ins[:, label_ins], dz_ins[:, 1 - label_ins] = t, -t
    b_ins[:] = bar[:, None]
    exact = np.zeros((R, 2), bool)
    exact[clamped] = True
    zero = np.zeros((R, 2), np.float32)
    zero[:, 1 - label_ins] = -0.0
    return {"ce": (ce, rounded(ce, 8 * E * ce), np.maximum(1, ce)),
            "focal": loss_scalar(terms, R), "terms": terms,
            "dz_img": (dz_img, b_img, s_img),
            "dz_ins": (dz_ins, b_ins, np.full((R, 2), abs(gr))),
            "exact": {"dz_ins": (exact, zero)}}


# ------------------------------------------------------------------ US-DAF
def gate_test(e0):
    return e0 > f32(0.5)


def ins_denom(n):
    return f32(4) * f32(max(n, 1))


def gate_column(c):
    """The column whose gradient takes the gate as weight."""
    return c == 0


def label_column(c):
    """Column c of the instance head (1..3) -> index of its scale label."""
    return c - 1


def near0_bwd():
    return NEAR_0


SMALL, LARGE = f32(400), f32(10000)


def scale_labels(rois):
    r = _a(rois).reshape(-1, 5)
    area = _w((r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2]))
    return np.stack([area <= SMALL, (area > SMALL) & (area < LARGE), area >= LARGE],
                    1).astype(np.float32)


def sweep_rows(total):
    """The flat indices the backward's capped grid-stride loop reaches: all of them."""
    return np.arange(total)


def _ins_labels(rois, n, y, col=None):
    col = col or label_column
    lab = np.empty((n, 4), np.float32)
    lab[:, 0] = y
    sl = scale_labels(rois) if n else np.zeros((0, 3), np.float32)
    for c in (1, 2, 3):
        lab[:, c] = sl[:, col(c)]
    return lab


def us_daf(z_imgs, z_inss, roiss, gates_in, gloss, held=np.nan):
    """tlod_us_daf_loss_f32 / _bwd_f32 restated: the sigmoid in float64 in the kernel's form,
    cast; everything after it float32 in the kernel's order (numpy's float32 log for logf).
    z_imgs, z_inss, roiss: (source, target); gates_in: None or (gate_s, gate_t); gloss (4):
    [img_s, ins_s, img_t, ins_t].  held: what an element the sweep never reaches keeps."""
    g = _a(gloss)
    out, loss = {}, np.zeros(4, np.float32)
    for dom, tag in enumerate("st"):
        y = f32(1 - dom)
        zi, zn = _a(z_imgs[dom]).ravel(), _a(z_inss[dom]).reshape(-1, 4)
        npix, n = zi.size, zn.shape[0]
        with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
            p = (1.0 / (1.0 + np.exp(-_d(zi)))).astype(np.float32)
            s = (1.0 / (1.0 + np.exp(-_d(zn)))).astype(np.float32)
            ls = np.maximum(np.log(p), LOG_CLAMP)
            l1s = np.maximum(np.log(_w(f32(1) - p)), LOG_CLAMP)
            t = _w(_w((y - f32(1)) * l1s) - _w(y * ls))
            lab = _ins_labels(roiss[dom], n, y)
            a = _w(s + NEAR_0)
            b = _w(_w(f32(1) - s) + NEAR_0)
            e = -_w(_w(lab * np.log(a)) + _w(_w(f32(1) - lab) * np.log(b)))
            gate = gate_test(e[:, 0]).astype(np.float32) if gates_in is None \
                else _a(gates_in[dom]).ravel()
            rows = _d(_w(e[:, 0] * gate)) + _d(e[:, 1]) + _d(e[:, 2]) + _d(e[:, 3])
            loss[2 * dom] = loss_scalar(t, npix)
            loss[2 * dom + 1] = f32(np.float64(math.fsum(rows)) / np.float64(ins_denom(n)))
            # ---- the backward
            gi = _w(g[2 * dom] / f32(npix))
            gn = _w(g[2 * dom + 1] / ins_denom(n))
            qq = _w(p * _w(f32(1) - p))
            dzi = _w(_w(gi * _w(p - y)) * _w(qq / np.maximum(qq, GRAD_FLOOR)))
            ab, bb = _w(s + near0_bwd()), _w(_w(f32(1) - s) + near0_bwd())
            de = -_w(_w(lab / ab) - _w(_w(f32(1) - lab) / bb))
            w32 = np.where(gate_column(np.arange(4))[None, :], gate[:, None],
                           f32(1)).astype(np.float32)
            dzn = _w(_w(_w(gn * w32) * de) * _w(s * _w(f32(1) - s)))
        # the kernel's one index space: pixels, then instance elements
        seen = np.zeros(npix + 4 * n, bool)
        seen[sweep_rows(npix + 4 * n)] = True
        flat = np.where(seen, np.concatenate([dzi, dzn.ravel()]), f32(held)).astype(np.float32)
        out.update({"s_img_" + tag: p, "s_ins_" + tag: s, "gate_" + tag: gate,
                    "dz_img_" + tag: flat[:npix], "dz_ins_" + tag: flat[npix:].reshape(n, 4)})
    out["loss"] = loss
    return out


def sigmoid_truth(z):
    z = _d(z)
    with np.errstate(over="ignore"):
        ez = np.exp(-np.abs(z))
    s = np.where(z >= 0, 1 / (1 + ez), ez / (1 + ez))
    return s, rounded(s, 6 * E * s)


def us_daf_truth(z_imgs, z_inss, roiss, gates_in, gloss):
    """name -> (fp64 truth, bar, scale) for s_img_*, s_ins_* (rounded once) and loss (bounded);
    e0_*: the truth of the gate's element loss; gate_*: the gate it implies."""
    out = {}
    loss, bloss, sloss = np.zeros(4), np.zeros(4), np.ones(4)
    for dom, tag in enumerate("st"):
        y = f32(1 - dom)
        zi, zn = _a(z_imgs[dom]).ravel(), _a(z_inss[dom]).reshape(-1, 4)
        npix, n = zi.size, zn.shape[0]
        si, bsi = sigmoid_truth(zi)
        sn, bsn = sigmoid_truth(zn)
        out["s_img_" + tag], out["s_ins_" + tag] = (si, bsi, 1.0), (sn, bsn, 1.0)
        p, s = si.astype(np.float32), sn.astype(np.float32)
        op = _d(p if y == 1 else f32(1) - p)  # the float32 operand of the live logf
        with np.errstate(divide="ignore"):
            t = -np.maximum(np.log(op), -100.0)
        bt = np.where(t == 100.0, 0.0, SLACK * XL * np.abs(t))
        loss[2 * dom] = math.fsum(t) / npix
        sloss[2 * dom] = L._mean_scale(t, npix)
        bloss[2 * dom] = L._mean_bar(loss[2 * dom], bt, npix, sloss[2 * dom])
        lab = _ins_labels(roiss[dom], n, y, lambda c: c - 1)
        live = np.where(lab == 1, s + f32(1e-10), (f32(1) - s) + f32(1e-10))
        e = -np.log(_d(live))
        be = SLACK * XL * np.abs(e)
        out["e0_" + tag] = e[:, 0]
        gate = (e[:, 0] > 0.5).astype(np.float64) if gates_in is None \
            else _d(_a(gates_in[dom])).ravel()
        out["gate_" + tag] = gate
        wgt = np.ones((n, 4))
        wgt[:, 0] = gate
        den = 4.0 * max(n, 1)
        if n:
            loss[2 * dom + 1] = math.fsum((e * wgt).ravel()) / den
            sloss[2 * dom + 1] = float((np.maximum(1, np.abs(e)) * np.abs(wgt)).sum()) / den
            sloss[2 * dom + 1] = max(sloss[2 * dom + 1], TINY)
            bloss[2 * dom + 1] = L._mean_bar(loss[2 * dom + 1], be * np.abs(wgt), den,
                                             sloss[2 * dom + 1])
    out["loss"] = (loss, bloss, sloss)
    return out


def gate_margin(e0):
    """|e[0] - 0.5| in u."""
    return np.abs(_d(e0) - 0.5) / U


# ------------------------------------------------------------------ masked 2-way NLL
def cells_visited(HW):
    """The cells the backward's capped grid (64 blocks of 256) writes: all of them."""
    return np.arange(HW)


def nll_count(cells):
    return cells


def on_map(m):
    return m == f32(1)


def masked_nll2(scores, maps, need, gout, held=np.nan):
    """masked_nll2_fwd / _bwd_kernel in float32 (numpy's exp / log): loss, count (K, B),
    g = gout / count, dscore (K, B, 2, HW).  held: what a cell the sweep never reaches keeps."""
    K, B = len(scores), len(need)
    gout = _a(gout).reshape(K, B)
    HW = _a(maps[0])[0].size
    loss, count, g = (np.zeros((K, B), np.float32) for _ in range(3))
    ds = np.zeros((K, B, 2, HW), np.float32)
    seen = np.zeros(HW, bool)
    seen[cells_visited(HW)] = True
    for k in range(K):
        sc, mp = _a(scores[k]).reshape(B, 2, HW), _a(maps[k]).reshape(B, HW)
        for b in range(B):
            on = on_map(mp[b])
            one = int(need[b]) == 1
            l0, l1 = L.log_softmax2(sc[b, 0, on], sc[b, 1, on])
            n = f32(nll_count(int(on.sum())))
            count[k, b] = n
            if n > 0:
                loss[k, b] = loss_scalar(-(l1 if one else l0), n)
                g[k, b] = _w(gout[k, b] / n)
                ds[k, b, 0, on] = _w(g[k, b] * _w(_w(np.exp(l0)) - f32(0 if one else 1)))
                ds[k, b, 1, on] = _w(g[k, b] * _w(_w(np.exp(l1)) - f32(1 if one else 0)))
    ds[..., ~seen] = held
    return {"loss": loss, "count": count, "g": g, "dscore": ds}


def masked_nll2_truth(scores, maps, need, gout):
    """loss and dscore as (fp64 truth, bar, scale); "zeros": the cells of dscore that are
    exactly +0.0 (off the map, or an empty map)."""
    K, B = len(scores), len(need)
    gout = _a(gout).reshape(K, B)
    HW = _a(maps[0])[0].size
    loss, bl, sl = np.zeros((K, B)), np.zeros((K, B)), np.ones((K, B))
    ds, bds, sds = (np.zeros((K, B, 2, HW)) for _ in range(3))
    zeros = np.ones((K, B, 2, HW), bool)
    for k in range(K):
        sc, mp = _d(_a(scores[k])).reshape(B, 2, HW), _a(maps[k]).reshape(B, HW)
        for b in range(B):
            on = mp[b] == 1
            one = int(need[b]) == 1
            if not on.any():
                continue
            n = float(on.sum())
            gd = float(f32(gout[k, b]) / f32(n))
            ls, bls, p, bp = ls2_truth(sc[b, 0, on], sc[b, 1, on])
            terms = -(ls[1] if one else ls[0])
            tb = np.minimum(bls[1] if one else bls[0], CAP * np.maximum(1, np.abs(terms)))
            loss[k, b] = terms.sum() / n
            sl[k, b] = L._mean_scale(terms, n)
            bl[k, b] = L._mean_bar(loss[k, b], tb, n, sl[k, b])
            for ch in (0, 1):
                yk = 1.0 if (ch == 1) == one else 0.0
                ds[k, b, ch, on] = gd * (p[ch] - yk)
                bds[k, b, ch, on] = abs(gd) * np.minimum(
                    SLACK * (bp[ch] + 3 * U * np.abs(p[ch] - yk)), CAP)
                zeros[k, b, ch, on] = False
            sds[k, b] = abs(gd)
    return {"loss": (loss, bl, sl), "dscore": (ds, bds, sds), "zeros": zeros}


# ------------------------------------------------------------------ KD KL
def kd_norm_rows(R, wmod):
    """The rows whose weight the normaliser sum w + 1 counts: each weight once."""
    return np.arange(min(R, wmod))


def kd_norm_plus():
    return 1.0


def kd_weight_index(r, wmod):
    return r % wmod


def kd_fwd_rows(R):
    """The rows the forward's 1024-thread stride reaches: all of them."""
    return np.arange(R)


def kd_bwd_rows(R):
    """The rows the backward's capped grid (1024 blocks of 256) reaches: all of them."""
    return np.arange(R)


def kd_temperature_in_gradient(T):
    return T


def _kd_gather(x, R, C, rs, cs):
    idx = np.arange(R)[:, None] * rs + np.arange(C)[None, :] * cs
    return _d(_a(x).ravel()[idx]), idx


def kd_kl(student, teacher, weight, R, C, rs, cs, wmod, T, gout, held=np.nan):
    """kd_kl_fwd / _bwd_kernel in float64 in the kernel's own order (kl_row), cast as the
    kernel casts: out (2) = [loss, sum w + 1], dstudent (flat, the layout of student)."""
    S, idx = _kd_gather(student, R, C, rs, cs)
    Tt, _ = _kd_gather(teacher, R, C, rs, cs)
    Td = float(f32(T))
    w = _d(_a(weight).ravel()[kd_weight_index(np.arange(R), wmod)])
    z1, z2 = S / Td, Tt / Td
    m1, m2 = z1.max(1), z2.max(1)
    Z1, Z2 = np.zeros(R), np.zeros(R)
    for c in range(C):
        Z1 = Z1 + np.exp(z1[:, c] - m1)
        Z2 = Z2 + np.exp(z2[:, c] - m2)
    l1 = (z1 - m1[:, None]) - np.log(Z1)[:, None]
    l2 = (z2 - m2[:, None]) - np.log(Z2)[:, None]
    kl = np.zeros(R)
    for c in range(C):
        kl = kl + np.exp(l1[:, c]) * (l1[:, c] - l2[:, c])
    fr = kd_fwd_rows(R)
    nr = np.intersect1d(kd_norm_rows(R, wmod), fr)
    v1 = math.fsum(w[nr]) + kd_norm_plus()
    v0 = math.fsum((w * kl)[fr][w[fr] != 0])
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.array([np.float64(v0) / np.float64(v1), v1]).astype(np.float32)
        g = np.float64(f32(gout)) / np.float64(out[1]) / kd_temperature_in_gradient(Td)
        d = (g * w)[:, None] * (np.exp(l1) * ((l1 - l2) - kl[:, None]))
    d = np.where((w == 0)[:, None], 0.0, d).astype(np.float32)
    seen = np.zeros(R, bool)
    seen[kd_bwd_rows(R)] = True
    d[~seen] = held
    flat = np.zeros(_a(student).size, np.float32)
    flat[idx.ravel()] = d.ravel()
    return {"out": out, "dstudent": flat}


def _em1mx(u):
    """exp(u) - 1 - u without the cancellation at small u."""
    small = np.abs(u) < 0.1
    us = np.where(small, u, 0.0)
    ser = np.zeros_like(us)
    for k in range(16, 2, -1):
        ser = (1 + ser) * us / k
    ser = (1 + ser) * us * us / 2
    with np.errstate(over="ignore"):
        return np.where(small, ser, np.expm1(u) - u)


def _softmax(z):
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def kd_kl_truth(student, teacher, weight, R, C, rs, cs, wmod, T, gout):
    """out (2) and dstudent as (fp64 truth, bar, scale); "zeros": the elements of dstudent
    that are exactly +0.0 (rows of weight 0); "kl": the row terms.

    With delta = (s - t) / T up to a constant per row (s - t is exact in double) and u = log
    p2 - log p1 =
    log sum p2 e^delta - delta:  KL = sum p1 (e^u - 1 - u)  (sum p1 (e^u - 1) = 0: every term
    is >= 0, nothing cancels between classes), and the gradient factor (log p1_j - log p2_j) -
    KL = delta_j - sum p1 delta: the two log-sum-exps drop out."""
    S, idx = _kd_gather(student, R, C, rs, cs)
    Tt, _ = _kd_gather(teacher, R, C, rs, cs)
    # np.longdouble throughout (64 bits on x86): a float64 softmax of logits 100 apart carries
    # 100 E from its exponents alone; the results are rounded to float64 at the end
    ld = np.longdouble
    S, Tt, Td = S.astype(ld), Tt.astype(ld), ld(f32(T))
    w = _a(weight).ravel()[np.arange(R) % wmod].astype(ld)
    z1, z2 = S / Td, Tt / Td
    p1, p2 = _softmax(z1), _softmax(z2)
    # both softmaxes ignore a shift common to the classes: take delta from the teacher's best
    # class, so that a student that is its teacher plus a constant gives delta = 0 exactly
    diff = S - Tt
    k = np.argmax(z2, 1)[:, None]
    delta = (diff - np.take_along_axis(diff, k, 1)) / Td
    m1, m2 = z1.max(1, keepdims=True), z2.max(1, keepdims=True)
    lz1 = np.log(np.exp(z1 - m1).sum(1, keepdims=True))
    lz2 = np.log(np.exp(z2 - m2).sum(1, keepdims=True))
    l1, l2 = (z1 - m1) - lz1, (z2 - m2) - lz2
    near = np.abs(delta).max(1, keepdims=True) <= 1.0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        Dn = np.log1p((p2 * np.expm1(np.where(near, delta, 0.0))).sum(1, keepdims=True))
    u = np.where(near, Dn - delta, l2 - l1)
    kl = (p1 * _em1mx(u)).sum(1)
    N = w[:min(R, wmod)].sum() + ld(1)
    loss = (w * kl).sum() / N
    # ---- the kernel's double error, in kl_row's order
    dT = 0.0 if Td == 1.0 else 1.0

    def eps_l(z, m, lz, l, p):
        # z / T is formed the same way for the max and in the loops: at the row's best class
        # z - m is exactly 0 and exp(0) exactly 1; elsewhere both quotients carry their E
        top = z == m
        a = np.where(top, 0.0, E * dT * (np.abs(z) + np.abs(m)) + E * np.abs(z - m))
        zeta = (p * (np.where(top, 0.0, 2 * E) + a)).sum(1, keepdims=True) + C * E
        return a + zeta + 2 * E * np.abs(lz) + E * np.abs(l)
    e1, e2 = eps_l(z1, m1, lz1, l1, p1), eps_l(z2, m2, lz2, l2, p2)
    au = np.abs(u)
    e_kl = (p1 * ((e1 + 3 * E) * au + e1 + e2) + (C + 1) * E * p1 * au).sum(1)
    tree = (R / 1024 + 22) * E
    e_loss = ((w * e_kl).sum() + tree * (w * kl).sum()) / N + 3 * E * abs(loss)
    s_loss = float((w * np.maximum(1, kl)).sum() / N)
    out = np.array([loss, N], np.float64)
    bout = np.array([rounded(loss, e_loss), rounded(N, (wmod / 1024 + 22) * E * N)], np.float64)
    g = ld(f32(gout)) / ld(f32(N)) / Td  # the kernel divides by the float32 it saved
    # delta_j - sum_c p1_c delta_c = sum_{c != j} p1_c (delta_j - delta_c): where p1_j is near 1
    # the sum holds only the small p1_c, so the truth does not cancel as the kernel does
    fac = np.stack([(p1 * (diff[:, j:j + 1] - diff)).sum(1) for j in range(C)], 1) / Td
    d = (g * w)[:, None] * p1 * fac
    e_d = np.abs(g * w)[:, None] * p1 * ((e1 + 2 * E) * np.abs(fac) + e1 + e2 + E * au
                                         + e_kl[:, None] + E * np.abs(fac)) + 6 * E * np.abs(d)
    zeros = np.broadcast_to((w == 0)[:, None], d.shape)
    bar = np.where(zeros, 0.0, rounded(d, e_d))
    n = _a(student).size
    flat, fbar, fscale, fz = np.zeros(n), np.zeros(n), np.zeros(n), np.ones(n, bool)
    flat[idx.ravel()], fbar[idx.ravel()] = d.ravel(), bar.ravel()
    fscale[idx.ravel()] = np.broadcast_to(np.abs(g * w)[:, None], d.shape).ravel()
    fz[idx.ravel()] = zeros.ravel()
    return {"out": (out, bout, np.array([max(s_loss, 0.0), float(N)])),
            "dstudent": (flat, fbar, fscale), "zeros": fz, "kl": _d(kl)}


# ------------------------------------------------------------------ PA-ATF: the 14 terms
PA_IMG, PA_INS, PA_TERMS = 6, 2, 14
PA_CLAMP = 100.0


def pa_switch(sp):
    """The backward's test for a live image logit."""
    return sp < 100.0


def pa_ins_factor(n, label):
    return n - 2 * label


def pa_ins_zeros(n, label):
    return n - label


def pa_club_other(label):
    return 1 - label


def _softplus(x):
    with np.errstate(over="ignore"):
        return np.where(x > 0, x + np.log1p(np.exp(-np.abs(x))), np.log1p(np.exp(-np.abs(x))))


def pa_atf(z, n, label, gloss):
    """loss_fwd / loss_bwd_kernel of csrc/pa_atf.hip in float64 in the kernel's order, cast as
    the kernel casts: loss (14), dz (a list of 14 float32 arrays shaped as z)."""
    gl = _d(_a(gloss))
    loss, dz = np.zeros(PA_TERMS, np.float32), []
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        for t in range(PA_TERMS):
            x, nt, lab = _d(_a(z[t])), int(n[t]), int(label[t])
            g = gl[t] / nt
            if t < PA_IMG:
                x = x.ravel()
                u = -x if lab else x
                sp = _softplus(u)
                terms = np.minimum(sp, PA_CLAMP)
                d = np.where(pa_switch(sp), 1.0 / (1.0 + np.exp(-u)), 0.0)
                dz.append((g * (-d if lab else d)).astype(np.float32))
            elif t < PA_IMG + PA_INS:
                s = 1.0 / (1.0 + np.exp(-x.ravel()))
                terms = (float(lab) * (1.0 - s) + float(pa_ins_zeros(nt, lab)) * s) / nt
                dz.append((g * float(pa_ins_factor(nt, lab)) / nt * s * (1.0 - s))
                          .astype(np.float32))
            else:
                x = x.reshape(-1, 2)
                zl, zo = x[:, lab], x[:, pa_club_other(lab)]
                terms = _softplus(zo - zl)
                d = g * (1.0 / (1.0 + np.exp(zo - zl)) - 1.0)
                o = np.empty((nt, 2), np.float32)
                o[:, lab], o[:, pa_club_other(lab)] = d, -d
                dz.append(o)
            loss[t] = f32(math.fsum(terms) / nt) if np.isfinite(terms).all() else f32(np.nan)
    return {"loss": loss, "dz": dz}


def pa_atf_truth(z, n, label, gloss):
    """"loss": the 14 float32 scalars the double means are expected to be (1 ulp allowed);
    "dz": per term (fp64 truth, bar, scale); "exact": per term (mask, bytes) of the contract
    zeros: image logits past the clamp, and an instance term whose n - 2 label is 0."""
    gl = _d(_a(gloss))
    loss, dz, exact = np.zeros(PA_TERMS, np.float32), [], []
    for t in range(PA_TERMS):
        x, nt, lab = _d(_a(z[t])), int(n[t]), int(label[t])
        g = gl[t] / nt
        if t < PA_IMG:
            x = x.ravel()
            u = -x if lab else x
            sp = np.logaddexp(0.0, u)
            terms = np.minimum(sp, 100.0)
            live = sp < 100.0
            with np.errstate(over="ignore"):
                eu = np.exp(-np.abs(u))
            sig = np.where(u >= 0, 1 / (1 + eu), eu / (1 + eu))
            sgn = -1.0 if lab else 1.0
            v = np.where(live, g * sgn * sig, 0.0)
            bar = np.where(live, rounded(v, 6 * E * np.abs(v)), 0.0)
            zero = np.full(x.shape, f32(g * (sgn * 0.0)), np.float32)
            ex = (~live, zero)
        elif t < PA_IMG + PA_INS:
            x = x.ravel()
            with np.errstate(over="ignore"):
                ex_ = np.exp(-np.abs(x))
            s, c = np.where(x >= 0, 1 / (1 + ex_), ex_ / (1 + ex_)), \
                np.where(x >= 0, ex_ / (1 + ex_), 1 / (1 + ex_))  # sigmoid(z), 1 - sigmoid(z)
            terms = (lab * c + (nt - lab) * s) / nt
            k = g * (nt - 2 * lab) / nt
            v = k * s * c
            bar = rounded(v, 12 * E * np.abs(v) + 5 * E * abs(k) * s * s)  # |v| s / c = |k| s^2
            dead = np.full(x.shape, nt == 2 * lab)
            bar = np.where(dead, 0.0, bar)
            ex = (dead, np.full(x.shape, f32(g * 0.0), np.float32))
        else:
            x = x.reshape(-1, 2)
            xx = x[:, 1 - lab] - x[:, lab]
            terms = np.logaddexp(0.0, xx)
            with np.errstate(over="ignore"):
                d = g * (-1.0 / (1.0 + np.exp(-xx)))
            b1 = rounded(d, abs(g) * 5 * E + 2 * E * np.abs(d))
            v, bar = np.zeros((nt, 2)), np.zeros((nt, 2))
            v[:, lab], v[:, 1 - lab] = d, -d
            bar[:] = b1[:, None]
            ex = (np.zeros((nt, 2), bool), np.zeros((nt, 2), np.float32))
        loss[t] = loss_scalar(terms, nt)
        dz.append((v, bar, np.full(np.shape(v), abs(g))))
        exact.append(ex)
    return {"loss": loss, "dz": dz, "exact": exact}


# ------------------------------------------------------------------ IDF: DAM and separation
SEP_EPS = 1e-6  # a double in the kernel
SEP_WAVES = 16


def dam_drop(avg, thr):
    return avg < thr


def dam_thr_images(N):
    """The images whose avg enter image n's threshold: its own."""
    return [[n] for n in range(N)]


def modulate(a, att_other):
    """a (N, C, P) times one plus the other stack's attention (N, P), in float32."""
    return _w(a * _w(f32(1) + att_other)[:, None, :])


def sep_sign_b():
    return -1.0


def sep_mean_over(P):
    return float(P)


def _slices(v):
    """Sum of v (N, C, P) over the channels in the workgroup's order: slice w adds c = w, w +
    16, ... in turn, then the 16 slices in order."""
    tot = np.zeros((v.shape[0], v.shape[2]))
    for w in range(SEP_WAVES):
        s = np.zeros_like(tot)
        for c in range(w, v.shape[1], SEP_WAVES):
            s = s + v[:, c]
        tot = tot + s
    return tot


def dam(x):
    """dam_avg / dam_threshold_kernel: x (N, C, P) -> att (N, P) float32."""
    x = _d(_a(x))
    N, C, P = x.shape
    with np.errstate(over="ignore"):
        avg = (_slices(1.0 / (1.0 + np.exp(-x))) / C).astype(np.float32)
    att = np.empty_like(avg)
    for n, imgs in enumerate(dam_thr_images(N)):
        pool = _d(avg[imgs]).ravel()
        thr = f32(math.fsum(pool) / pool.size)
        att[n] = np.where(dam_drop(avg[n], thr), f32(0), avg[n])
    return att


def dam_truth(x):
    """avg (N, P) and thr (N) as (truth, bar, scale), np.longdouble inside; thr is the mean of
    the float32 avg, as the kernel takes it."""
    ld = np.longdouble
    x = _a(x).astype(ld)
    N, C, P = x.shape
    e = np.exp(-np.abs(x))
    s = np.where(x >= 0, 1 / (1 + e), e / (1 + e))
    avg = _d(s.sum(1) / C)
    bavg = rounded(avg, (C / 16 + 24) * E * avg)
    thr = _d(avg.astype(np.float32).astype(ld).sum(1) / P)
    return {"avg": (avg, bavg, 1.0), "thr": (thr, rounded(thr, (P / 64 + 12) * E * thr), 1.0)}


def separation(a, b, att_a, att_b, g_a_out, g_b_out, g_dist):
    """sep_fwd / sep_mean / sep_bwd_kernel in float64 in the kernel's order, cast as the kernel
    casts.  a, b (N, C, P); att_b None: weight 1, no modulation; g_a_out / g_b_out None: the
    backward without the modulation terms; g_dist None: forward only."""
    a32, b32 = _a(a), _a(b)
    N, C, P = a32.shape
    w = np.ones((N, P)) if att_b is None else _d(_a(att_b))
    e = (_d(a32) - _d(b32)) * w[:, None, :] + SEP_EPS
    dd = np.sqrt(_slices(e * e))
    out = {"d": dd.astype(np.float32),
           "dist": np.array([math.fsum(r) / sep_mean_over(P) for r in dd]).astype(np.float32)}
    if att_b is not None:
        out["a_out"], out["b_out"] = modulate(a32, _a(att_b)), modulate(b32, _a(att_a))
    if g_dist is None:
        return out
    d32 = _d(out["d"])
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(d32 > 0, _d(_a(g_dist))[:, None] / sep_mean_over(P) * w / d32, 0.0)
    t = k[:, None, :] * e
    if g_a_out is None:
        out["g_a"], out["g_b"] = t.astype(np.float32), (sep_sign_b() * t).astype(np.float32)
    else:
        ma, mb = 1.0 + _d(_a(att_b)), 1.0 + _d(_a(att_a))
        out["g_a"] = (_d(_a(g_a_out)) * ma[:, None, :] + t).astype(np.float32)
        out["g_b"] = (_d(_a(g_b_out)) * mb[:, None, :] + sep_sign_b() * t).astype(np.float32)
    return out


def separation_truth(a, b, att_a, att_b, g_a_out, g_b_out, g_dist):
    """d, dist, g_a, g_b as (truth, bar, scale), np.longdouble inside.  The backward divides by
    the float32 d the forward saved, and so does its truth.  "zeros": the elements of g_a / g_b
    that are exactly +0.0 (a zero weight under a zero upstream gradient)."""
    ld = np.longdouble
    al, bl = _a(a).astype(ld), _a(b).astype(ld)
    N, C, P = al.shape
    w = np.ones((N, P), ld) if att_b is None else _a(att_b).astype(ld)
    dw = (al - bl) * w[:, None, :]
    e = dw + ld(SEP_EPS)
    ss = (e * e).sum(1)
    d = np.sqrt(ss)
    # e = fl(fl(delta w) + eps): E (|delta w| + |e|) absolute; ss adds C squares
    e_ss = (2 * np.abs(e) * E * (np.abs(dw) + np.abs(e))).sum(1) + (C / 16 + 20) * E * ss
    with np.errstate(divide="ignore", invalid="ignore"):
        e_d = _d(np.where(d > 0, e_ss / (2 * d), 0) + E * d)
    dist = d.sum(1) / P
    e_dist = e_d.mean(1) + (P / 64 + 12) * E * _d(dist)
    out = {"d": (_d(d), rounded(_d(d), e_d), np.maximum(_d(d), 1.0)),
           "dist": (_d(dist), rounded(_d(dist), e_dist), np.maximum(_d(dist), 1.0))}
    if g_dist is None:
        return out
    d32 = _d(d).astype(np.float32).astype(ld)
    gd = _a(g_dist).astype(ld)[:, None] / P
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(d32 > 0, gd * w / d32, 0)
    t = k[:, None, :] * e
    e_t = _d(np.abs(k))[:, None, :] * E * _d(np.abs(dw) + np.abs(e)) + 5 * E * _d(np.abs(t))
    zeros = np.zeros((N, C, P), bool)
    if g_a_out is None:
        A = B = np.zeros((N, C, P), ld)
    else:
        A = _a(g_a_out).astype(ld) * (1 + _a(att_b).astype(ld))[:, None, :]
        B = _a(g_b_out).astype(ld) * (1 + _a(att_a).astype(ld))[:, None, :]
        zeros = np.broadcast_to((w == 0)[:, None, :], zeros.shape) \
            & (_a(g_a_out) == 0) & (_a(g_b_out) == 0)
    scale = np.broadcast_to(_d(np.abs(gd))[:, :, None], (N, C, P)) + 2 * _d(
        np.maximum(np.abs(A), np.abs(B)))
    for name, base, sgn in (("g_a", A, 1), ("g_b", B, -1)):
        v = _d(base + sgn * t)
        err = e_t + 3 * E * (_d(np.abs(base)) + _d(np.abs(t)))
        out[name] = (v, np.where(zeros, 0.0, rounded(v, err)), np.maximum(scale, TINY))
    out["zeros"] = zeros
    return out
