"""The fused clip + SGD / Adam step of csrc/optim.hip, restated in numpy float32 operation by
operation, and the fp64 truth the fused optimizers are measured against.

The step is fixed-order float32 arithmetic compiled without contraction, so every function
here is required to equal the device bit for bit (tests/test_fused_optim_gpu.py):

  chunk_sumsq   one workgroup of sgd_sumsq_kernel / adam_sumsq_kernel: four lane-strided
                accumulators per thread on the 16-byte path (one on the scalar path), the
                64-lane shuffle tree, the four-wave sum;
  grad_norm     sgd_norm_kernel: doubles strided by 256, the 128..1 tree, sqrt in double,
                total rounded to float32, scale = clip / fmaxf(total, clip) (1 when clip <= 0);
  grad_term     d = (g * gs) * scale + wd * p, the gradient both updates start from;
  sgd1, adam1   one element of the update, in the kernel's association;
  adam_consts   AdamK: the betas and eps rounded to float32, 1 - beta rounded once from double;
  adam_corr     {1 / (1 - b1^t), 1 / sqrt(1 - b2^t)} in double, rounded to float32 (the device
                computes these with its own double pow: the one value not pinned exactly);
  step          a whole call over a descriptor table.

Every operand is np.float32 (lr and weight_decay are rounded first, as the descriptor dtypes
of tlod/optim.py store them); a float32 numpy operation rounds once, to nearest even, as the
device's does.  Sums are spelled out: np.sum's pairwise order is not the kernel's.

Everything a defect could plausibly touch goes through a module-level name (chunk_sumsq,
grad_norm, clip_scale, grad_term, sgd1, adam1, adam_consts, row_counts, is_live, advances,
shared_counts), so tests/test_fused_optim_cpu.py can swap one for a defective version.

No torch and no tlod at import: Truth and check_bar take torch tensors but only call their
methods.
"""
import math
from collections import namedtuple

import numpy as np

f32 = np.float32
B1, B2, EPS = 0.9, 0.999, 1e-8
TINY = float(np.finfo(np.float32).tiny)  # 2^-126, the smallest normal float32


# ------------------------------------------------------------------ watching intermediates
class Watch:
    """Records the smallest nonzero and the largest magnitude of every float32 intermediate
    the restatement forms while it is installed (`with Watch() as w:`)."""

    def __init__(self):
        self.lo, self.hi, self.bad = math.inf, 0.0, 0

    def note(self, x):
        a = np.abs(np.asarray(x, dtype=np.float64)).ravel()
        self.bad += int(np.count_nonzero(~np.isfinite(a)))
        a = a[np.isfinite(a)]
        if a.size:
            self.hi = max(self.hi, float(a.max()))
        a = a[a > 0]
        if a.size:
            self.lo = min(self.lo, float(a.min()))

    def __enter__(self):
        global _watch
        self._prev, _watch = _watch, self
        return self

    def __exit__(self, *exc):
        global _watch
        _watch = self._prev


_watch = None


def _w(x):
    if _watch is not None:
        _watch.note(x)
    return x


def _vec(x):
    return np.ascontiguousarray(x, dtype=np.float32).ravel()


# ------------------------------------------------------------------ the norm
def chunk_sumsq(grad, gs, vec):
    """*partial of one workgroup over grad (the |count| elements of one table row).  vec: what
    vec4_ok decides for the row, a 16-byte aligned gradient pointer and count % 4 == 0."""
    g, gs = _vec(grad), f32(gs)
    width = 4 if vec else 1
    assert g.size % width == 0
    n = g.size // width
    rounds = -(-n // 256)
    # thread t, round r reads element r * 256 + t; a slot past the end adds +0 to a
    # non-negative accumulator, which changes nothing
    x = np.zeros((rounds * 256, width), dtype=np.float32)
    x[:n] = g.reshape(n, width)
    x = x.reshape(rounds, 256, width)
    s = np.zeros((256, 4), dtype=np.float32)
    for r in range(rounds):
        t = _w(x[r] * gs)
        s[:, :width] = _w(s[:, :width] + _w(t * t))
    s = _w(_w(s[:, 0] + s[:, 1]) + _w(s[:, 2] + s[:, 3]))
    a = s.reshape(4, 64).copy()  # lane 0 of each wave after the __shfl_down tree
    o = 32
    while o:
        a[:, :o] = _w(a[:, :o] + a[:, o:2 * o])
        o >>= 1
    ws = a[:, 0]
    return _w(_w(ws[0] + ws[1]) + _w(ws[2] + ws[3]))


def clip_scale(total, clip):
    total, clip = f32(total), f32(clip)
    return clip / max(total, clip) if clip > 0 else f32(1)


def grad_norm(partials, clip):
    """(total, scale) of the norm launch over the float32 partials."""
    p = np.asarray(partials, dtype=np.float32).astype(np.float64)
    rounds = -(-p.size // 256)
    x = np.zeros(rounds * 256, dtype=np.float64)
    x[:p.size] = p
    x = x.reshape(rounds, 256)
    ws = np.zeros(256, dtype=np.float64)
    for r in range(rounds):
        ws = ws + x[r]
    o = 128
    while o:
        ws[:o] = ws[:o] + ws[o:2 * o]
        o >>= 1
    total = _w(f32(np.sqrt(ws[0])))
    return total, _w(clip_scale(total, clip))


# ------------------------------------------------------------------ one element of the update
def grad_term(g, p, gs, scale, wd):
    return _w(_w(_w(g * f32(gs)) * f32(scale)) + _w(f32(wd) * p))


def sgd1(g, p, b, gs, scale, wd, lr, momentum):
    """(p, b) after sgd1 of csrc/optim.hip."""
    d = grad_term(g, p, gs, scale, wd)
    b = _w(_w(f32(momentum) * b) + d)
    return _w(p - _w(f32(lr) * b)), b


AdamK = namedtuple("AdamK", "b1 omb1 b2 omb2 eps")


def adam_consts(b1=B1, b2=B2, eps=EPS):
    return AdamK(f32(b1), f32(1.0 - b1), f32(b2), f32(1.0 - b2), f32(eps))


def adam1(g, p, m, v, gs, scale, wd, step, c2, k):
    """(p, m, v) after adam1 of csrc/optim.hip: omb2 * d * d is (omb2 * d) * d, the
    denominator (sqrtf(v) * c2) + eps, the quotient m / denominator taken before step."""
    d = grad_term(g, p, gs, scale, wd)
    m = _w(_w(k.b1 * m) + _w(k.omb1 * d))
    v = _w(_w(k.b2 * v) + _w(_w(k.omb2 * d) * d))
    den = _w(_w(np.sqrt(v) * f32(c2)) + k.eps)
    return _w(p - _w(f32(step) * _w(m / den))), m, v


def adam_corr(t, b1=B1, b2=B2):
    return f32(1.0 / (1.0 - b1 ** t)), f32(1.0 / math.sqrt(1.0 - b2 ** t))


# ------------------------------------------------------------------ a call over a table
# pid: the parameter the row belongs to (Adam's step count and corr pair are per parameter);
# param, grad and every state array hold the row's |count| elements; count < 0 marks a
# norm-only row; active: None (a null pointer) or the float the pointer reads; vec: the
# 16-byte decision of the row's sum of squares.
Row = namedtuple("Row", "pid param grad state count lr wd active vec")
Result = namedtuple("Result", "partials total scale rows counts corr")


def row_counts(count):
    """(elements the norm reads, elements the chunk update writes) of a row."""
    return abs(count), max(count, 0)


def is_live(active):
    return active is None or f32(active) != 0


def advances(active):
    """Whether the norm launch advances the step count of a parameter (Adam)."""
    return is_live(active)


def shared_counts(counts):
    return counts


def step(kind, rows, gs, clip, momentum=0.9, betas=(B1, B2), eps=EPS, counts=None, corr=None,
         corr_given=None):
    """One tlod_sgd_clip_f32 (kind "sgd") or tlod_adam_clip_f32 ("adam") call.  Returns
    Result: the partials, total and scale, per row the new (param, state...) arrays (the old
    ones where the row is norm-only or its parameter not live), and for Adam the parameters'
    new step counts {pid: t} and corr pairs {pid: (c0, c1)} (counts / corr: the old ones).
    corr_given overrides the corr pairs the update reads (the device's own values)."""
    partials = np.array([chunk_sumsq(r.grad[:row_counts(r.count)[0]], gs, r.vec) for r in rows],
                        dtype=np.float32)
    total, scale = grad_norm(partials, clip)
    counts, corr = dict(counts or {}), dict(corr or {})
    if kind == "adam":
        k = adam_consts(betas[0], betas[1], eps)
        for pid, active in dict((r.pid, r.active) for r in rows).items():
            if advances(active):
                counts[pid] = counts.get(pid, 0) + 1
        counts = shared_counts(counts)
        for pid in set(r.pid for r in rows):
            if counts.get(pid, 0) > 0:
                corr[pid] = adam_corr(counts[pid], betas[0], betas[1])
    use = dict(corr)
    use.update(corr_given or {})
    out = []
    for r in rows:
        n = row_counts(r.count)[1]
        new = [np.array(a, dtype=np.float32) for a in (r.param,) + tuple(r.state)]
        if n > 0 and is_live(r.active):
            g, (p, *st) = _vec(r.grad)[:n], [a[:n] for a in new]
            lr, wd = f32(r.lr), f32(r.wd)
            if kind == "sgd":
                res = sgd1(g, p, st[0], gs, scale, wd, lr, momentum)
            else:
                c0, c2 = use.get(r.pid, (0.0, 0.0))  # (a corr pair never written reads 0)
                res = adam1(g, p, st[0], st[1], gs, scale, wd, _w(lr * f32(c0)), c2, k)
            for a, b in zip(new, res):
                a[:n] = b
        out.append(tuple(new))
    return Result(partials, total, scale, out, counts, corr)


# ------------------------------------------------------------------ the fp64 truth
class Truth:
    """clip_gradient + the optimizer's update in fp64 (the clip scale in fp64 too).  Adam:
    d = g + wd*p; m = b1*m + (1-b1)*d; v = b2*v + (1-b2)*d*d;
    p -= (lr / (1-b1^t)) * m / (sqrt(v) / sqrt(1-b2^t) + eps), t the parameter's own count.
    SGD: d = g + wd*p; buf = mom*buf + d; p -= lr*buf."""

    def __init__(self, groups, clip, kind="adam", momentum=0.9):
        import torch
        self.kind, self.clip, self.momentum = kind, clip, momentum
        self.groups = [dict(g, params=[p.detach().double().clone() for p in g["params"]])
                       for g in groups]
        self.params = [p for g in self.groups for p in g["params"]]
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]
        self.t = [0] * len(self.params)
        self.norm = 0.0  # the last step's gradient norm

    def step(self, grads, norm_only=()):
        """norm_only: indices of parameters whose gradient enters the norm and nothing else
        (a table's norm-only rows without the tiles that would update them)."""
        gs = [None if g is None else g.detach().double() for g in grads]
        s = 1.0
        self.norm = math.sqrt(sum(float((g * g).sum()) for g in gs if g is not None))
        if self.clip > 0:
            tot = self.norm
            s = self.clip / max(tot, self.clip)
        i = -1
        for grp in self.groups:
            lr, wd = grp["lr"], grp["weight_decay"]
            for p in grp["params"]:
                i += 1
                if gs[i] is None or i in norm_only:
                    continue
                d = gs[i] * s + wd * p
                if self.kind == "sgd":
                    self.m[i] = self.momentum * self.m[i] + d
                    p -= lr * self.m[i]
                    continue
                self.t[i] += 1
                t = self.t[i]
                self.m[i] = B1 * self.m[i] + (1 - B1) * d
                self.v[i] = B2 * self.v[i] + (1 - B2) * d * d
                p -= (lr / (1 - B1 ** t)) * self.m[i] / (
                    self.v[i].sqrt() / math.sqrt(1 - B2 ** t) + EPS)


def check_bar(fused, ref, truth, what=""):
    """max |fused - truth| <= max(2 * max |ref - truth|, 4 ulp of max |truth|), per tensor;
    returns the largest fused / torch error ratio seen (printed for DESIGN.md)."""
    worst = 0.0
    for i, (f, r, t) in enumerate(zip(fused, ref, truth)):
        e_f = float((f.detach().double() - t).abs().max())
        e_t = float((r.detach().double() - t).abs().max())
        top = float(t.abs().max())
        ulp = 2.0 ** (math.floor(math.log2(top)) - 23) if top > 0 else 2.0 ** -149
        bar = max(2 * e_t, 4 * ulp)
        print(f"{what} tensor {i}: E_fused {e_f:.3e}  E_torch {e_t:.3e}  "
              f"ratio {e_f / e_t if e_t else float('nan'):.3f}  4ulp {4 * ulp:.3e}")
        assert e_f <= bar, (what, i, e_f, e_t, 4 * ulp)
        if e_t:
            worst = max(worst, e_f / e_t)
    return worst
