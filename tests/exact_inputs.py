"""Operands for which fp64, f32 and the split-bf16 arithmetic must agree to the last bit.

The split-bf16 kernels (csrc/bs_common.h) split each f32 operand exactly into three bf16
planes, x = hi + mid + lo, and sum six (bf16x6) or three (bf16x3) of the nine plane products
on the bf16 MFMA.  The Gaussian-data tests hold them to bars ~30x their real error, so a
mistake confined to a mid or lo plane (a plane staged from the wrong offset in a ragged tail,
a dropped a2b0 in one code path) fits under the bar.  The operands built here close that gap:

  1. the products the math mode drops are exactly zero (by the operands' significant bits),
  2. every term of every output sum is a multiple of one grain 2^-q,
  3. sum |terms| < 2^(24-q) for every output.

Under 2 and 3 every partial sum — inside an MFMA, across k-steps, across split-K slabs,
through the slab reduce and the epilogue — is an f32 number exactly, in any order, so the
kernel must reproduce the fp64 reference cast to f32 bit for bit (torch.equal), whatever its
tiling or schedule.  Every kept plane product then has to be right at every index.  ("Bit
for bit" with one exception, here and wherever these tests say it: torch.equal takes -0.0
and +0.0 for equal, so the sign of an exact zero is not pinned.)

Operand classes (`dense`: +-(1 + r 2^-Q), r uniform in [0, 2^Q); `sparse`: mostly zeros, the
nonzero entries +-(1 + r 2^-Qs)):

  class   dense Q  sparse Qs  exact under          pins
  24x8    19       0 (+-1)    bf16x6, f32          a0b0 a1b0 a2b0 (dense = A) / a0b0 a0b1 a0b2
  16x16   9        9          bf16x6, f32          a1b1 and the four hi / mid products
  16x8    15       0 (+-1)    bf16x3, bf16x6, f32  the three bf16x3 products on two planes
  hi      7        7          everything           a0b0 alone: the check of the exactness
                                                   model itself (8-bit values, hi planes only)

Every path under test is a bilinear operation ref(A, B) (a GEMM, a convolution, one of its
gradients) plus an epilogue, so one description serves them all: `Op` holds the fp64
reference, how the sparse pattern of each operand is laid out (`perm` / `lead`: which view
of the operand has the reduction index K last and how many of its leading dimensions index
a row; `per`: how many entries per row may be nonzero), and along which dimension a plane is
rolled "by one element along K" in the sensitivity check (`kdim`).

Each case runs `rounds` times with the sparse pattern shifted, until every element of the
dense operand has met a nonzero partner in some output (`coverage`).  This module needs no
GPU; tests/test_exact_inputs_cpu.py asserts the three conditions, the coverage and the
sensitivity (on the torch model of the split below) for every case the GPU modules run.
"""
import functools
import math
import zlib

import torch
import torch.nn.functional as F

CLASSES = {"24x8": (19, 0), "16x16": (9, 9), "16x8": (15, 0), "hi": (7, 7)}
# the classes each math mode must reproduce exactly
EXACT = {"f32": ("24x8", "16x16", "16x8", "hi"), "bf16x6": ("24x8", "16x16", "16x8", "hi"),
         "bf16x3": ("16x8", "hi")}
# kept plane products (a plane, b plane) of bs_mac<6>; bs_mac<3> keeps the first three
PRODUCTS = ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2))
# (dense = A, dense = B): the products with a nonzero contribution in each class
PINS = {"24x8": (((0, 0), (1, 0), (2, 0)), ((0, 0), (0, 1), (0, 2))),
        "16x16": (((0, 0), (1, 0), (0, 1), (1, 1)),) * 2,
        "16x8": (((0, 0), (1, 0)), ((0, 0), (0, 1))),
        "hi": (((0, 0),),) * 2}


def grain(cls):
    """q: every product of a dense and a sparse value of the class is a multiple of 2^-q."""
    return sum(CLASSES[cls])


# ------------------------------------------------------------------------------ values
def _gen(seed, rnd, salt):
    return torch.Generator().manual_seed((seed * 1009 + rnd) * 7 + salt)


def values(shape, Q, g):
    """+-(1 + r 2^-Q), r uniform in [0, 2^Q): Q + 1 significant bits, exact in f32."""
    r = torch.randint(0, 1 << Q, shape, generator=g, dtype=torch.int64)
    s = torch.randint(0, 2, shape, generator=g, dtype=torch.int64) * 2 - 1
    return (s.double() * (1.0 + r.double() * 2.0 ** -Q)).float()


def dense(shape, cls, seed, rnd):
    """The dense operand of a class.  Its mid plane (Q >= 8) and lo plane (Q >= 16) must be
    nonzero in at least half of the elements: a draw of a very small operand that misses
    that is drawn again (a 1 x 3 operand has a lo plane with two zeros once in ten draws)."""
    Q = CLASSES[cls][0]
    for salt in range(1, 400, 10):
        x = values(shape, Q, _gen(seed, rnd, salt))
        planes = split3(x)[1:1 + (Q >= 8) + (Q >= 16)]
        if all(float((p != 0).float().mean()) >= 0.5 for p in planes):
            return x
    raise AssertionError((shape, cls))


def _stride(K):
    """A stride coprime to K (the pattern then visits every k before repeating one)."""
    for p in (37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79):
        if math.gcd(p, K) == 1:
            return p
    return 1


def row_pattern(R, K, per, rnd):
    """(R, K) bool: row r is nonzero at k = ((r per + j + rnd R per) P) mod K, j < per, P a
    stride coprime to K.  R per consecutive slots per round: ceil(K / (R per)) rounds visit
    every k, and a row never has more than `per` entries."""
    P = _stride(K)
    r = torch.arange(R, dtype=torch.int64).view(R, 1)
    j = torch.arange(min(per, K), dtype=torch.int64).view(1, -1)
    k = ((r * per + j + rnd * R * per) * P) % K
    m = torch.zeros(R, K, dtype=torch.bool)
    m.scatter_(1, k, True)
    return m


def integers(shape, lo, hi, seed, salt=5):
    """Integers in [lo, hi] as f32 (bias / residual / accumulate-base terms: multiples of any
    grain 2^-q, q >= 0)."""
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed, 0, salt)).float()


def pow2_scale(n, seed):
    """Per-channel epilogue scales in {1, 1/2} (powers of two: scaling is exact)."""
    return 0.5 ** torch.randint(0, 2, (n,), generator=_gen(seed, 0, 9)).float()


# ------------------------------------------------------------------------------ operations
class Op:
    """One bilinear operation c = ref(A, B) on CPU tensors in the reference's own layouts.

    shape_a / shape_b: the operands' shapes.  perm_a / perm_b with lead_a / lead_b: the
    permutation of an operand whose first `lead` dimensions index a row of the sparse
    pattern and whose remaining dimensions, flattened, are its K index; per_a / per_b: the
    most nonzero entries per row (they keep every output sum at <= 9 terms).  kdim_a /
    kdim_b: the dimension that a "roll by one element along K" shifts.  pats_a: instead of
    the row pattern, a function returning A's patterns round by round (greedy_act)."""

    def __init__(self, name, shape_a, shape_b, ref, perm_a, per_a, perm_b, per_b, kdim_a, kdim_b,
                 lead_a=1, lead_b=1, excl_b=None, pats_a=None, out_shape=None):
        self.out_shape = tuple(out_shape)
        self.name, self.shape_a, self.shape_b, self.ref = name, tuple(shape_a), tuple(shape_b), ref
        self.perm = (perm_a, perm_b)
        self.per = (per_a, per_b)
        self.kdim = (kdim_a, kdim_b)
        self.lead = (lead_a, lead_b)   # leading dims of the permuted operand that form a row
        self.excl_b = excl_b           # bool tensor: elements of B that meet only padding
        self.shapes = (self.shape_a, self.shape_b)
        self.pats_a = pats_a           # () -> the per-round patterns of A (greedy_act)

    def pattern(self, side, rnd):
        if side == 0 and self.pats_a is not None:
            pats = self.pats_a()
            return pats[rnd % len(pats)]
        shape, perm, lead = self.shapes[side], self.perm[side], self.lead[side]
        pshape = [shape[d] for d in perm]
        R = math.prod(pshape[:lead])
        K = math.prod(pshape[lead:])
        m = row_pattern(R, K, self.per[side], rnd).view(pshape)
        inv = [perm.index(d) for d in range(len(perm))]
        return m.permute(inv).contiguous()

    def operands(self, cls, side, seed, rnd):
        """(A, B) f32: operand `side` (0 = A, 1 = B) dense, the other sparse."""
        d = dense(self.shapes[side], cls, seed, rnd)
        o = 1 - side
        s = values(self.shapes[o], CLASSES[cls][1], _gen(seed, rnd, 2)) * self.pattern(o, rnd)
        return (d, s) if side == 0 else (s, d)


def gemm_op(M, N, K):
    """c[m][n] = sum_k A[m][k] B[n][k]."""
    return Op(f"gemm{(M, N, K)}", (M, K), (N, K), lambda a, b: a @ b.t(),
              (0, 1), 8, (0, 1), 8, 1, 1, out_shape=(M, N))


def _taps_reachable(shape_w, H, W, KS):
    """Weight elements whose tap reads something other than padding at some output pixel."""
    ok = torch.ones(shape_w, dtype=torch.bool)
    if KS == 3:
        if H == 1:
            ok[:, :, 0, :] = ok[:, :, 2, :] = False
        if W == 1:
            ok[:, :, :, 0] = ok[:, :, :, 2] = False
    return ok


@functools.lru_cache(maxsize=None)
def greedy_act(kind, N, C, H, W, KS, stride, pad):
    """The sparse activation patterns of a KS > 1 convolution (kind fwd: x; dgrad: dy), one
    bool (N, C, h, w) tensor per round, one active channel per pixel: an output sums over a
    KS x KS window of pixels, so it has at most 9 terms (a strided 5x5 window holds 25
    pixels: a round then keeps the pixels of one 2x2 phase only, at most 9 per window).

    The dense partner is the weight: w[., c, tap] is covered once channel c is active at a
    pixel from which `tap` reaches an in-range output.  On small maps few pixels reach every
    tap (a 3 x 3 map: the centre alone), so a fixed rotation of channels over pixels needs
    hundreds of rounds, or never gets there when the channel count resonates with the row
    length.  Instead each pixel, best-connected first, takes the channel that still lacks
    the most of the taps it reaches; rounds are added until no (channel, tap) pair is
    lacking.  Deterministic, no random numbers."""
    Ho, Wo = (H + 2 * pad - KS) // stride + 1, (W + 2 * pad - KS) // stride + 1
    k = torch.arange(KS)

    def reach(n_in, n_out, fwd):  # (positions, taps) bool along one axis
        pos = torch.arange(n_in).view(-1, 1)
        if fwd:  # input position -> output (pos + pad - k) / stride
            o = pos + pad - k
            return (o % stride == 0) & (o >= 0) & (o // stride < n_out)
        o = pos * stride - pad + k  # output-gradient position -> input position
        return (o >= 0) & (o < n_out)
    if kind == "fwd":
        h, w, rh, rw = H, W, reach(H, Ho, True), reach(W, Wo, True)
    else:
        h, w, rh, rw = Ho, Wo, reach(Ho, H, False), reach(Wo, W, False)
    valid = (rh.view(h, 1, KS, 1) & rw.view(1, w, 1, KS)).reshape(h * w, KS * KS)
    need = valid.any(0).view(1, -1).repeat(C, 1)
    order = sorted(range(h * w), key=lambda p: (-int(valid[p].sum()), p))
    phases = 4 if KS > 3 else 1
    pats = []
    while bool(need.any()):
        assert len(pats) < 512, (kind, N, C, H, W, KS)
        rnd = len(pats)
        m = torch.zeros(N, C, h * w, dtype=torch.bool)
        a, b = divmod(rnd % phases, 2)
        for n in range(N):
            for p in order:
                if phases > 1 and ((p // w) % 2, (p % w) % 2) != (a, b):
                    continue
                gain = (need & valid[p]).sum(1)
                c = int(gain.argmax())
                if int(gain[c]) == 0:
                    c = (p + rnd + n) % C
                m[n, c, p] = True
                need[c] &= ~valid[p]
        pats.append(m.view(N, C, h, w))
    return pats


def conv_op(kind, N, Cin, Cout, H, W, KS=3, stride=1, pad=None):
    """kind fwd: A = x, B = w -> y; dgrad: A = dy, B = w -> dx; wgrad: A = dy, B = x -> dw.
    x (N, Cin, H, W), w (Cout, Cin, KS, KS), `same` padding unless given.  Sparse patterns:
    activations of a 3x3 (or strided) conv one active channel per pixel (<= 9 terms per
    output; strided 5x5 windows see pixels of one 2x2 phase only, below), of a 1x1 conv 8;
    weights 8 nonzero (ci, tap) pairs per output row; in the weight gradient 8 nonzero pixels
    per channel of the sparse operand."""
    pad = KS // 2 if pad is None else pad
    Ho, Wo = (H + 2 * pad - KS) // stride + 1, (W + 2 * pad - KS) // stride + 1
    xs, ws, ys = (N, Cin, H, W), (Cout, Cin, KS, KS), (N, Cout, Ho, Wo)
    act_per = 1 if KS > 1 else 8
    name = f"conv{KS}s{stride}_{kind}{(N, Cin, Cout, H, W)}"
    excl = ~_taps_reachable(ws, H, W, KS) if stride == 1 else None
    pats = None
    if KS > 1 and kind != "wgrad":
        def pats():
            return greedy_act(kind, N, Cin if kind == "fwd" else Cout, H, W, KS, stride, pad)
    if kind == "fwd":
        return Op(name, xs, ws, lambda a, b: F.conv2d(a, b, stride=stride, padding=pad),
                  (0, 2, 3, 1), act_per, (0, 1, 2, 3), 8, 1, 1, lead_a=3, excl_b=excl,
                  pats_a=pats, out_shape=ys)
    if kind == "dgrad":
        return Op(name, ys, ws,
                  lambda a, b: torch.nn.grad.conv2d_input(xs, b, a, stride=stride, padding=pad),
                  (0, 2, 3, 1), act_per, (1, 0, 2, 3), 8, 1, 0, lead_a=3, excl_b=excl,
                  pats_a=pats, out_shape=xs)
    assert kind == "wgrad"
    return Op(name, ys, xs,
              lambda a, b: torch.nn.grad.conv2d_weight(b, ws, a, stride=stride, padding=pad),
              (1, 0, 2, 3), 8, (1, 0, 2, 3), 8, "hw", "hw", out_shape=ws)


# ------------------------------------------------------------------------------ epilogues
class Epilogue:
    """out = mask(act(c * scale + bias + residual)) around the bilinear result c, with terms
    that keep the exactness conditions: scale in {1, 1/2} per channel (a channel scaled by
    1/2 has grain 2^-(q+1)), bias and residual small integers, the mask a ReLU output.
    `parts`: a string of s (scale) b (bias) r (residual) a (ReLU) m (mask).  chan: the output
    dimension that scale and bias run along.  The same tensors serve every round of a case."""

    def __init__(self, out_shape, chan, parts, seed):
        self.parts = parts
        C = out_shape[chan]
        bc = [1] * len(out_shape)
        bc[chan] = C
        self.bc = bc
        self.scale = pow2_scale(C, seed) if "s" in parts else None
        self.bias = integers((C,), -2, 2, seed, 6) if "b" in parts else None
        self.residual = integers(out_shape, -2, 2, seed, 7) if "r" in parts else None
        self.relu = "a" in parts
        self.mask = torch.relu(integers(out_shape, -2, 2, seed, 8)) if "m" in parts else None

    def post(self, c, act=True):
        """The epilogue in fp64 on the bilinear result c (act=False: before ReLU and mask)."""
        v = c
        if self.scale is not None:
            v = v * self.scale.double().view(self.bc)
        if self.bias is not None:
            v = v + self.bias.double().view(self.bc)
        if self.residual is not None:
            v = v + self.residual.double()
        if act and self.relu:
            v = torch.relu(v)
        if act and self.mask is not None:
            v = v * (self.mask > 0)
        return v

    def abs_sum(self, c_abs):
        """sum |terms| per output, from the bilinear result on |A|, |B|."""
        v = c_abs
        if self.scale is not None:
            v = v * self.scale.double().view(self.bc)
        if self.bias is not None:
            v = v + self.bias.double().abs().view(self.bc)
        if self.residual is not None:
            v = v + self.residual.double().abs()
        return v

    def q(self, q):
        """The grain per output: q + 1 where the channel is scaled by 1/2."""
        if self.scale is None:
            return q
        return (q - torch.log2(self.scale.double())).view(self.bc)


BS_MODES = (("bf16x6", "24x8"), ("bf16x6", "16x16"), ("bf16x3", "16x8"), ("bf16x3", "16x16"))
F32_MODES = (("f32", "24x8"),)


class Case:
    """One path at one shape: `path` names the GPU module's runner, maker(*key) builds the
    Op, `epi` the epilogue parts (Epilogue) along output dimension `chan`, `modes` the (math,
    class) pairs and `sides` the dense sides to run.  wscale: operand B reaches the kernel
    unscaled beside a per-row scale in {1, 1/2} along B's dimension 0 (the reference takes
    B * wscale: grain 2^-(q+1)).  arg: anything else the runner needs (a layout, a kernel
    size); env: environment variables for the run; post: applied after the epilogue."""

    def __init__(self, path, maker, key, epi="", chan=1, modes=BS_MODES, sides=(0, 1),
                 wscale=False, arg=None, env=None, post=None):
        self.path, self.maker, self.key, self.parts, self.chan = path, maker, tuple(key), epi, chan
        self.modes, self.sides, self.arg, self.env, self.post = modes, sides, arg, env or {}, post
        self.has_wscale = wscale
        self.id = f"{path}-{'x'.join(str(k) for k in key)}" + (f"-{epi}" if epi else "") + \
            ("-wscale" if wscale else "") + (f"-{arg}" if arg is not None else "")
        self.seed = zlib.crc32(self.id.encode()) % 100003

    def build(self):
        op = self.maker(*self.key)
        epi = Epilogue(op.out_shape, self.chan, self.parts, self.seed) if self.parts else None
        return op, epi

    @property
    def q_extra(self):
        return 1 if self.has_wscale else 0

    def wscale(self, op):
        return pow2_scale(op.shape_b[0], self.seed + 1) if self.has_wscale else None

    def eff(self, op):
        """(A, B) -> the operands the reference takes."""
        if not self.has_wscale:
            return None
        w = self.wscale(op).view([-1] + [1] * (len(op.shape_b) - 1))
        return lambda A, B: (A, B * w)

    def rounds(self, side):
        return rounds_for(self.maker, self.key, side)


def expand(cases):
    """([(case, math, cls, side)], [id]) for pytest.mark.parametrize."""
    out, ids = [], []
    for c in cases:
        for math_, cls in c.modes:
            for side in c.sides:
                out.append((c, math_, cls, side))
                ids.append(f"{c.id}-{math_}-{cls}-dense{'AB'[side]}")
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return out, ids


def run_case(case, math, cls, side, run):
    """The GPU check of one expanded case; run(A, B, epi, op) -> the kernel's result."""
    op, epi = case.build()
    run_rounds(op, case.rounds(side), cls, side, math, lambda A, B: run(A, B, epi, op), case.seed,
               epi, case.post, case.q_extra, case.eff(op))


def run_rounds(op, rounds, cls, side, math, run, seed, epi=None, post=None, q_extra=0, eff=None):
    """The GPU check of one case: over the rounds, run(A, B) -> the kernel's result for CPU
    operands A, B, compared bit for bit with the fp64 reference (through the epilogue).

    A class the math mode must reproduce (EXACT) is held to the fp64 reference.  Class 16x16
    under bf16x3 is the fidelity check: a1b1 is nonzero and dropped, so the result must equal
    the three-product model bit for bit (every kept term is still a multiple of the grain)
    and must differ from the reference in some round — a path that ran six products for
    "bf16x3" would match it.  post: a function applied after the epilogue (pooling)."""
    q = grain(cls) + q_extra
    fid = cls not in EXACT[math]
    assert not fid or (math, cls) == ("bf16x3", "16x16")
    differs = False
    for rnd in range(rounds):
        A, B = op.operands(cls, side, seed, rnd)
        got = run(A, B)
        if eff is not None:
            A, B = eff(A, B)
        c = model(op.ref, A, B, 3) if fid else op.ref(A.double(), B.double())
        want = epi.post(c) if epi is not None else c
        want = post(want) if post is not None else want
        what = f"{op.name} {math} {cls} dense={'AB'[side]} round {rnd}"
        assert_bits(got, want, epi.q(q) if epi is not None and post is None else q, what)
        if fid:
            full = op.ref(A.double(), B.double())
            full = epi.post(full) if epi is not None else full
            full = post(full) if post is not None else full
            differs |= not torch.equal(full.float(), want.float())
    if fid:
        assert differs, f"{op.name}: bf16x3 on class 16x16 matches the six-product reference"


def check_conditions(op, rounds, cls, side, seed, epi=None, q_extra=0, eff=None):
    """The CPU check of one case: exactness (conditions 2 and 3, every round), through the
    epilogue when there is one."""
    q = grain(cls) + q_extra
    for rnd in range(rounds):
        A, B = op.operands(cls, side, seed, rnd)
        if eff is not None:
            A, B = eff(A, B)
        c = op.ref(A.double(), B.double())
        ca = op.ref(A.double().abs(), B.double().abs())
        what = f"{op.name} {cls} dense={'AB'[side]} round {rnd}"
        assert_exact_case(c, ca, q, what)  # the bilinear part (split-K slabs hold it raw)
        if epi is not None:
            assert_exact_case(epi.post(c), epi.abs_sum(ca), epi.q(q), what + " epilogue")
            assert_exact_case(epi.post(c, act=False), epi.abs_sum(ca), epi.q(q),
                              what + " pre-activation")


def check_sensitivity(op, cls, side, seed, math):
    """Without a GPU, the proof that the case would fail on the bug it is for (round 0, the
    torch model of the split): the planes the class pins are nonzero in at least half of the
    dense operand's elements; each kept product the class pins contributes (removing it
    changes the modelled result); each pinned plane of the dense operand rolled by one
    element along K changes it."""
    A, B = op.operands(cls, side, seed, 0)
    planes = (split3(A), split3(B))
    nprod = 3 if math == "bf16x3" else 6
    pins = [ij for ij in PINS[cls][side] if ij in PRODUCTS[:nprod]]
    for ij in PRODUCTS[:nprod]:  # the class's claim: the other kept products are zero
        if ij not in pins:
            assert not (bool(planes[0][ij[0]].any()) and bool(planes[1][ij[1]].any())), ij
    for ij in pins:
        p = planes[side][ij[side]]
        frac = float((p != 0).float().mean())
        assert frac >= 0.5, \
            f"{op.name} {cls}: plane {ij[side]} nonzero in {frac:.0%} of the dense operand"
        t = op.ref(planes[0][ij[0]].double(), planes[1][ij[1]].double())
        assert bool(t.any()), f"{op.name} {cls}: removing product {ij} changes nothing"
        rolled = roll_k(p, op.kdim[side]).double()
        t2 = op.ref(rolled, planes[1][ij[1]].double()) if side == 0 else \
            op.ref(planes[0][ij[0]].double(), rolled)
        assert not torch.equal(t, t2), \
            f"{op.name} {cls}: plane {ij[side]} rolled along K changes nothing"
    total = model(op.ref, A, B, nprod)
    if cls in EXACT[math]:
        assert torch.equal(total, op.ref(A.double(), B.double()))
    else:
        assert not torch.equal(total, op.ref(A.double(), B.double()))


# ------------------------------------------------------------------------------ the model
def split3(x):
    """The three bf16 planes of an f32 tensor as f32 (bs_common.h split2; the construction of
    _ref_pack in tests/test_conv_bs_gpu.py): hi = the truncated top 8 significant bits, mid
    and lo the round-to-nearest-even bf16 of the remainders."""
    x = x.float().contiguous()
    hi = (x.view(torch.int32) & -65536).view(torch.float32)
    r = x - hi
    mid = r.to(torch.bfloat16).float()
    lo = (r - mid).to(torch.bfloat16).float()
    assert torch.equal(hi.double() + mid.double() + lo.double(), x.double())
    return [hi, mid, lo]


def roll_k(p, kdim):
    """A plane rolled by one element along K: a dimension, or "hw" for the flattened pixels
    of a map (the weight gradient's K)."""
    if kdim == "hw":
        return torch.roll(p.flatten(2), 1, 2).view_as(p)
    return torch.roll(p, 1, kdim)


def model(op_ref, A, B, nprod, drop=None):
    """bs_mac<nprod> in fp64: the sum of the kept plane products, each taken through the
    bilinear reference.  drop: one (i, j) product left out."""
    pa, pb = split3(A), split3(B)
    out = None
    for ij in PRODUCTS[:nprod]:
        if ij == drop:
            continue
        t = op_ref(pa[ij[0]].double(), pb[ij[1]].double())
        out = t if out is None else out + t
    return out


# ------------------------------------------------------------------------------ assertions
def assert_exact_case(ref64, abs64, q, what=""):
    """Conditions 2 and 3 in fp64.  ref64: the reference result; abs64: sum |terms| per
    output (the reference on |A|, |B|, plus |bias|, |residual| ...); q: the grain 2^-q, a
    number or a tensor broadcastable to ref64 (outputs scaled by 2^-k have grain 2^-(q+k))."""
    g = torch.as_tensor(2.0, dtype=torch.float64) ** torch.as_tensor(q, dtype=torch.float64)
    t = ref64 * g
    assert torch.equal(t, t.round()), f"{what}: a term is not a multiple of the grain"
    worst = float((abs64 * g).max())
    assert worst < 2.0 ** 24, f"{what}: sum|terms| = {worst:.0f} grains, not below 2^24"
    assert torch.equal(ref64.float().double(), ref64), f"{what}: reference not an f32 number"


def is_exact_case(ref64, abs64, q):
    """Whether conditions 2 and 3 hold (assert_exact_case as a predicate): the decision, made
    by the conditions themselves, whether an output is held to fp64 bit for bit."""
    try:
        assert_exact_case(ref64, abs64, q)
    except AssertionError:
        return False
    return True


def f32_sum_bound(abs64, n):
    """The error bound of an f32 sum of n terms in any order, n u sum |terms| with u = 2^-24
    (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4: gamma_(n-1) <= n u up
    to n = 4096): what is true of a sum that misses condition 3."""
    assert n <= 4096
    return abs64 * (n * 2.0 ** -24)


def assert_f32_sum(got, ref64, abs64, n, q, what=""):
    """An f32 sum of n multiples of 2^-q that misses condition 3: every partial sum is still
    a multiple of 2^-q (rounding only coarsens the grain), and the result lies within
    f32_sum_bound of fp64."""
    got = got.detach().double().cpu().view(ref64.shape)
    t = got * 2.0 ** q
    assert torch.equal(t, t.round()), f"{what}: not a multiple of 2^-{q}"
    err = (got - ref64).abs()
    bound = f32_sum_bound(abs64, n)
    worst = int((err - bound).argmax())
    assert bool((err <= bound).all()), \
        f"{what}: |error| {float(err.flatten()[worst]):.3g} at {worst} above the f32 " \
        f"summation bound {float(bound.flatten()[worst]):.3g}"


def coverage(op, side, rounds):
    """bool, shape of operand `side`: the elements that meet a nonzero partner in at least
    one output over the rounds (the gradient of sum ref(dense, |sparse|) w.r.t. dense)."""
    cov = torch.zeros(op.shapes[side], dtype=torch.bool)
    for rnd in range(rounds):
        cov |= coverage_round(op, side, rnd)
    return cov


def coverage_round(op, side, rnd):
    d = torch.ones(op.shapes[side], dtype=torch.float32, requires_grad=True)
    s = op.pattern(1 - side, rnd).float()
    out = op.ref(d, s) if side == 0 else op.ref(s, d)
    (g,) = torch.autograd.grad(out.sum(), d)
    return g != 0


def reachable(op, side):
    """The elements of operand `side` that can meet any partner at all: everything, except
    the taps of a 3x3 weight that read only padding on a one-row / one-column map."""
    ok = torch.ones(op.shapes[side], dtype=torch.bool)
    if side == 1 and op.excl_b is not None:
        ok &= ~op.excl_b
    return ok


MAX_ROUNDS = 96


@functools.lru_cache(maxsize=None)
def _rounds(op_key, side, maker):
    op = maker(*op_key)
    want = reachable(op, side)
    cov = torch.zeros_like(want)
    most = len(op.pats_a()) if side == 1 and op.pats_a is not None else MAX_ROUNDS
    for rnd in range(most):
        cov |= coverage_round(op, side, rnd)
        if torch.equal(cov, want):
            return rnd + 1
        assert not bool((cov & ~want).any())
    raise AssertionError(f"{op.name} side {side}: coverage "
                         f"{int(cov.sum())}/{int(want.sum())} after {most} rounds")


def rounds_for(maker, key, side):
    """The number of rounds after which operand `side` of maker(*key) is covered: the
    pattern shifts by one round's worth of slots per round (row_pattern), rounds are added
    until the coverage is 100 % of the reachable elements."""
    return _rounds(tuple(key), side, maker)


def _hex(t):
    return f"0x{int(t.view(torch.int32)) & 0xffffffff:08x}"


def assert_bits(got, ref64, q=None, what=""):
    """got (f32, any device) must equal the fp64 reference cast to f32 bit for bit.  On a
    mismatch: how many elements differ, the first differing index, both values as hex bit
    patterns and the error in grains 2^-q (the planes' magnitudes: a hi product ~2^q grains,
    a mid ~2^(q-8), a lo ~2^(q-16) — enough to tell a plane from a tile edge in the log)."""
    got = got.detach().float().cpu().contiguous()
    ref = ref64.detach().float().contiguous().view(got.shape)
    if torch.equal(got, ref):  # (-0.0 == 0.0: the sign of an exact zero is not pinned)
        return
    bad = (got != ref) | torch.isnan(got)
    idx = bad.nonzero()
    first = tuple(int(i) for i in idx[0])
    err = got.double()[first] - ref64.detach().view(got.shape)[first]
    grains = ""
    if q is not None:
        qm = int(torch.as_tensor(q).max())
        grains = f", error {float(err) * 2.0 ** qm:+.4g} x 2^-{qm}"
    last = tuple(int(i) for i in idx[-1])
    raise AssertionError(
        f"{what}: {int(bad.sum())} of {got.numel()} elements differ from fp64; first at "
        f"{first} (last at {last}): got {_hex(got[first])} ({float(got[first])!r}), want "
        f"{_hex(ref[first])} ({float(ref[first])!r}){grains}")
