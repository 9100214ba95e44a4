"""The counter RNG of csrc/common.h and the four sampling rules built on it, restated in numpy.

  mix64      the splitmix64 finaliser (golden-ratio increment, two xor-shift multiplies);
  rng_u64    mix64(mix64(seed ^ stream * 0xd1b54a32d192ed03) + idx);
  rng_unit   (rng_u64 >> 11) * 2^-53 in float64, in [0, 1);
  key32      rng_u64 >> 32.

The rules return indices or masks, never boxes, so one restatement serves the GPU tests (which
hand them to the kernels' replay inputs and to the oracle) and the CPU tests (which check their
distributions and that a plausible defect changes them):

  anchor_subset   at_sample_lds_kernel / block_random_subset (csrc/targets.hip);
  pt_draws        pt_sample_kernel, perm == nullptr (csrc/targets.hip);
  pick_rows       proposal_pick_kernel, pick == nullptr (csrc/proposal.hip);
  dropout_keep    relu_dropout_kernel (csrc/act.hip).

Everything a defect could plausibly touch goes through the module-level names below
(rng_u64, pt_streams, anchor_streams, pick_stream, dropout_below, pick_order), so
tests/test_device_rng_cpu.py can swap one of them for a defective version.
"""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9e3779b97f4a7c15
MUL1, MUL2 = 0xbf58476d1ce4e5b9, 0x94d049bb133111eb
STREAM_MUL = 0xd1b54a32d192ed03
DROPOUT_STREAM = 0x5eed
_u = np.uint64


def _arr(x):
    """x (Python int of any size below 2^64, or an integer array) as a uint64 array."""
    if isinstance(x, np.ndarray):
        return x.astype(np.uint64)
    return np.asarray(x, dtype=np.uint64)  # (Python ints >= 2^63 convert exactly this way)


def mix64(z):
    z = _arr(z)
    with np.errstate(over="ignore"):
        z = z + _u(GOLDEN)
        z = (z ^ (z >> _u(30))) * _u(MUL1)
        z = (z ^ (z >> _u(27))) * _u(MUL2)
        return z ^ (z >> _u(31))


def rng_u64(seed, stream, idx):
    """idx vectorised; seed and stream are Python ints (taken mod 2^64, as the C ABI does)."""
    with np.errstate(over="ignore"):
        base = mix64((int(seed) & M64) ^ ((int(stream) * STREAM_MUL) & M64))
        return mix64(base + _arr(idx))


def rng_unit(seed, stream, idx):
    return (rng_u64(seed, stream, idx) >> _u(11)).astype(np.float64) * 2.0 ** -53


def key32(seed, stream, idx):
    return (rng_u64(seed, stream, idx) >> _u(32)).astype(np.uint32)


def _rng_key(seed, stream, idx):
    """(rng_u64(seed, stream, idx) >> 32) of csrc/common.h (splitmix64 twice), in numpy."""
    return key32(seed, stream, np.asarray(idx))


# ------------------------------------------------------------------ inverting the generator
def _unxorshift(z, s):
    out = z
    for _ in range(64 // s + 1):
        out = z ^ (out >> s)
    return out


def unmix64(v):
    """The z with mix64(z) == v (Python ints): every step of the finaliser is a bijection."""
    v = _unxorshift(v & M64, 31)
    v = (v * pow(MUL2, -1, 1 << 64)) & M64
    v = _unxorshift(v, 27)
    v = (v * pow(MUL1, -1, 1 << 64)) & M64
    v = _unxorshift(v, 30)
    return (v - GOLDEN) & M64


def seed_for(stream, idx, value):
    """The seed under which rng_u64(seed, stream, idx) == value: a draw placed by hand, e.g.
    exactly on the dropout threshold, which no search over seeds would find."""
    base = (unmix64(value) - idx) & M64
    return unmix64(base) ^ ((stream * STREAM_MUL) & M64)


# ------------------------------------------------------------------ the four rules
def anchor_streams(b):
    """(fg, bg) streams of image b in the anchor-target sampling kernels."""
    return 2 * b, 2 * b + 1


def pt_streams(b):
    """(fg, bg) streams of image b in pt_sample_kernel."""
    return 16 + 2 * b, 17 + 2 * b


def pick_stream(b):
    return b


def anchor_subset(cand_idx, m, seed, stream):
    """Positions (into cand_idx) of the m candidates the sampler drops: the m smallest
    (key32, anchor index) pairs.  cand_idx: the kernels' anchor indices (h, w, a order)."""
    cand_idx = np.asarray(cand_idx)
    if m <= 0:
        return np.zeros(0, np.int64)
    return np.lexsort((cand_idx, key32(seed, stream, cand_idx)))[:m]


def pt_draws(nfg, nbg, S, fg_per, seed, b):
    """(perm, uniforms) of image b, as proposal_target's replay mode takes them: perm is the
    whole fg permutation (the kernel keeps the first min(fg_per, nfg)), empty when only one
    kind of candidate exists; uniforms are the with-replacement draws, float64."""
    st_fg, st_bg = pt_streams(b)
    if nfg > 0 and nbg > 0:
        i = np.arange(nfg, dtype=np.uint64)
        keys = (key32(seed, st_fg, i).astype(np.uint64) << _u(32)) | i
        perm = np.argsort(keys, kind="stable").astype(np.int32)
        return perm, rng_unit(seed, st_bg, np.arange(S - min(fg_per, nfg)))
    if nfg > 0:
        return np.zeros(0, np.int32), rng_unit(seed, st_fg, np.arange(S))
    if nbg > 0:
        return np.zeros(0, np.int32), rng_unit(seed, st_bg, np.arange(S))
    raise ValueError("no fg and no bg candidate")


def pick_order(keys, k):
    """The k rows with the smallest (key, row) pairs, in ascending row."""
    r = np.arange(len(keys))
    return np.sort(np.lexsort((r, keys))[:k])


def pick_rows(n, k, seed, b):
    """Rows of the n survivors past the head that proposal_pick keeps: the k smallest
    (rng_u64(seed, b, r), r), returned in ascending r."""
    if n <= 0 or k <= 0:
        return np.zeros(0, np.int64)
    return pick_order(rng_u64(seed, pick_stream(b), np.arange(n)), min(k, n)).astype(np.int64)


def dropout_below(u, thr):
    """True where the element is dropped: u < thr (the kernel keeps u >= (double)p)."""
    return u < thr


def dropout_keep(n, p, seed):
    """Keep mask of relu_dropout_kernel over flat indices 0..n-1: p <= 0, or
    rng_unit(seed, 0x5eed, i) >= float64(float32(p))."""
    if p <= 0:
        return np.ones(n, bool)
    return ~dropout_below(rng_unit(seed, DROPOUT_STREAM, np.arange(n)), float(np.float32(p)))


class Replay:
    """The ``rng=`` object of proposal_target / oracle.rpn.proposal_target, fed from pt_draws
    image by image: permutation(nfg) then rand(n) when both kinds exist, rand(S) otherwise."""

    def __init__(self, counts, S, fg_per, seed):
        self.counts, self.S, self.fg_per, self.seed = list(counts), S, fg_per, seed
        self.b, self.u = 0, None

    def _next(self):
        nfg, nbg = self.counts[self.b]
        d = pt_draws(nfg, nbg, self.S, self.fg_per, self.seed, self.b)
        self.b += 1
        return nfg, d

    def permutation(self, n):
        assert self.u is None
        nfg, (perm, self.u) = self._next()
        assert n == nfg == len(perm), (n, nfg)
        return perm

    def rand(self, n):
        if self.u is None:
            _, (perm, self.u) = self._next()
            assert len(perm) == 0
        u, self.u = self.u, None
        assert len(u) == n, (len(u), n)
        return u

    def done(self):
        return self.b == len(self.counts) and self.u is None
