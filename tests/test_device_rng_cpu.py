"""tests/device_rng.py without a GPU: the generator against known answers and an independent
plain-integer restatement, the four sampling rules' distributions, the case builders of
tests/test_device_rng_gpu.py (imported, so the two cannot drift apart), and — for each
plausible defect — that a defective rule changes what some committed GPU case expects.
"""
import numpy as np
import pytest

import device_rng as R
import test_device_rng_gpu as G

M64 = (1 << 64) - 1


# ------------------------------------------------------------------ the generator
def test_mix64_known_answers():
    """splitmix64's first three outputs for seed 0 (its state advances by the golden ratio
    before each finalisation, which mix64 folds in)."""
    g = 0x9e3779b97f4a7c15
    assert int(R.mix64(0)) == 0xe220a8397b1dcdaf
    assert int(R.mix64(g)) == 0x6e789e6aa1b965f4
    assert int(R.mix64((2 * g) & M64)) == 0x06c45d188009454f
    assert [int(v) for v in R.mix64(np.array([0, g, (2 * g) & M64], np.uint64))] == \
        [0xe220a8397b1dcdaf, 0x6e789e6aa1b965f4, 0x06c45d188009454f]


def _py_mix(z):
    z = (z + 0x9e3779b97f4a7c15) & M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def _py_u64(seed, stream, idx):
    return _py_mix((_py_mix(seed ^ ((stream * 0xd1b54a32d192ed03) & M64)) + idx) & M64)


SEEDS = (0, 123, 2 ** 32 + 123, 2 ** 62 - 1, 2 ** 63 + 5, 2 ** 64 - 1)
STREAMS = (0, 1, 17, 0x5eed)
INDICES = [0, 1, 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1]


@pytest.mark.parametrize("seed", SEEDS)
def test_rng_against_plain_integers(seed):
    idx = np.array(INDICES, np.uint64)
    for stream in STREAMS:
        want = [_py_u64(seed, stream, i) for i in INDICES]
        assert [int(v) for v in R.rng_u64(seed, stream, idx)] == want
        assert [int(v) for v in R.key32(seed, stream, idx)] == [w >> 32 for w in want]
        u = R.rng_unit(seed, stream, idx)
        assert u.dtype == np.float64 and bool((u < 1.0).all()) and bool((u >= 0.0).all())
        assert u.tolist() == [(w >> 11) * 2.0 ** -53 for w in want]
        assert R._rng_key(seed, stream, idx).dtype == np.uint32
    # every seed bit matters: the 32-bit truncation is another stream
    if seed >> 32:
        assert int(R.rng_u64(seed, 0, idx)[0]) != int(R.rng_u64(seed & 0xffffffff, 0, idx)[0])


def test_largest_unit_stays_inside_every_list():
    u = 1.0 - 2.0 ** -53  # rng_unit's largest value
    n = np.arange(1, 4097, dtype=np.float64)
    assert bool((np.floor(u * n) < n).all())


def test_generator_inverse_places_a_draw():
    for v in (0, 1, 0x8000000000000000, M64, 0x123456789abcdef0):
        assert int(R.mix64(R.unmix64(v))) == v
    for stream, idx, v in ((0x5eed, 100, 1 << 63), (17, 2 ** 40, 12345), (0, 0, M64)):
        seed = R.seed_for(stream, idx, v)
        assert 0 <= seed <= M64 and _py_u64(seed, stream, idx) == v


# ------------------------------------------------------------------ the rules: uniformity
def _z(count, trials, p):
    return np.abs(count - trials * p) / np.sqrt(trials * p * (1 - p))


def test_pt_draws_are_uniform():
    """Over 3000 seeds (both kinds present, nfg = 40, nbg = 13, S = 64, fg_per = 16): every fg
    position is in the kept prefix at the rate 16 / 40 and turns up in each of its 16 slots
    at the rate 1 / 40; every bg index is drawn at the rate 1 / 13.  Bars: 5 sd of the
    binomial.  The single-kind branches draw S uniforms from the fg / the bg stream."""
    nfg, nbg, S, fg_per, seeds = 40, 13, 64, 16, 3000
    slot = np.zeros((nfg, fg_per))
    bg = np.zeros(nbg)
    for s in range(seeds):
        perm, u = R.pt_draws(nfg, nbg, S, fg_per, s, s % 3)
        assert sorted(perm.tolist()) == list(range(nfg)) and len(u) == S - fg_per
        slot[perm[:fg_per], np.arange(fg_per)] += 1
        bg += np.bincount(np.floor(u * nbg).astype(int), minlength=nbg)
    assert _z(slot.sum(1), seeds, fg_per / nfg).max() < 5.0
    assert slot.min() > 0 and _z(slot, seeds, 1 / nfg).max() < 5.0
    assert _z(bg, seeds * (S - fg_per), 1 / nbg).max() < 5.0
    for nf, nb, st in ((7, 0, 16 + 2), (0, 7, 17 + 2)):
        hits = np.zeros(7)
        for s in range(seeds // 10):
            perm, u = R.pt_draws(nf, nb, S, fg_per, s, 1)
            assert len(perm) == 0 and u.tolist() == R.rng_unit(s, st, np.arange(S)).tolist()
            hits += np.bincount(np.floor(u * 7).astype(int), minlength=7)
        assert _z(hits, seeds // 10 * S, 1 / 7).max() < 5.0


def test_pt_draws_keep_fewer_than_fg_per():
    perm, u = R.pt_draws(5, 9, 64, 16, 1, 0)
    assert len(perm) == 5 and len(u) == 64 - 5


def test_pick_rows_are_uniform():
    n, k, seeds = 24, 6, 4000
    hits = np.zeros(n)
    for s in range(seeds):
        rows = R.pick_rows(n, k, s, s % 2)
        assert len(rows) == k and bool((np.diff(rows) > 0).all())
        hits[rows] += 1
    assert _z(hits, seeds, k / n).max() < 5.0
    assert R.pick_rows(5, 9, 0, 0).tolist() == [0, 1, 2, 3, 4]
    assert len(R.pick_rows(0, 4, 0, 0)) == 0 and len(R.pick_rows(4, 0, 0, 0)) == 0


@pytest.mark.parametrize("p", [0.5, 0.1, 0.9])
def test_dropout_keep_is_uniform_and_uncorrelated(p):
    n, seeds = 64, 4000
    q = 1.0 - float(np.float32(p))
    keep = np.stack([R.dropout_keep(n, p, s) for s in range(seeds + 1)]).astype(np.float64)
    assert _z(keep[:seeds].sum(0), seeds, q).max() < 5.0               # every index, over seeds
    assert _z(keep[:seeds].sum(1), n, q).max() < 5.0                   # every seed, over indices
    adj = (keep[:seeds, :-1] * keep[:seeds, 1:]).sum(0)                # i and i + 1
    assert _z(adj, seeds, q * q).max() < 5.0
    nxt = (keep[:seeds] * keep[1:]).sum(0)                             # seeds s and s + 1
    assert _z(nxt, seeds, q * q).max() < 5.0
    assert R.dropout_keep(5, 0.0, 9).all()


def test_anchor_subset_is_the_lexsort_rule():
    idx = np.array([7, 3, 99, 12, 40000, 5])
    k = R.key32(11, 3, idx)
    order = sorted(range(len(idx)), key=lambda i: (int(k[i]), int(idx[i])))
    for m in range(len(idx) + 1):
        assert sorted(R.anchor_subset(idx, m, 11, 3).tolist()) == sorted(order[:m])
    assert len(R.anchor_subset(idx, -4, 11, 3)) == 0


# ------------------------------------------------------------------ the GPU cases' builders
@pytest.mark.parametrize("case", G.PT_CASES, ids=lambda c: c.name)
def test_pt_case_hits_its_counts(case):
    """pt_inputs asserts (nfg, nbg) per image from the oracle's overlaps, away from the
    thresholds; here also the sort sizes and limits the case is there for."""
    rois, gt, counts = G.pt_inputs(case.name)
    assert rois.shape[1] + gt.shape[1] <= 4096 and gt.shape[1] <= 128
    assert counts == [tuple(i) for i in case.imgs]
    out = G.pt_expected(case.name, 5)
    S = G.RCNN[case.net]["batch"]
    assert out[0].shape == (len(counts), S, 5)
    for b, (nfg, nbg) in enumerate(counts):
        want_fg = S if nbg == 0 else min(nfg, G.pt_fg_per(G.RCNN[case.net]))
        assert int((out[1][b] > 0).sum()) == want_fg


def test_pt_cases_cover_the_sort_sizes():
    P = set()
    for c in G.PT_CASES:
        for nfg, nbg in c.imgs:
            if nfg and nbg:
                P.add(1 << max(nfg - 1, 0).bit_length())
    assert {1, 64, 128, 1024, 2048, 4096} <= P
    rois, gt, _ = G.pt_inputs("largest_sort_one_bg")
    assert rois.shape[1] + gt.shape[1] == 4096


@pytest.mark.parametrize("case", G.AT_CASES, ids=lambda c: c.name)
def test_at_case_hits_its_branch(case):
    n = G.BASE.shape[0] * case.H * case.W
    assert (n <= 38912) == (case.name not in ("b2_list", "few_fg_list"))  # kAtMax: LDS-key kernel
    for nfg, nbg in G.at_counts(case.name):
        if case.kind == "big":
            assert nfg > 128 and nbg > 256
        elif case.kind == "small":
            assert 0 < nfg < 128 and nbg > 256 - nfg
        else:
            assert nfg + nbg <= 256 and nfg + nbg > 0
    exp = G.at_expected(case.name, 5)
    for b, (nfg, nbg) in enumerate(G.at_counts(case.name)):
        assert int((exp[b] == 1).sum()) == min(nfg, 128)
        assert int((exp[b] >= 0).sum()) == min(256, nfg + nbg)
    if case.B == 2:
        assert not np.array_equal(exp[0], exp[1])


@pytest.mark.parametrize("counts,cap,post,head", G.PICK_CASES)
def test_pick_case_shapes(counts, cap, post, head):
    want, picks = G.pick_expected(counts, cap, post, head, 11)
    h = G.pick_head(post, head)
    for b, n in enumerate(counts):
        assert n <= cap <= 16384
        assert len(picks[b]) == min(max(n - h, 0), post - h)
        filled = min(n, h) + len(picks[b])
        assert bool((want[b, :filled, 1:] != 0).all()) and not want[b, filled:, 1:].any()


def test_drop_cases_cover_every_value():
    assert {s for s, _, _ in G.DROP_PARAMS} == set(G.DROP_SHAPES)
    for p in G.DROP_PS:
        assert {s for _, q, s in G.DROP_PARAMS if q == p} == set(G.DROP_SEEDS)
        assert {sh for sh, q, _ in G.DROP_PARAMS if q == p} == set(G.DROP_SHAPES)
    n = int(np.prod(G.DROP_SHAPES[4]))
    assert n > 8192 * 256 and n % 4 == 3  # second grid-stride trip, backward's scalar tail
    for p, below in G.DROP_EDGE:
        seed = G.drop_edge_seed(p, below)
        u = R.rng_unit(seed, R.DROPOUT_STREAM, np.array([G.EDGE_IDX]))[0]
        thr = float(np.float32(p))
        assert (u == thr) if below == 0 else (u == thr - 2.0 ** -53)
        assert bool(R.dropout_keep(G.EDGE_IDX + 1, p, seed)[G.EDGE_IDX]) == (below == 0)


# ------------------------------------------------------------------ defects change expectations
def _pt_all():
    return {(n, s): G.pt_expected(n, s) for n, s in G.PT_PARAMS} | \
        {("layer", k): G.pt_expected("b2_both_ordinary", G.pt_layer_seed(k)) for k in (1, 2)}


def _at_all():
    return {(n, s): G.at_expected(n, s) for n, s in G.AT_PARAMS} | \
        {("layer", k): G.at_expected("b2_lds", G.at_layer_seed(k)) for k in (1, 2)}


def _pick_all():
    return {(c, s): G.pick_expected(*c, s) for c in G.PICK_CASES for s in G.PICK_SEEDS}


def _drop_all():
    small = [(sh, p, s) for sh, p, s in G.DROP_PARAMS if np.prod(sh) < 4096]
    out = {k: G.drop_expected(G.drop_input(k[0]), k[1], k[2]).numpy() for k in small}
    y = G.drop_input((257,)).abs() + 0.5
    out.update({("edge", p, b): G.drop_expected(y, p, G.drop_edge_seed(p, b)).numpy()
                for p, b in G.DROP_EDGE})
    return out


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


def _changed(build, monkeypatch, patches):
    """Keys of build() whose expectation changes under the patched rules."""
    good = build()
    with monkeypatch.context() as m:
        for name, fn in patches.items():
            m.setattr(R, name, fn)
        bad = build()
    assert _same(list(good.values()), list(build().values()))  # the patch is gone again
    return {k for k in good if not _same(good[k], bad[k])}


def test_defect_swapped_fg_bg_stream(monkeypatch):
    pt = _changed(_pt_all, monkeypatch, {"pt_streams": lambda b: (17 + 2 * b, 16 + 2 * b)})
    assert pt == set(_pt_all())  # every case draws from one stream or the other
    at = _changed(_at_all, monkeypatch, {"anchor_streams": lambda b: (2 * b + 1, 2 * b)})
    assert at == set(_at_all()) - {("tiny_map", 5)}  # (nothing is drawn on the tiny map)


def test_defect_image_1_uses_image_0_stream(monkeypatch):
    pt = _changed(_pt_all, monkeypatch, {"pt_streams": lambda b: (16, 17)})
    assert pt == {k for k in _pt_all() if k[0] == "layer" or str(k[0]).startswith("b2_")}
    at = _changed(_at_all, monkeypatch, {"anchor_streams": lambda b: (0, 1)})
    assert at == {k for k in _at_all() if k[0] == "layer" or str(k[0]).startswith("b2_")}
    pk = _changed(_pick_all, monkeypatch, {"pick_stream": lambda b: 0})
    # every case whose image 1 has a real choice to make
    assert pk == {(c, s) for c, s in _pick_all()
                  if c[0][1] - G.pick_head(c[2], c[3]) > c[2] - G.pick_head(c[2], c[3]) > 0}
    assert pk


def test_defect_seed_masked_to_32_bits(monkeypatch):
    u64 = R.rng_u64
    patch = {"rng_u64": lambda seed, stream, idx: u64(seed & 0xffffffff, stream, idx)}
    pt = _changed(_pt_all, monkeypatch, patch)
    assert pt == {k for k in _pt_all() if k[0] == "layer" or k[1] >> 32}
    at = _changed(_at_all, monkeypatch, patch)
    assert at == {k for k in _at_all() if k[0] != "layer" and k[1] >> 32}  # (3 * 1000003 + k < 2^32)
    assert at
    pk = _changed(_pick_all, monkeypatch, patch)
    assert pk and all(s >> 32 for _, s in pk) and {s for _, s in pk} == set(G.PICK_SEEDS[1:])
    dr = _changed(_drop_all, monkeypatch, patch)
    wide = {k for k in _drop_all() if (k[0] == "edge" or k[2] >> 32)}
    # (a mask of one or three elements can come out the same by chance)
    assert {k for k in wide if k[0] == "edge" or k[0][0] >= 255} <= dr <= wide


def test_defect_exclusive_dropout_threshold(monkeypatch):
    dr = _changed(_drop_all, monkeypatch, {"dropout_below": lambda u, thr: u <= thr})
    assert dr == {("edge", p, 0) for p in G.DROP_PS}


def test_defect_picks_in_key_order(monkeypatch):
    def key_order(keys, k):
        return np.lexsort((np.arange(len(keys)), keys))[:k]
    pk = _changed(_pick_all, monkeypatch, {"pick_order": key_order})
    # every case that appends at least two rows for some image
    assert pk == {(c, s) for c, s in _pick_all()
                  if any(min(max(n - G.pick_head(c[2], c[3]), 0), c[2] - G.pick_head(c[2], c[3])) > 1
                         for n in c[0])}
    assert pk
