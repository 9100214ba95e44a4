"""The exact-operand generators (tests/exact_inputs.py) meet their conditions for every case
the GPU modules run — proved here without a GPU, on the fp64 references and the torch model
of the split (truncated hi, round-to-nearest-even mid and lo; the six / three kept products).

For every case of tests/test_conv_exact_gpu.py and tests/test_gemm_exact_gpu.py (the lists
are imported, so the two cannot drift apart):
  exactness    every round: ref * 2^q is integral and sum |terms| < 2^(24-q), bias, residual
               and power-of-two scales included;
  coverage     over the rounds the GPU test runs, every element of the dense operand meets a
               nonzero partner in some output — 100 %, except the taps of a dense 3x3 weight
               that read only padding on a one-row or one-column map (exactly those);
  sensitivity  the pinned planes are nonzero in at least half of the dense operand, removing
               any one kept product or rolling any one pinned plane by one element along K
               changes the modelled result.
"""
import pytest
import torch

import exact_inputs as E
import test_conv_exact_gpu as conv_cases
import test_gemm_exact_gpu as gemm_cases

PARAMS = conv_cases.PARAMS + gemm_cases.PARAMS
IDS = conv_cases.IDS + gemm_cases.IDS


def _dedup(key):
    seen, out, ids = set(), [], []
    for p, i in zip(PARAMS, IDS):
        k = key(p)
        if k not in seen:
            seen.add(k)
            out.append(p)
            ids.append(i)
    return out, ids


# the operands depend on (case, class, dense side), not on the math mode
_COND = _dedup(lambda p: (p[0].id, p[2], p[3]))
# the coverage depends on (operation, dense side) alone
_COV = _dedup(lambda p: (p[0].maker, p[0].key, p[3]))


@pytest.mark.parametrize("case,math,cls,side", _COND[0], ids=_COND[1])
def test_exactness_conditions(case, math, cls, side):
    op, epi = case.build()
    E.check_conditions(op, case.rounds(side), cls, side, case.seed, epi, case.q_extra,
                       case.eff(op))


@pytest.mark.parametrize("case,math,cls,side", _COV[0], ids=_COV[1])
def test_coverage_is_complete(case, math, cls, side):
    op, _ = case.build()
    rounds = case.rounds(side)
    cov = E.coverage(op, side, rounds)
    want = torch.ones(op.shapes[side], dtype=torch.bool)
    kind = case.key[0] if isinstance(case.key[0], str) else ""
    if side == 1 and kind in ("fwd", "dgrad") and op.shape_b[2:] == (3, 3):
        # the stated exclusion: border taps of a dense 3x3 weight on a one-row / one-column
        # map meet only padding
        H, W = op.shape_a[2:]
        if H == 1:
            want[:, :, 0, :] = want[:, :, 2, :] = False
        if W == 1:
            want[:, :, :, 0] = want[:, :, :, 2] = False
    assert torch.equal(cov, want), f"{op.name}: {int(cov.sum())} of {int(want.sum())} covered"
    if rounds > 1:  # no round to spare
        assert not torch.equal(E.coverage(op, side, rounds - 1), want)


@pytest.mark.parametrize("case,math,cls,side", PARAMS, ids=IDS)
def test_sensitivity(case, math, cls, side):
    op, _ = case.build()
    E.check_sensitivity(op, cls, side, case.seed, math)


@pytest.mark.parametrize("dy_dense", conv_cases.DB_SIDES, ids=["dy_sparse", "dy_dense"])
@pytest.mark.parametrize("shape,KS", conv_cases.DB_CASES)
@pytest.mark.parametrize("cls", [c for c, _ in conv_cases.DB_MODES])
def test_db_conditions(shape, KS, cls, dy_dense):
    """Which db cases test_wgrad_db_exact holds to fp64 bit for bit is decided by
    assert_exact_case (db_case); here, that the decision excludes no more than it must.
    db[co] sums N H W values of dy below 2 in magnitude, each a multiple of 2^-q: with
    2 N H W <= 2^(24-q) the conditions hold whatever the draw, so the case must be exact —
    every sparse case, every dense case of class 16x16, class 16x8 dense up to N H W = 256.
    Where it is not, the f32 summation bound asserted instead stays far below 1, the least
    that a dy value left out or added twice moves db by.  dW beside it is exact always."""
    op, dy, x, q, exact = conv_cases.db_case(shape, KS, cls, dy_dense)
    d = dy.double()
    s, a = d.sum((0, 2, 3)), d.abs().sum((0, 2, 3))
    n = d[:, 0].numel()
    assert q == E.CLASSES[cls][0 if dy_dense else 1]
    if dy_dense:
        assert bool((dy != 0).all())  # every (channel, pixel) pair is a term
    else:
        assert bool((dy != 0).any(0).any(-1).any(-1).all())  # every channel has a term
        assert exact
    if 2 * n <= 2 ** (24 - q):
        assert exact, f"db {shape} {cls}: excluded although 2 N H W = {2 * n} <= 2^{24 - q}"
    if cls == "16x16":
        assert exact
    if exact:
        E.assert_exact_case(s, a, q, f"db {shape}")
    else:
        assert float(a.max()) >= 2.0 ** (24 - q)  # condition 3 is what fails, nothing else
        assert float(E.f32_sum_bound(a, n).max()) < 2.0 ** -6
    E.assert_exact_case(op.ref(d, x.double()), op.ref(d.abs(), x.double().abs()), E.grain(cls),
                        f"dw beside db {shape}")


def test_hi_only_conditions():
    for M, N, K in [(1, 7, 3), (256, 256, 16)]:
        A, B = E.dense((M, K), "hi", 1, 0), E.dense((N, K), "hi", 2, 0)
        for t in (A, B):
            hi, mid, lo = E.split3(t)
            assert torch.equal(hi, t) and not bool(mid.any()) and not bool(lo.any())
        E.assert_exact_case(A.double() @ B.double().t(), A.double().abs() @ B.double().abs().t(),
                            E.grain("hi"), "hi-only")


def test_split_model_is_exact_and_ordered():
    """split3 reproduces the operand exactly on Gaussian data (the construction of
    _ref_pack), with |mid| <= 2^-7 |hi| and |lo| <= 2^-15 |hi|: hi is truncated, so the
    remainder is below one unit of its 8th bit, 2^-7 |hi|; mid and lo are rounded to nearest,
    so lo is at most half a unit of mid's 8th bit, 2^-8 of the remainder."""
    x = torch.randn(4096, generator=torch.Generator().manual_seed(0))
    hi, mid, lo = E.split3(x)
    assert torch.equal(hi.double() + mid.double() + lo.double(), x.double())
    assert bool((mid.abs() <= hi.abs() * 2.0 ** -7).all())
    assert bool((lo.abs() <= hi.abs() * 2.0 ** -15).all())


def _gaussian_bars(A, B, bad):
    """(normwise, elementwise / max) error of a modelled result against fp64."""
    ref = A.double() @ B.double().t()
    return (float((bad - ref).norm() / ref.norm()),
            float((bad - ref).abs().max() / ref.abs().max()))


def _shifted(A, plane, cols):
    """The six-product model of A B^T with one plane of A taken from k - 1 in the last
    `cols` columns (a plane staged from the wrong offset in a ragged K tail)."""
    def run(B):
        pa, pb = E.split3(A), E.split3(B)
        p = pa[plane].clone()
        p[:, -cols:] = pa[plane][:, -cols - 1:-1]
        pa[plane] = p
        return sum(pa[i].double() @ pb[j].double().t() for i, j in E.PRODUCTS)
    return run


def test_lo_shift_invisible_on_gaussian_visible_on_exact():
    """The gap these tests close, on the GEMM (37, 53, 300): the lo plane of A shifted by one
    k in the last 12 columns stays far inside the bf16x6 bars (1e-5 normwise, 1e-4
    elementwise) on the suite's Gaussian data, the same shift of the mid plane is caught
    only because 12 columns are hit; on exact data both change hundreds of outputs, and
    so does a dropped a2b0."""
    M, N, K = 37, 53, 300
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K + 11)
    A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    nrm, elt = _gaussian_bars(A, B, _shifted(A, 2, 12)(B))
    assert 0 < nrm < 1e-5 / 3 and 0 < elt < 1e-4 / 3, (nrm, elt)
    nrm, elt = _gaussian_bars(A, B, _shifted(A, 1, 12)(B))
    assert nrm > 1e-5, (nrm, elt)
    # exact data, class 24x8 with A dense: the union over the rounds the GPU test runs
    op = E.gemm_op(M, N, K)
    rounds = E.rounds_for(E.gemm_op, (M, N, K), 0)
    lo_bad = torch.zeros(M, N, dtype=torch.bool)
    drop_bad = torch.zeros(M, N, dtype=torch.bool)
    for rnd in range(rounds):
        Ae, Be = op.operands("24x8", 0, 5, rnd)
        ref = Ae.double() @ Be.double().t()
        assert torch.equal(E.model(op.ref, Ae, Be, 6), ref)
        lo_bad |= _shifted(Ae, 2, 12)(Be) != ref
        drop_bad |= E.model(op.ref, Ae, Be, 6, drop=(2, 0)) != ref
    # Each round's 53 x 8 pattern slots visit every k at least once, and the 8 entries of a
    # row lie 37 apart (mod 300), never two in one 12-column window: the 12 shifted columns
    # meet 12 different rows of B, each in all 37 outputs of its column of C.  An output
    # escapes only where lo[m, k] == lo[m, k - 1] (both zero, in 19 % of the elements each):
    # at least three quarters of 12 x 37 must differ.
    assert int(lo_bad.sum()) >= 12 * M * 3 // 4, int(lo_bad.sum())
    assert int(drop_bad.sum()) > M * N // 2, int(drop_bad.sum())
