"""Every plane of the split-bf16 GEMM kernels, bit for bit (gemm.hip: tlod_gemm_bs_f32 in its
four operand layouts, the _ex and _mask epilogues, the split-K slabs; tlod_gemm_nhwc3_bs_f32
modes 0 / 1 / 2; StridedConvFunction's im2col -> GEMM -> col2im).

The operands come from tests/exact_inputs.py: every term of every output is a multiple of one
grain and every sum fits 24 bits, so fp64, f32 and the kept plane products agree exactly and
the kernel's result must be torch.equal to the fp64 reference — no tolerance (torch.equal
takes -0.0 for +0.0: the sign of an exact zero is the one bit not pinned).  Each case runs
class 24x8 and 16x16 under bf16x6 and class 16x8 under bf16x3, each with either operand the
dense one, over as many rounds of shifted sparse patterns as cover every element of the
dense operand.  Class 16x16 under bf16x3 is the math-mode fidelity check: it must equal the
three-product model and differ from fp64 (the nprod argument reaches the kernel).
tests/test_exact_inputs_cpu.py proves the conditions for every case below without a GPU.
"""
import pytest
import torch

import exact_inputs as E

pytestmark = pytest.mark.gpu
dev = "cuda"

LAYOUTS = [(1, 1), (1, 0), (0, 0), (0, 1)]  # (a_kcontig, b_kcontig)
GEMM_SHAPES = [(37, 53, 300), (1, 7, 3), (37, 513, 17), (256, 256, 16), (5, 300, 64)]
# The smallest K whose tlod_gemm_bs_workspace_bytes > 0 at this one-tile M, N, found by
# asking the planner on the MI355X for every chunk count (K in 16-column chunks, kTK): under
# bf16x6 it splits from 6 chunks (K = 81, not at K = 80), under bf16x3, whose tile costs half
# as much, from 10 (K = 145, not at K = 144) — and from there on, so (37, 53, 300) above
# splits too.  81 and 145 also leave a ragged last chunk of one column in the last slab.
SPLIT_K6 = (37, 53, 81)    # bf16x6 alone
SPLIT_K = (37, 53, 145)    # both math modes
NHWC3_SHAPES = [(1, 4, 4, 256, 256), (3, 5, 7, 256, 48), (2, 1, 3, 512, 16)]  # R, H, W, C, O
SCONV = [(1, 20, 24, 17, 23, 5, 3, 2), (1, 20, 24, 17, 23, 3, 2, 1)]  # N Cin Cout H W KS stride pad


def _nhwc3_op(kind, R, H, W, C, O):
    return E.conv_op(kind, R, C, O, H, W)


def _sconv_op(kind, *key):
    return E.conv_op(kind, *key)


CASES = [E.Case("gemm", E.gemm_op, s, arg=l) for s in GEMM_SHAPES for l in LAYOUTS]
CASES += [E.Case("gemm", E.gemm_op, SPLIT_K, arg=l) for l in LAYOUTS]
CASES += [E.Case("gemm", E.gemm_op, SPLIT_K6, arg=l, modes=E.BS_MODES[:2]) for l in LAYOUTS]
CASES += [E.Case("gemm", E.gemm_op, s, epi=e, arg=(1, 1))
          for s in ((37, 53, 300), (37, 513, 17)) for e in ("b", "bra")]
CASES += [E.Case("gemm_mask", E.gemm_op, s, epi="rm", arg=(1, 0)) for s in ((37, 53, 300), SPLIT_K)]
for _s in NHWC3_SHAPES:
    CASES += [E.Case("nhwc3_0", _nhwc3_op, ("fwd",) + _s),
              E.Case("nhwc3_0", _nhwc3_op, ("fwd",) + _s, epi="bra"),
              E.Case("nhwc3_1", _nhwc3_op, ("dgrad",) + _s),
              E.Case("nhwc3_1", _nhwc3_op, ("dgrad",) + _s, epi="rm"),
              E.Case("nhwc3_2", _nhwc3_op, ("wgrad",) + _s, chan=0)]
# StridedConvFunction runs its GEMMs in bf16x6 only (no math argument)
CASES += [E.Case("sconv_" + k, _sconv_op, (k,) + s, modes=E.BS_MODES[:2])
          for s in SCONV for k in ("fwd", "dgrad", "wgrad")]

PARAMS, IDS = E.expand(CASES)


def _lay(t, kcontig):
    return t if kcontig else t.t().contiguous()


def _d(t):
    return None if t is None else t.to(dev)


def _rows(t):  # NCHW -> channels-last rows
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def _nchw(rows, shape):  # channels-last rows -> NCHW of `shape`
    n, c, h, w = shape
    return rows.view(n, h, w, c).permute(0, 3, 1, 2)


def run_gemm(case, A, B, epi, op, math):
    from tlod.linear import gemm
    (M, K), N = A.shape, B.shape[0]
    ak, bk = case.arg
    return gemm(_lay(A, ak).to(dev), _lay(B, bk).to(dev), M, N, K, ak, bk,
                _d(epi.bias) if epi else None, math, residual=_d(epi.residual) if epi else None,
                relu=bool(epi and epi.relu))


def run_gemm_mask(case, A, B, epi, op, math):
    from tlod.linear import gemm_mask
    (M, K), N = A.shape, B.shape[0]
    ak, bk = case.arg
    return gemm_mask(_lay(A, ak).to(dev), _lay(B, bk).to(dev), M, N, K, ak, bk, _d(epi.mask),
                     _d(epi.residual), math)


def run_nhwc3(mode):
    def run(case, A, B, epi, op, math):
        from tlod.linear import gemm_nhwc3
        _, R, H, W, C, O = case.key
        if mode == 0:  # A = x, B = w -> rows (R H W, O)
            wm = B.permute(0, 2, 3, 1).reshape(O, 9 * C)
            y = gemm_nhwc3(0, _rows(A).to(dev), wm.to(dev), R, H, W, C, O,
                           bias=_d(epi.bias) if epi else None,
                           residual=_d(_rows(epi.residual)) if epi else None,
                           relu=bool(epi and epi.relu), math=math)
            return _nchw(y.cpu(), op.out_shape)
        if mode == 1:  # A = dy, B = w -> rows (R H W, C), through the tap-flipped weight
            wm = B.permute(0, 2, 3, 1).reshape(O, 9 * C)
            wd = wm.view(O, 9, C).flip(1).transpose(0, 1).reshape(9 * O, C)
            dx = gemm_nhwc3(1, _rows(A).to(dev), wd.to(dev), R, H, W, C, O,
                            residual=_d(_rows(epi.residual)) if epi else None,
                            mask=_d(_rows(epi.mask)) if epi else None, math=math)
            return _nchw(dx.cpu(), op.out_shape)
        dw = gemm_nhwc3(2, _rows(A).to(dev), _rows(B).to(dev), R, H, W, C, O, math=math)
        return dw.cpu().view(O, 3, 3, C).permute(0, 3, 1, 2)  # (O, 9C) -> (O, C, 3, 3)
    return run


def run_sconv(kind):
    def run(case, A, B, epi, op, math):
        from tlod.conv import StridedConvFunction
        assert math == "bf16x6"
        _, N, Cin, Cout, H, W, KS, stride, pad = case.key
        if kind == "fwd":
            return StridedConvFunction.apply(A.to(dev), B.to(dev), None, stride, pad, False)
        # the backward's two GEMMs each read dy and one forward operand: the other forward
        # operand is zero (it does not enter that gradient)
        dy = A.to(dev)
        x = (torch.zeros(N, Cin, H, W) if kind == "dgrad" else B).to(dev).requires_grad_(True)
        w = (B if kind == "dgrad" else torch.zeros(Cout, Cin, KS, KS)).to(dev).requires_grad_(True)
        StridedConvFunction.apply(x, w, None, stride, pad, False).backward(dy)
        return x.grad if kind == "dgrad" else w.grad
    return run


RUN = {"gemm": run_gemm, "gemm_mask": run_gemm_mask, "nhwc3_0": run_nhwc3(0),
       "nhwc3_1": run_nhwc3(1), "nhwc3_2": run_nhwc3(2), "sconv_fwd": run_sconv("fwd"),
       "sconv_dgrad": run_sconv("dgrad"), "sconv_wgrad": run_sconv("wgrad")}


@pytest.mark.parametrize("math", ["bf16x6", "bf16x3"])
@pytest.mark.parametrize("M,N,K", [(1, 7, 3), (256, 256, 16)])
def test_exactness_model_hi_only(M, N, K, math):
    """The exactness model itself, on the smallest case: 8-bit operands (the hi planes alone,
    a0b0 the only nonzero product), both operands dense.  If this is not bit-exact the model
    (the bf16 MFMA keeps 24 bits relative to its largest addend) is wrong for the hardware,
    not the kernels."""
    from tlod.linear import gemm
    A = E.dense((M, K), "hi", 1, 0)
    B = E.dense((N, K), "hi", 2, 0)
    ref = A.double() @ B.double().t()
    E.assert_exact_case(ref, A.double().abs() @ B.double().abs().t(), E.grain("hi"), "hi-only")
    E.assert_bits(gemm(A.to(dev), B.to(dev), M, N, K, 1, 1, None, math), ref, E.grain("hi"),
                  f"hi-only gemm {(M, N, K)} {math}")


def test_split_k_shape_splits():
    """The deep-K cases take the split-K slab path (as test_gemm_split_k_deterministic asserts
    it): SPLIT_K in both math modes, SPLIT_K6 under bf16x6."""
    from tlod import _lib
    ws = _lib.lib().tlod_gemm_bs_workspace_bytes
    for ak, bk in LAYOUTS:
        assert ws(*SPLIT_K, ak, bk, 6) > 0 and ws(*SPLIT_K, ak, bk, 3) > 0
        assert ws(*SPLIT_K6, ak, bk, 6) > 0


@pytest.mark.parametrize("case,math,cls,side", PARAMS, ids=IDS)
def test_gemm_exact(case, math, cls, side):
    E.run_case(case, math, cls, side,
               lambda A, B, epi, op: RUN[case.path](case, A, B, epi, op, math))
