"""Every plane of the split-bf16 convolution kernels, bit for bit: the patch-staged and the
warp-specialised 3x3 forward / dgrad (conv.hip) with their split-K and stream-K tails, the
masked dgrad, the implicit-GEMM 3x3 and the 1x1 conv GEMM with its _ex epilogue (gemm.hip),
the weight gradients (wgrad_ws.hip for 3x3 under bf16x6, conv.hip otherwise), the fused
conv + ReLU + pool and the direct Cin <= 4 kernel.

The operands come from tests/exact_inputs.py: every term of every output is a multiple of one
grain and every sum fits 24 bits, so the kernel's result must be torch.equal to the fp64
F.conv2d / conv2d_input / conv2d_weight reference — no tolerance — whatever its tiling or
schedule (torch.equal takes -0.0 for +0.0: the sign of an exact zero is the one bit not
pinned).  Each case runs class 24x8 and 16x16 under bf16x6 and class 16x8 under bf16x3, each
with either operand the dense one (activations dense with weights sparse and the reverse; in
the weight gradient dy dense with x sparse and the reverse), over as many rounds of shifted
sparse patterns as cover every element of the dense operand.  Class 16x16 under bf16x3 is
the math-mode fidelity check: it must equal the three-product model and differ from fp64.
Where the dispatch has an f32 path, it runs as a control on class 24x8.
tests/test_exact_inputs_cpu.py proves the conditions for every case below without a GPU.
"""
import pytest
import torch
import torch.nn.functional as F

import exact_inputs as E

pytestmark = pytest.mark.gpu
dev = "cuda"

ALL = E.BS_MODES + E.F32_MODES
# N, Cin, Cout, H, W
PATCH = [(1, 13, 20, 9, 33), (2, 64, 72, 19, 37)]           # Cin < 128, ragged channels
WS = [(1, 128, 136, 5, 40), (1, 144, 128, 61, 9), (1, 128, 128, 2, 70)]  # Cin >= 128
# split-K / stream-K tails; Cin = 520 is 65 chunks of 8 channels, an odd count
TAILS = [(1, 512, 512, 12, 20), (1, 520, 64, 5, 7)]
# dgrad reduces over Cout: the odd chunk count in dgrad needs Cout = 520 (dgrad only)
TAILS_DGRAD = [(1, 64, 520, 5, 7)]
GEMM3 = [(3, 257, 256, 5, 7), (1, 256, 260, 3, 3), (1, 16, 256, 40, 2)]
ONE = [(3, 96, 80, 9, 33), (1, 72, 257, 5, 7), (2, 130, 200, 1, 3), (2, 512, 18, 5, 7)]
# (1, 136, 40, 5, 9): a second Cin >= 128 shape for wgrad_ws.hip, ragged in both channel counts
WGRAD = [(2, 32, 64, 5, 7), (1, 16, 32, 1, 40), (1, 16, 32, 40, 1), (3, 8, 36, 3, 3),
         (1, 130, 132, 9, 33), (1, 136, 40, 5, 9)]
POOL = [(1, 64, 128, 33, 31), (2, 3, 64, 8, 10)]
DIRECT = [(2, 3, 64, 8, 10), (1, 4, 20, 9, 8)]
# Cout = 18 goes to the 1x1 GEMM only while TLOD_CONV1X1_MIN <= 18.  16 is also the default
# (tlod/conv.py), so the variable changes no routing today: it keeps this one shape on the
# GEMM should the default move (run_fwd1 / run_dgrad1 assert the routing either way).
MIN16 = {(2, 512, 18, 5, 7): {"TLOD_CONV1X1_MIN": "16"}}


def _op1(kind, *key):
    return E.conv_op(kind, *key, KS=1)


def _pool(v):
    return F.max_pool2d(v, 2, 2)


CASES = []
for _s in PATCH + WS + TAILS:
    CASES += [E.Case("fwd3", E.conv_op, ("fwd",) + _s, modes=ALL),
              E.Case("dgrad3", E.conv_op, ("dgrad",) + _s, modes=ALL)]
# the full epilogue (scale 2^k, bias, residual, ReLU) and the masked dgrad
CASES += [E.Case("fwd3", E.conv_op, ("fwd",) + s, epi="sbra") for s in PATCH + WS[:1] + TAILS[:1]]
CASES += [E.Case("dgrad3", E.conv_op, ("dgrad",) + s, epi="m") for s in PATCH[:1] + WS[:1]]
for _s in GEMM3:
    CASES += [E.Case("gemm3_fwd", E.conv_op, ("fwd",) + _s),
              E.Case("gemm3_fwd", E.conv_op, ("fwd",) + _s, epi="sbra")]
    if _s[1] >= 256:  # as test_conv_gemm_fwd_dgrad: the GEMM takes >= 256 output rows
        CASES += [E.Case("gemm3_dgrad", E.conv_op, ("dgrad",) + _s)]
CASES += [E.Case("dgrad3", E.conv_op, ("dgrad",) + s, modes=ALL) for s in TAILS_DGRAD]
for _s in ONE:
    _env = MIN16.get(_s)
    CASES += [E.Case("fwd1", _op1, ("fwd",) + _s, modes=ALL, env=_env),
              E.Case("fwd1", _op1, ("fwd",) + _s, epi="sbra", env=_env),
              E.Case("dgrad1", _op1, ("dgrad",) + _s, modes=ALL, env=_env),
              E.Case("dgrad1", _op1, ("dgrad",) + _s, epi="rm", wscale=True, env=_env)]
for _s in WGRAD:
    for _ks in (3, 1):
        _mk = E.conv_op if _ks == 3 else _op1
        CASES += [E.Case("wgrad", _mk, ("wgrad",) + _s, chan=0, modes=ALL, arg=_ks),
                  # accumulate=True onto a base, with row_scale = 2^k: base + s * dW
                  E.Case("wgrad", _mk, ("wgrad",) + _s, epi="sr", chan=0, arg=_ks)]
CASES += [E.Case("pool", E.conv_op, ("fwd",) + s, epi="ba", post=_pool, modes=ALL) for s in POOL]
CASES += [E.Case("direct", E.conv_op, ("fwd",) + s, epi=e,
                 modes=(("f32", "24x8"), ("f32", "16x16"), ("f32", "16x8")))
          for s in DIRECT for e in ("b", "ba")]

PARAMS, IDS = E.expand(CASES)


def _d(t):
    return None if t is None else t.to(dev)


def _epi(epi):
    if epi is None:
        return dict(bias=None, relu=False, scale=None, residual=None)
    return dict(bias=_d(epi.bias), relu=epi.relu, scale=_d(epi.scale), residual=_d(epi.residual))


def _takes_split_k(case, math):
    """The planner assertion of test_conv_split_k_paths, for the TAILS shapes: the workspace
    query that tlod.conv makes for this call (the split-bf16 dgrad runs the forward kernel
    on the transposed pack, so it asks the forward query with the channel counts swapped)."""
    from tlod import _lib
    kind, N, Cin, Cout, H, W = case.key
    L = _lib.lib()
    if math == "f32":
        if kind == "fwd":
            return L.tlod_conv_fwd_workspace_bytes(N, Cin, H, W, Cout, 3) > 0
        return L.tlod_conv_dgrad_workspace_bytes(N, Cin, H, W, Cout, 3) > 0
    cin, cout = (Cin, Cout) if kind == "fwd" else (Cout, Cin)
    nprod = 6 if math == "bf16x6" else 3
    return L.tlod_conv_fwd_bs_workspace_bytes(N, cin, H, W, cout, 3, nprod) > 0


def run_fwd3(case, A, B, epi, op, math):
    from tlod.conv import _gemm_conv, conv_fwd
    assert not _gemm_conv(3, math, B.shape[0])
    if case.key[1:] in TAILS:
        assert _takes_split_k(case, math)
    return conv_fwd(A.to(dev), B.to(dev), math=math, **_epi(epi))


def run_dgrad3(case, A, B, epi, op, math):
    import tlod.conv as tc
    assert not tc._gemm_conv(3, math, B.shape[1])
    if case.key[1:] in TAILS + TAILS_DGRAD:
        assert _takes_split_k(case, math)
    if epi is None:
        return tc.conv_dgrad(A.to(dev), B.to(dev), math=math)
    before = tc.STATS["masked_dgrad"]
    dx = tc.conv_dgrad(A.to(dev), B.to(dev), math=math, mask=_d(epi.mask))
    assert tc.STATS["masked_dgrad"] == before + 1  # tlod_conv_dgrad_bs_mask_f32 ran
    return dx


def run_gemm3_fwd(case, A, B, epi, op, math):
    from tlod.conv import _conv_gemm
    e = _epi(epi)
    return _conv_gemm(A.to(dev), B.to(dev), 0, e["bias"], e["relu"], e["scale"], e["residual"],
                      B.shape[0], math, "fwd")


def run_gemm3_dgrad(case, A, B, epi, op, math):
    from tlod.conv import _conv_gemm, pack_dgrad
    return _conv_gemm(A.to(dev), pack_dgrad(B.to(dev)), 1, None, False, None, None, B.shape[1],
                      math, "dgrad")


def run_fwd1(case, A, B, epi, op, math):
    from tlod.conv import _gemm1x1, conv_fwd
    assert math == "f32" or _gemm1x1(1, math, B.shape[1], B.shape[0])
    return conv_fwd(A.to(dev), B.to(dev), math=math, **_epi(epi))


def run_dgrad1(case, A, B, epi, op, math):
    import tlod.conv as tc
    assert math == "f32" or tc._gemm1x1(1, math, B.shape[0], B.shape[1])
    if epi is None:
        return tc.conv_dgrad(A.to(dev), B.to(dev), math=math)
    # tlod_conv1x1_gemm_bs_ex_f32: (dgrad through w * wscale + residual) * (mask > 0)
    before = tc.STATS["masked_dgrad"]
    dx = tc.conv_dgrad(A.to(dev), B.to(dev), math=math, mask=_d(epi.mask),
                       residual=_d(epi.residual), wscale=_d(case.wscale(op)))
    assert tc.STATS["masked_dgrad"] == before + 1
    return dx


def run_wgrad(case, A, B, epi, op, math):
    from tlod.conv import conv_wgrad
    KS = case.arg
    if epi is None:
        return conv_wgrad(A.to(dev), B.to(dev), KS, math=math)
    out = epi.residual.clone().to(dev)
    got = conv_wgrad(A.to(dev), B.to(dev), KS, out=out, accumulate=True, math=math,
                     row_scale=_d(epi.scale))
    assert got.data_ptr() == out.data_ptr()
    return got


def run_pool(case, A, B, epi, op, math):
    from tlod.conv import conv_fwd_pool
    return conv_fwd_pool(A.to(dev), B.to(dev), _d(epi.bias), math=math)


def run_direct(case, A, B, epi, op, math):
    from tlod.conv import conv_fwd
    assert A.shape[1] <= 4  # tlod_conv3x3_direct_f32, whatever the math mode
    return conv_fwd(A.to(dev), B.to(dev), _d(epi.bias), relu=epi.relu)


RUN = {"fwd3": run_fwd3, "dgrad3": run_dgrad3, "gemm3_fwd": run_gemm3_fwd,
       "gemm3_dgrad": run_gemm3_dgrad, "fwd1": run_fwd1, "dgrad1": run_dgrad1,
       "wgrad": run_wgrad, "pool": run_pool, "direct": run_direct}


@pytest.mark.parametrize("case,math,cls,side", PARAMS, ids=IDS)
def test_conv_exact(case, math, cls, side, monkeypatch):
    """Paths by case id: fwd3 / dgrad3 the patch-staged kernel (Cin < 128), the
    warp-specialised one (Cin >= 128) and their split-K tails (workspace > 0 asserted), `-m`
    the masked dgrad; gemm3_* the implicit-GEMM 3x3; fwd1 / dgrad1 the 1x1 conv GEMM
    (`-rm-wscale`: its _ex form); wgrad-..-3 / -1 the weight gradients; pool the fused
    conv + ReLU + pool — at (2, 3, 64, 8, 10) still the split-bf16 pool kernel on one ragged
    channel chunk: conv_fwd_pool has no direct-kernel route, so the direct Cin <= 4 kernel
    runs as its own `direct` cases through conv_fwd."""
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    E.run_case(case, math, cls, side,
               lambda A, B, epi, op: RUN[case.path](case, A, B, epi, op, math))


DB_CASES = [(s, ks) for s in WGRAD for ks in (3, 1)]


DB_MODES = [("24x8", "bf16x6"), ("16x16", "bf16x6"), ("16x8", "bf16x3")]
DB_SIDES = [False, True]  # dy sparse (8 pixels per channel) with x dense, and dy dense


def db_case(shape, KS, cls, dy_dense):
    """The bias-gradient check: (op, dy, x, q, exact).  db[co] = sum over n, h, w of dy is a
    plain f32 sum of the staged dy values — no planes, no partner — so its grain is dy's own,
    2^-q with q the Q of dy's side of the class, and its sum |terms| is sum |dy|.  exact:
    whether conditions 2 and 3 hold for it, decided by assert_exact_case itself
    (E.is_exact_case), not by a list."""
    op = (E.conv_op if KS == 3 else _op1)("wgrad", *shape)
    dy, x = op.operands(cls, 0 if dy_dense else 1, 77, 0)
    q = E.CLASSES[cls][0 if dy_dense else 1]
    d = dy.double()
    return op, dy, x, q, E.is_exact_case(d.sum((0, 2, 3)), d.abs().sum((0, 2, 3)), q)


@pytest.mark.parametrize("dy_dense", DB_SIDES, ids=["dy_sparse", "dy_dense"])
@pytest.mark.parametrize("cls,math", DB_MODES)
@pytest.mark.parametrize("shape,KS", DB_CASES)
def test_wgrad_db_exact(shape, KS, cls, math, dy_dense):
    """db from the weight-gradient launch, in both directions.  With dy sparse it has at most
    8 terms per channel; with dy dense every (channel, pixel) pair of dy is a term, rows past
    Cout and ragged pixel-tile tails included.  Wherever conditions 2 and 3 hold (db_case)
    it must equal fp64 bit for bit: every sparse case, every dense case of class 16x16
    (10-bit values, sum |dy| < 2 N H W <= 594 < 2^15) and of class 16x8 (16-bit values) up
    to sum |dy| < 2^9; tests/test_exact_inputs_cpu.py::test_db_conditions asserts which.

    Inexact by design, and only there: dy dense in class 24x8 (20-bit values, sum |dy| >=
    N H W >= 27 while condition 3 needs < 2^5), and in class 16x8 where sum |dy| reaches 2^9
    (of these shapes (1, 130, 132, 9, 33) alone, N H W = 297).  The lines that make it so:
    `rs[i] += t` (wgws_produce in wgrad_ws.hip, conv_wgrad_bs_kernel in conv.hip) adds the
    staged f32 values, the `__shfl_xor` lines after the chunk loop add the 8 (4) lanes of a
    row, and the loop of db_reduce_kernel (conv.hip) adds the splits, each addition rounded
    to 24 bits.  What is true of such a sum in any order, and asserted: it is a
    multiple of dy's grain and lies within N H W 2^-24 sum |dy| of fp64 (E.assert_f32_sum) —
    below 1.1e-2 here, while a dy value left out or added twice moves db by at least 1 (no
    planes enter db, so there is no smaller mistake of staging to see).  dW from the same
    launch is exact in every case."""
    from tlod.conv import conv_wgrad
    op, dy, x, q, exact = db_case(shape, KS, cls, dy_dense)
    db = torch.full((shape[2],), float("nan"), device=dev)
    dw = conv_wgrad(dy.to(dev), x.to(dev), KS, math=math, db=db)
    d = dy.double()
    what = f"db {shape} KS={KS} {cls} dy {'dense' if dy_dense else 'sparse'}"
    if exact:
        E.assert_bits(db, d.sum((0, 2, 3)), q, what)
    else:
        assert dy_dense and cls != "16x16"
        E.assert_f32_sum(db, d.sum((0, 2, 3)), d.abs().sum((0, 2, 3)), d[:, 0].numel(), q, what)
    E.assert_bits(dw, op.ref(d, x.double()), E.grain(cls), f"dw beside {what}")
