"""Where the kernels write: every C ABI entry point (include/tlod.h) called on raw pointers
into guarded buffers (tests/abi_guard.py) — poisoned outputs, exact-size workspaces, inputs
compared bit for bit afterwards — and then judged against its family's existing reference at
that family's existing bar (_close / oracle functions imported from the family's test module;
no tolerance is introduced here, integer outputs are bit-exact).

A  workspace-bearing entry points run with exactly *_workspace_bytes of guarded scratch
   (NULL, 0 when the query says 0); the conv / GEMM planners under tlod_set_cu_reserve of 0,
   37 and 248 (about eight CUs of slots: small maps take the whole-rounds-plus-split-tail
   plans), query and launch under the same reserve;
B  the same call with ws_bytes = query - 1 (the memory is still all there) must return
   TLOD_EWORKSPACE and leave every output pure poison;
C  ACCUMULATE contracts: prefilled with finite random P, the result is P + the oracle
   gradient at the family's bar and bit-equal to P wherever the oracle gradient is exactly 0;
D  full-write / zero-fill / padding contracts of entry points without a workspace.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_conv_bs_gpu as tcb
import test_conv_gpu as tcg
import test_conv_small_gpu as tcs
import test_linear_gpu as tlg
import test_losses_gpu as tlo
import test_ops_gpu as top
import test_rpn_gpu as trp
from abi_guard import TLOD_EWORKSPACE, Call
from oracle import nms as onms
from oracle import roi as oroi
from oracle import rpn as orpn

pytestmark = pytest.mark.gpu
f32, i32, i64, u8 = torch.float32, torch.int32, torch.int64, torch.uint8


def lib():
    from tlod import _lib
    return _lib.lib()


def _ok(st, what=""):
    assert st == 0, (what, st, lib().tlod_last_error().decode(errors="replace"))


def _same(ref):
    """verify: the output equals ref bit for bit."""
    def verify(o):
        assert torch.equal(o.payload.cpu(), ref)
    return verify


def _ws(c, q, over):
    """(ws pointer, ws_bytes) of an exact-size guarded workspace; over: the ws_bytes to claim
    instead (case B: the buffer itself stays full size)."""
    ws = c.ws(q)
    return (ws.ptr if ws is not None else None), (q if over is None else over)


def guard_case(launch, verify=None):
    """launch(c, over) builds the call's buffers in c, queries the workspace, makes the call
    and returns (status, query, outputs).  Case A (+ C / D through verify), then case B."""
    c = Call()
    st, q, outs = launch(c, None)
    _ok(st, launch.__name__)
    c.check()
    if verify is not None:
        # a verify asserts; one that hands back a comparison's verdict (torch.equal, a mask)
        # checked nothing.  (The families' _close return the error they asserted on.)
        verdict = verify(outs)
        assert not isinstance(verdict, (bool, torch.Tensor, np.ndarray, np.bool_)), \
            f"{launch.__name__}: verify returned {verdict!r} instead of asserting"
    if q > 0:
        c2 = Call()
        st2, q2, _ = launch(c2, q - 1)
        assert q2 == q
        assert st2 == TLOD_EWORKSPACE, (launch.__name__, st2, q)
        c2.check_rejected()
    return q


@pytest.fixture(params=[0, 37, 248])
def reserve(request):
    from tlod import _lib
    _lib.check(lib().tlod_set_cu_reserve(request.param), "set_cu_reserve")
    yield request.param
    _lib.check(lib().tlod_set_cu_reserve(0), "set_cu_reserve")


# ===================================================================== convolutions
# the ragged shapes the suite already trusts, one that splits (asserted > 0 below and on the
# CPU build) and one large map of few channels that does not (asserted == 0)
CONV_SHAPES = [(1, 130, 132, 9, 33), (3, 8, 36, 3, 3), (1, 72, 257, 5, 7), (1, 512, 512, 12, 20),
               (1, 16, 16, 150, 250)]  # N, Cin, Cout, H, W
SPLIT, NOSPLIT = (1, 512, 512, 12, 20), (1, 16, 16, 150, 250)


@functools.lru_cache(maxsize=None)
def conv_data(N, Cin, Cout, H, W, KS):
    """Inputs and fp64 references of one conv shape, computed once and shared (read only)."""
    g = torch.Generator().manual_seed(N * 1000 + Cin + Cout + H + 7 * KS)
    KK, pad = KS * KS, KS // 2
    d = dict(N=N, Cin=Cin, Cout=Cout, H=H, W=W, KS=KS)
    d["x"] = torch.randn(N, Cin, H, W, generator=g)
    d["w"] = torch.randn(Cout, Cin, KS, KS, generator=g) * (2.0 / (Cin * KK)) ** 0.5
    d["b"] = torch.randn(Cout, generator=g)
    d["sc"] = torch.rand(Cout, generator=g) + 0.5
    d["res"] = torch.randn(N, Cout, H, W, generator=g)
    d["gy"] = torch.randn(N, Cout, H, W, generator=g)
    d["mask"] = torch.relu(torch.randn(N, Cin, H, W, generator=g))
    d["res_in"] = torch.randn(N, Cin, H, W, generator=g)
    d["rs"] = torch.rand(Cout, generator=g) + 0.5
    d["P_dw"] = torch.randn(Cout, Cin, KS, KS, generator=g)
    d["P_db"] = torch.randn(Cout, generator=g)
    x64, w64, gy64 = d["x"].double(), d["w"].double(), d["gy"].double()
    d["y"] = F.conv2d(x64, w64, padding=pad)
    d["dx"] = torch.nn.grad.conv2d_input(d["x"].shape, w64, gy64, padding=pad)
    d["dw"] = torch.nn.grad.conv2d_weight(x64, d["w"].shape, gy64, padding=pad)
    d["db"] = gy64.sum((0, 2, 3))
    # the f32 packs (include/tlod.h): wk[(ci*KK + s)][co] = w[co][ci][s],
    # wd[(co*KK + s)][ci] = w[co][ci][KK-1-s]
    d["wk"] = d["w"].reshape(Cout, Cin * KK).t().contiguous()
    d["wd"] = d["w"].reshape(Cout, Cin, KK).flip(2).permute(0, 2, 1).reshape(Cout * KK, Cin) \
        .contiguous()
    if KS == 3:  # the split-bf16 planes, built with torch ops (bit-exact: test_pack_bs_bit_exact)
        d["wp_fwd"] = tcb._ref_pack(d["w"], False)
        d["wp_dgrad"] = tcb._ref_pack(d["w"], True)
    return d


def _epi_ref(d):
    ch = (1, -1, 1, 1)
    return torch.relu(d["y"] * d["sc"].double().view(ch) + d["b"].double().view(ch)
                      + d["res"].double())


def _relu_close(close, y, ref, *a):
    # as the family's tests do: a mask flip at f32 rounding of 0 does not count
    close(y * (ref > 0).to(y.device), ref, *a)


def op_fwd_f32(d, ex):
    N, Cin, Cout, H, W, KS = (d[k] for k in ("N", "Cin", "Cout", "H", "W", "KS"))
    L = lib()

    def launch(c, over):
        q = L.tlod_conv_fwd_workspace_bytes(N, Cin, H, W, Cout, KS)
        x, wk, b = c.inp(d["x"], "x"), c.inp(d["wk"], "wk"), c.inp(d["b"], "bias")
        y = c.out((N, Cout, H, W), f32, "y")
        if ex:
            sc, res = c.inp(d["sc"], "scale"), c.inp(d["res"], "residual")
            st = c.run(L.tlod_conv_fwd_ex_f32, x, wk, sc, b, res, y, N, Cin, H, W, Cout, KS, 1,
                       *_ws(c, q, over))
        else:
            st = c.run(L.tlod_conv_fwd_f32, x, wk, b, y, N, Cin, H, W, Cout, KS, 0,
                       *_ws(c, q, over))
        return st, q, y

    def verify(y):
        if ex:
            _relu_close(tcg._close, y.payload, _epi_ref(d))
        else:
            tcg._close(y.payload, d["y"] + d["b"].double().view(1, -1, 1, 1))
    return launch, verify


def op_dgrad_f32(d):
    N, Cin, Cout, H, W, KS = (d[k] for k in ("N", "Cin", "Cout", "H", "W", "KS"))
    L = lib()

    def launch(c, over):
        q = L.tlod_conv_dgrad_workspace_bytes(N, Cin, H, W, Cout, KS)
        gy, wd = c.inp(d["gy"], "dy"), c.inp(d["wd"], "wd")
        dx = c.out((N, Cin, H, W), f32, "dx")
        st = c.run(L.tlod_conv_dgrad_f32, gy, wd, dx, N, Cin, H, W, Cout, KS, *_ws(c, q, over))
        return st, q, dx
    return launch, lambda dx: tcg._close(dx.payload, d["dx"])


def _acc_verify(close, got, P, ref, *a):
    """got = P + ref at the family's bar; (case C) bit-equal to P where ref is exactly 0."""
    close(got, P.double() + ref, *a)
    zero = (ref == 0)
    if bool(zero.any()):
        assert torch.equal(got.cpu()[zero], P[zero])


def op_wgrad_f32(d, accumulate):
    N, Cin, Cout, H, W, KS = (d[k] for k in ("N", "Cin", "Cout", "H", "W", "KS"))
    L = lib()

    def launch(c, over):
        q = L.tlod_conv_wgrad_workspace_bytes(N, Cin, H, W, Cout, KS)
        gy, x = c.inp(d["gy"], "dy"), c.inp(d["x"], "x")
        dw = c.acc(d["P_dw"], "dw") if accumulate else c.out(d["w"].shape, f32, "dw")
        st = c.run(L.tlod_conv_wgrad_f32, gy, x, dw, accumulate, N, Cin, H, W, Cout, KS,
                   *_ws(c, q, over))
        return st, q, dw

    def verify(dw):
        if accumulate:
            _acc_verify(tcg._close, dw.payload, d["P_dw"], d["dw"])
        else:
            tcg._close(dw.payload, d["dw"])
    return launch, verify


def op_fwd_bs(d, nprod):
    N, Cin, Cout, H, W = (d[k] for k in ("N", "Cin", "Cout", "H", "W"))
    L, math = lib(), "bf16x6" if nprod == 6 else "bf16x3"

    def launch(c, over):
        q = L.tlod_conv_fwd_bs_workspace_bytes(N, Cin, H, W, Cout, 3, nprod)
        x, wp = c.inp(d["x"], "x"), c.inp(d["wp_fwd"], "wp")
        sc, b, res = c.inp(d["sc"], "scale"), c.inp(d["b"], "bias"), c.inp(d["res"], "residual")
        y = c.out((N, Cout, H, W), f32, "y")
        st = c.run(L.tlod_conv_fwd_bs_f32, x, wp, sc, b, res, y, N, Cin, H, W, Cout, 3, 1, nprod,
                   *_ws(c, q, over))
        return st, q, y
    return launch, lambda y: _relu_close(tcb._close, y.payload, _epi_ref(d), math)


def op_dgrad_bs_mask(d, nprod):
    N, Cin, Cout, H, W = (d[k] for k in ("N", "Cin", "Cout", "H", "W"))
    L, math = lib(), "bf16x6" if nprod == 6 else "bf16x3"

    def launch(c, over):
        # the dgrad form: Cin := the layer's Cout, Cout := the layer's Cin
        q = L.tlod_conv_fwd_bs_workspace_bytes(N, Cout, H, W, Cin, 3, nprod)
        gy, wp, m = c.inp(d["gy"], "dy"), c.inp(d["wp_dgrad"], "wp"), c.inp(d["mask"], "mask")
        dx = c.out((N, Cin, H, W), f32, "dx")
        st = c.run(L.tlod_conv_dgrad_bs_mask_f32, gy, wp, m, dx, N, Cout, H, W, Cin, nprod,
                   *_ws(c, q, over))
        return st, q, dx
    return launch, lambda dx: tcb._close(dx.payload, d["dx"] * (d["mask"] > 0), math)


def op_wgrad_bs(d, nprod, accumulate, ex):
    N, Cin, Cout, H, W, KS = (d[k] for k in ("N", "Cin", "Cout", "H", "W", "KS"))
    L, math = lib(), "bf16x6" if nprod == 6 else "bf16x3"

    def launch(c, over):
        q = L.tlod_conv_wgrad_bs_workspace_bytes(N, Cin, H, W, Cout, KS, nprod)
        gy, x = c.inp(d["gy"], "dy"), c.inp(d["x"], "x")
        if accumulate:
            dw, db = c.acc(d["P_dw"], "dw"), c.acc(d["P_db"], "db")
        else:
            dw, db = c.out(d["w"].shape, f32, "dw"), c.out((Cout,), f32, "db")
        if ex:
            rs = c.inp(d["rs"], "row_scale")
            st = c.run(L.tlod_conv_wgrad_bs_ex_f32, gy, x, dw, db, accumulate, rs, N, Cin, H, W,
                       Cout, KS, nprod, *_ws(c, q, over))
        else:
            st = c.run(L.tlod_conv_wgrad_bs_f32, gy, x, dw, db, accumulate, N, Cin, H, W, Cout,
                       KS, nprod, *_ws(c, q, over))
        return st, q, (dw, db)

    def verify(outs):
        dw, db = outs
        ref = d["dw"] * d["rs"].double().view(-1, 1, 1, 1) if ex else d["dw"]
        if accumulate:
            _acc_verify(tcb._close, dw.payload, d["P_dw"], ref, math)
            _acc_verify(tcb._close, db.payload, d["P_db"], d["db"], "bf16x6")
        else:
            tcb._close(dw.payload, ref, math)
            tcb._close(db.payload, d["db"], "bf16x6")  # f32 row sums (test_conv_bs_wgrad)
    return launch, verify


def op_conv_gemm(d, w_layout, ex=False):
    """tlod_conv3x3_gemm_bs_f32 / tlod_conv1x1_gemm_bs_f32 (KS of the data) and, ex, the 1x1
    tlod_conv1x1_gemm_bs_ex_f32 with mask (+ w_scale in the dgrad layout)."""
    N, Cin, Cout, H, W, KS = (d[k] for k in ("N", "Cin", "Cout", "H", "W", "KS"))
    L = lib()
    qf, fn = ((L.tlod_conv3x3_gemm_bs_workspace_bytes, L.tlod_conv3x3_gemm_bs_f32) if KS == 3
              else (L.tlod_conv1x1_gemm_bs_workspace_bytes, L.tlod_conv1x1_gemm_bs_f32))

    def launch(c, over):
        if w_layout == 0:
            q = qf(N, Cin, H, W, Cout, 0, 6)
            x, w = c.inp(d["x"], "x"), c.inp(d["w"], "w")
            sc, b, res = c.inp(d["sc"], "scale"), c.inp(d["b"], "bias"), c.inp(d["res"], "res")
            y = c.out((N, Cout, H, W), f32, "y")
            if ex:
                m = c.inp(torch.relu(d["gy"]), "mask")
                st = c.run(L.tlod_conv1x1_gemm_bs_ex_f32, x, w, 0, sc, b, res, m, None, y, N, Cin,
                           H, W, Cout, 1, 6, *_ws(c, q, over))
            else:
                st = c.run(fn, x, w, 0, sc, b, res, y, N, Cin, H, W, Cout, 1, 6, *_ws(c, q, over))
            return st, q, y
        # the input gradient: x = dy, Cin := the layer's Cout, Cout := the layer's Cin
        q = qf(N, Cout, H, W, Cin, 1, 6)
        gy = c.inp(d["gy"], "dy")
        w = c.inp(d["wd"] if KS == 3 else d["w"], "w")
        dx = c.out((N, Cin, H, W), f32, "dx")
        if ex:
            res, m, ws_ = c.inp(d["res_in"], "res"), c.inp(d["mask"], "mask"), c.inp(d["rs"], "ws")
            st = c.run(L.tlod_conv1x1_gemm_bs_ex_f32, gy, w, 1, None, None, res, m, ws_, dx, N,
                       Cout, H, W, Cin, 0, 6, *_ws(c, q, over))
        else:
            st = c.run(fn, gy, w, 1, None, None, None, dx, N, Cout, H, W, Cin, 0, 6,
                       *_ws(c, q, over))
        return st, q, dx

    def verify(o):
        if w_layout == 0:
            ref = _epi_ref(d)
            if ex:
                ref = ref * (d["gy"] > 0)
            _relu_close(tcb._close, o.payload, ref, "bf16x6")
        elif ex:
            w64 = d["w"].double() * d["rs"].double().view(-1, 1, 1, 1)
            ref = torch.nn.grad.conv2d_input(d["x"].shape, w64, d["gy"].double())
            tcb._close(o.payload, (ref + d["res_in"].double()) * (d["mask"] > 0), "bf16x6")
        else:
            tcb._close(o.payload, d["dx"], "bf16x6")
    return launch, verify


def op_drm_fwd(d, s=2):
    N, Cin, Cout, H, W = (d[k] for k in ("N", "Cin", "Cout", "H", "W"))
    L = lib()
    Ho, Wo = H // s, W // s

    def launch(c, over):
        q = L.tlod_conv_fwd_workspace_bytes(N, Cin, H, W, Cout, 1)
        x, wk = c.inp(d["x"], "x"), c.inp(d["wk"], "wk")
        y = c.out((N, Cout * s * s, Ho, Wo), f32, "y")
        st = c.run(L.tlod_drm_fwd_f32, x, wk, y, N, Cin, H, W, Cout, s, *_ws(c, q, over))
        return st, q, y

    def verify(y):
        ref = F.pixel_unshuffle(torch.relu(d["y"])[:, :, :Ho * s, :Wo * s], s)
        _relu_close(tcg._close, y.payload, ref)
    return launch, verify


CONV3_OPS = {
    "fwd_f32": lambda d: op_fwd_f32(d, False), "fwd_ex_f32": lambda d: op_fwd_f32(d, True),
    "dgrad_f32": op_dgrad_f32,
    "wgrad_f32": lambda d: op_wgrad_f32(d, 0), "wgrad_f32_acc": lambda d: op_wgrad_f32(d, 1),
    "fwd_bs6": lambda d: op_fwd_bs(d, 6), "fwd_bs3": lambda d: op_fwd_bs(d, 3),
    "dgrad_bs_mask6": lambda d: op_dgrad_bs_mask(d, 6),
    "dgrad_bs_mask3": lambda d: op_dgrad_bs_mask(d, 3),
    # nprod = 6 at KS = 3: the warp-specialized wgrad_ws kernel; nprod = 3: the slab kernel
    "wgrad_bs6": lambda d: op_wgrad_bs(d, 6, 0, False),
    "wgrad_bs3": lambda d: op_wgrad_bs(d, 3, 0, False),
    "wgrad_bs6_acc": lambda d: op_wgrad_bs(d, 6, 1, False),
    "wgrad_bs3_acc": lambda d: op_wgrad_bs(d, 3, 1, False),
    "wgrad_bs_ex6": lambda d: op_wgrad_bs(d, 6, 0, True),
    "wgrad_bs_ex3_acc": lambda d: op_wgrad_bs(d, 3, 1, True),
    "conv3x3_gemm_w0": lambda d: op_conv_gemm(d, 0),
    "conv3x3_gemm_w1": lambda d: op_conv_gemm(d, 1),
}
CONV1_OPS = {
    "fwd_f32": lambda d: op_fwd_f32(d, False), "fwd_ex_f32": lambda d: op_fwd_f32(d, True),
    "dgrad_f32": op_dgrad_f32,
    "wgrad_f32": lambda d: op_wgrad_f32(d, 0), "wgrad_f32_acc": lambda d: op_wgrad_f32(d, 1),
    "wgrad_bs6": lambda d: op_wgrad_bs(d, 6, 0, False),
    "wgrad_bs_ex6_acc": lambda d: op_wgrad_bs(d, 6, 1, True),
    "conv1x1_gemm_w0": lambda d: op_conv_gemm(d, 0),
    "conv1x1_gemm_w1": lambda d: op_conv_gemm(d, 1),
    "conv1x1_gemm_ex_w0": lambda d: op_conv_gemm(d, 0, True),
    "conv1x1_gemm_ex_w1": lambda d: op_conv_gemm(d, 1, True),
    "drm_fwd": op_drm_fwd,
}


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("op", sorted(CONV3_OPS))
def test_conv3x3(reserve, op, shape):
    guard_case(*CONV3_OPS[op](conv_data(*shape, 3)))


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("op", sorted(CONV1_OPS))
def test_conv1x1(reserve, op, shape):
    guard_case(*CONV1_OPS[op](conv_data(*shape, 1)))


def planner_queries(L):
    """(split, nosplit): workspace queries that must be > 0 / == 0 with no CUs reserved (the
    CPU build assumes 256 slots: tests/test_abi_guard_cpu.py asserts the same lists there)."""
    N, Ci, Co, H, W = SPLIT
    n, ci, co, h, w = NOSPLIT
    split = {
        "conv_fwd": L.tlod_conv_fwd_workspace_bytes(N, Ci, H, W, Co, 3),
        "conv_dgrad": L.tlod_conv_dgrad_workspace_bytes(N, Ci, H, W, Co, 3),
        "conv_wgrad": L.tlod_conv_wgrad_workspace_bytes(N, Ci, H, W, Co, 3),
        "conv_fwd_bs": L.tlod_conv_fwd_bs_workspace_bytes(N, Ci, H, W, Co, 3, 6),
        "conv_wgrad_bs ws": L.tlod_conv_wgrad_bs_workspace_bytes(N, Ci, H, W, Co, 3, 6),
        "conv_wgrad_bs slab": L.tlod_conv_wgrad_bs_workspace_bytes(N, Ci, H, W, Co, 3, 3),
        "conv_wgrad_bs 1x1": L.tlod_conv_wgrad_bs_workspace_bytes(N, Ci, H, W, Co, 1, 6),
        "conv3x3_gemm": L.tlod_conv3x3_gemm_bs_workspace_bytes(N, Ci, H, W, Co, 0, 6),
        "conv1x1_gemm": L.tlod_conv1x1_gemm_bs_workspace_bytes(N, Ci, H, W, Co, 0, 6),
        "gemm": L.tlod_gemm_bs_workspace_bytes(*GEMM_SPLIT, 1, 1, 6),
        "gemm_nhwc3 fwd": L.tlod_gemm_nhwc3_bs_workspace_bytes(0, *NHWC3_SHAPES[0], 6),
        "gemm_nhwc3 dgrad": L.tlod_gemm_nhwc3_bs_workspace_bytes(1, *NHWC3_SHAPES[0], 6),
        "gemm_nhwc3 wgrad": L.tlod_gemm_nhwc3_bs_workspace_bytes(2, *NHWC3_SPLIT, 6),
        "conv1x1_small_wgrad": L.tlod_conv1x1_small_wgrad_workspace_bytes(2, 64, 8, 12, 3),
    }
    nosplit = {
        "conv_fwd": L.tlod_conv_fwd_workspace_bytes(n, ci, h, w, co, 3),
        "conv_dgrad": L.tlod_conv_dgrad_workspace_bytes(n, ci, h, w, co, 3),
        "conv_fwd_bs": L.tlod_conv_fwd_bs_workspace_bytes(n, ci, h, w, co, 3, 6),
        "conv3x3_gemm": L.tlod_conv3x3_gemm_bs_workspace_bytes(n, ci, h, w, co, 0, 6),
        "conv1x1_gemm": L.tlod_conv1x1_gemm_bs_workspace_bytes(n, ci, h, w, co, 0, 6),
        "gemm": L.tlod_gemm_bs_workspace_bytes(*GEMM_SHAPES[0], 1, 1, 6),
        "gemm_nhwc3 wgrad": L.tlod_gemm_nhwc3_bs_workspace_bytes(2, *NHWC3_SHAPES[0], 6),
    }
    # (the weight gradients, tlod_conv_wgrad_f32 / _bs_f32, always reduce through at least one
    # slab: their queries are never 0, so they have no "no split" shape)
    return split, nosplit


# One shape that provably takes plan_schedule's whole-rounds-plus-split-tail plan.  The f32 3x3
# forward with Cout > 64 tiles the output in 128 channels x 8 rows x 32 columns
# (conv.hip FwdCfg<2, 4, 2, 2, 8, 3>) and its slab is ksplit * n_tail * (128 * 8 * 32) floats,
# ksplit >= 2.  This map is 33 tiles (1 x 33 x 1): one more than a multiple of 8, 16 and 32
# slots, so under a reserve of 248 CUs whole rounds run unsplit and a short tail is split.
TAIL = (1, 512, 128, 264, 8)
TAIL_TILE_BYTES = 128 * 8 * 32 * 4


def tail_plan_query(L):
    """(query, tiles) of TAIL under the current reserve; asserts the split-tail plan: the slab
    holds ksplit * n_tail < 2 * tiles pieces, so n_tail < tiles — not every tile is split."""
    N, Ci, Co, H, W = TAIL
    tiles = N * -(-Co // 128) * -(-H // 8) * -(-W // 32)
    q = L.tlod_conv_fwd_workspace_bytes(N, Ci, H, W, Co, 3)
    assert q > 0 and q % TAIL_TILE_BYTES == 0, q
    assert q // TAIL_TILE_BYTES < 2 * tiles, (q // TAIL_TILE_BYTES, tiles)
    return q, tiles


@functools.lru_cache(maxsize=None)
def tail_data():
    N, Cin, Cout, H, W = TAIL
    g = torch.Generator().manual_seed(264)
    d = dict(N=N, Cin=Cin, Cout=Cout, H=H, W=W, KS=3)
    d["x"] = torch.randn(N, Cin, H, W, generator=g)
    d["w"] = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (Cin * 9)) ** 0.5
    d["b"], d["sc"] = torch.randn(Cout, generator=g), torch.rand(Cout, generator=g) + 0.5
    d["res"] = torch.randn(N, Cout, H, W, generator=g)
    d["y"] = F.conv2d(d["x"].double(), d["w"].double(), padding=1)
    d["wk"] = d["w"].reshape(Cout, Cin * 9).t().contiguous()
    return d


@pytest.mark.parametrize("ex", [False, True])
def test_conv_fwd_split_tail_plan(ex):
    """tlod_conv_fwd_f32 / _ex_f32 on the whole-rounds-plus-split-tail plan (asserted from the
    query), exact-size slab, then query - 1."""
    from tlod import _lib
    L = lib()
    _lib.check(L.tlod_set_cu_reserve(248), "set_cu_reserve")
    try:
        q, _ = tail_plan_query(L)
        assert guard_case(*op_fwd_f32(tail_data(), ex)) == q
    finally:
        _lib.check(L.tlod_set_cu_reserve(0), "set_cu_reserve")


def test_planner_shapes_split_and_do_not():
    split, nosplit = planner_queries(lib())
    assert all(v > 0 for v in split.values()), split
    assert all(v == 0 for v in nosplit.values()), nosplit


# ===================================================================== GEMMs
GEMM_SHAPES = [(37, 513, 17), (1, 7, 3), (5, 3000, 64), (64, 64, 4096)]  # M, N, K
GEMM_SPLIT = (64, 64, 4096)


@functools.lru_cache(maxsize=None)
def gemm_data(M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    d = dict(A=torch.randn(M, K, generator=g), B=torch.randn(N, K, generator=g),
             bias=torch.randn(N, generator=g), res=torch.randn(M, N, generator=g),
             mask=torch.relu(torch.randn(M, N, generator=g)))
    d["AB"] = d["A"].double() @ d["B"].double().t()
    return d


@pytest.mark.parametrize("ak,bk", [(1, 1), (1, 0), (0, 0), (0, 1)])
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("kind", ["plain", "ex", "mask"])
def test_gemm(reserve, kind, M, N, K, ak, bk):
    d, L = gemm_data(M, N, K), lib()
    a = d["A"] if ak else d["A"].t().contiguous()
    b = d["B"] if bk else d["B"].t().contiguous()

    def launch(c, over):
        q = L.tlod_gemm_bs_workspace_bytes(M, N, K, ak, bk, 6)
        ga, gb = c.inp(a, "a"), c.inp(b, "b")
        out = c.out((M, N), f32, "c")
        if kind == "plain":
            st = c.run(L.tlod_gemm_bs_f32, ga, gb, c.inp(d["bias"], "bias"), out, M, N, K, ak, bk,
                       6, *_ws(c, q, over))
        elif kind == "ex":
            st = c.run(L.tlod_gemm_bs_ex_f32, ga, gb, c.inp(d["bias"], "bias"),
                       c.inp(d["res"], "residual"), 1, out, M, N, K, ak, bk, 6, *_ws(c, q, over))
        else:
            st = c.run(L.tlod_gemm_bs_mask_f32, ga, gb, c.inp(d["res"], "residual"),
                       c.inp(d["mask"], "mask"), out, M, N, K, ak, bk, 6, *_ws(c, q, over))
        return st, q, out

    def verify(out):
        if kind == "plain":
            tlg._close(out.payload, d["AB"] + d["bias"].double(), "bf16x6")
        elif kind == "ex":
            ref = torch.relu(d["AB"] + d["bias"].double() + d["res"].double())
            _relu_close(tlg._close, out.payload, ref, "bf16x6")
        else:
            tlg._close(out.payload, (d["AB"] + d["res"].double()) * (d["mask"] > 0), "bf16x6")
    guard_case(launch, verify)


NHWC3_SPLIT = (40, 4, 4, 256, 256)  # the weight gradient (mode 2) splits here
NHWC3_SHAPES = [(3, 5, 7, 256, 48), (2, 1, 3, 512, 16), (1, 4, 4, 256, 256),
                NHWC3_SPLIT]  # R, H, W, C, O


@functools.lru_cache(maxsize=None)
def nhwc3_data(R, H, W, C, O):
    g = torch.Generator().manual_seed(R * 31 + C + O + W)
    rows = R * H * W
    d = dict(x=torch.randn(rows, C, generator=g), dy=torch.randn(rows, O, generator=g),
             bias=torch.randn(O, generator=g), res=torch.randn(rows, O, generator=g),
             m=torch.relu(torch.randn(rows, C, generator=g)), r2=torch.randn(rows, C, generator=g))
    w = torch.randn(O, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    d["wm"] = w.permute(0, 2, 3, 1).reshape(O, 9 * C).contiguous()
    d["wd"] = d["wm"].view(O, 9, C).flip(1).transpose(0, 1).reshape(9 * O, C).contiguous()
    xc = d["x"].view(R, H, W, C).permute(0, 3, 1, 2).double()
    dyc = d["dy"].view(R, H, W, O).permute(0, 3, 1, 2).double()
    d["y"] = F.conv2d(xc, w.double(), padding=1).permute(0, 2, 3, 1).reshape(rows, O)
    d["dx"] = torch.nn.grad.conv2d_input(xc.shape, w.double(), dyc, padding=1) \
        .permute(0, 2, 3, 1).reshape(rows, C)
    d["dw"] = torch.nn.grad.conv2d_weight(xc, (O, C, 3, 3), dyc, padding=1) \
        .permute(0, 2, 3, 1).reshape(O, 9 * C)
    return d


@pytest.mark.parametrize("R,H,W,C,O", NHWC3_SHAPES)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_gemm_nhwc3(reserve, mode, R, H, W, C, O):
    d, L = nhwc3_data(R, H, W, C, O), lib()
    rows = R * H * W

    def launch(c, over):
        q = L.tlod_gemm_nhwc3_bs_workspace_bytes(mode, R, H, W, C, O, 6)
        if mode == 0:
            out = c.out((rows, O), f32, "c")
            st = c.run(L.tlod_gemm_nhwc3_bs_f32, 0, c.inp(d["x"], "x"), c.inp(d["wm"], "w"),
                       c.inp(d["bias"], "bias"), c.inp(d["res"], "residual"), None, 1, out, R, H,
                       W, C, O, 6, *_ws(c, q, over))
        elif mode == 1:
            out = c.out((rows, C), f32, "c")
            st = c.run(L.tlod_gemm_nhwc3_bs_f32, 1, c.inp(d["dy"], "dy"), c.inp(d["wd"], "wd"),
                       None, c.inp(d["r2"], "residual"), c.inp(d["m"], "mask"), 0, out, R, H, W, C,
                       O, 6, *_ws(c, q, over))
        else:
            out = c.out((O, 9 * C), f32, "c")
            st = c.run(L.tlod_gemm_nhwc3_bs_f32, 2, c.inp(d["dy"], "dy"), c.inp(d["x"], "x"),
                       None, None, None, 0, out, R, H, W, C, O, 6, *_ws(c, q, over))
        return st, q, out

    def verify(out):
        if mode == 0:
            ref = torch.relu(d["y"] + d["bias"].double() + d["res"].double())
            _relu_close(tlg._close, out.payload, ref, "bf16x6")
        elif mode == 1:
            tlg._close(out.payload, (d["dx"] + d["r2"].double()) * (d["m"] > 0), "bf16x6")
        else:
            tlg._close(out.payload, d["dw"], "bf16x6")
    guard_case(launch, verify)


SMALL_SHAPES = [(2, 64, 8, 12, 3), (1, 7, 5, 5, 1), (3, 33, 16, 16, 4)]  # N, Cin, H, W, Cout


@pytest.mark.parametrize("N,Cin,H,W,Cout", SMALL_SHAPES)
def test_conv1x1_small(reserve, N, Cin, H, W, Cout):
    """dgrad: dx written, not accumulated; wgrad: dweight and dbias written."""
    L = lib()
    g = torch.Generator().manual_seed(N * 1000 + Cin + Cout)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, generator=g) * 0.05
    dy = torch.randn(N, Cout, H, W, generator=g)
    w4 = w.double().view(Cout, Cin, 1, 1)

    def dgrad(c, over):
        dx = c.out((N, Cin, H, W), f32, "dx")
        st = c.run(L.tlod_conv1x1_small_dgrad_f32, c.inp(dy, "dy"), N, Cout, H, W, c.inp(w, "w"),
                   Cin, dx)
        return st, 0, dx
    guard_case(dgrad, lambda dx: tcs._close(
        dx.payload, torch.nn.grad.conv2d_input(x.shape, w4, dy.double())))

    def wgrad(c, over):
        q = L.tlod_conv1x1_small_wgrad_workspace_bytes(N, Cin, H, W, Cout)
        dw, db = c.out((Cout, Cin), f32, "dweight"), c.out((Cout,), f32, "dbias")
        st = c.run(L.tlod_conv1x1_small_wgrad_f32, c.inp(dy, "dy"), c.inp(x, "x"), N, Cin, H, W,
                   Cout, dw, db, *_ws(c, q, over))
        return st, q, (dw, db)

    def verify(o):
        tcs._close(o[0].payload, torch.nn.grad.conv2d_weight(
            x.double(), w4.shape, dy.double()).view(Cout, Cin))
        tcs._close(o[1].payload, dy.double().sum((0, 2, 3)))
    assert guard_case(wgrad, verify) > 0


# ===================================================================== NMS, RPN layers
@pytest.mark.parametrize("max_keep", [0, 64])
@pytest.mark.parametrize("n", [65, 300])
def test_nms(n, max_keep):
    """keep[num_keep:] is "not written": the poison must still be there."""
    from helpers import clustered_boxes, sorted_dets
    L = lib()
    rng = np.random.default_rng(n + max_keep)
    d = sorted_dets(clustered_boxes(rng, n), rng)
    ref = onms.nms(d, 0.5, max_keep=max_keep or None)

    def launch(c, over):
        q = L.tlod_nms_workspace_bytes(n)
        keep, num = c.out((n,), i32, "keep"), c.out((1,), i32, "num_keep")
        st = c.run(L.tlod_nms_f32, c.inp(torch.from_numpy(d), "dets"), n, 5, 0.5, max_keep, keep,
                   num, *_ws(c, q, over))
        if st == 0:
            c.sync()
            k = int(num.payload.item())
            assert 0 <= k <= n, k
            keep.untouched = torch.arange(n, device="cuda") >= k
        return st, q, (keep, num)

    def verify(o):
        k = int(o[1].payload.item())
        assert k == len(ref) and 0 < k < n
        np.testing.assert_array_equal(o[0].payload[:k].cpu().numpy(), ref)
    assert guard_case(launch, verify) > 0


@pytest.mark.parametrize("with_props", [True, False])
@pytest.mark.parametrize("pre_nms", [100, 600, 2000])  # < N = 420 < B*N = 840 <
def test_proposal(pre_nms, with_props):
    """post_nms exceeds the anchors of an image, so the zero padding of rois_out is written by
    the kernel; delta_scale 0 keeps the decode exact (test_proposal_layer_batch2_matches_oracle)."""
    from helpers import rpn_outputs
    L = lib()
    B, H, W, post = 2, 5, 7, 500
    A = trp.BASE.shape[0]
    rng = np.random.default_rng(pre_nms)
    prob, deltas = rpn_outputs(rng, B, A, H, W, delta_scale=0.0)
    im_info = np.array([[H * 16, W * 16, 1.0], [H * 16 - 9, W * 16 - 20, 1.0]], np.float32)
    base = np.ascontiguousarray(trp.BASE, np.float32)
    ref = orpn.proposal_layer(prob, deltas, im_info, base, 16, pre_nms, post, 0.7)
    assert (ref[:, -1, 1:] == 0).all()  # padded rows exist
    t = torch.from_numpy

    def launch(c, over):
        q = L.tlod_proposal_workspace_bytes(B, A, H, W, pre_nms)
        rois = c.out((B, post, 5), f32, "rois_out")
        props = c.out((B, H * W * A, 4), f32, "props_out") if with_props else None
        st = c.run(L.tlod_proposal_f32, c.inp(t(prob), "cls_prob"), c.inp(t(deltas), "deltas"),
                   c.inp(t(im_info), "im_info"), c.inp(t(base), "anchors"), B, A, H, W, 16,
                   pre_nms, post, 0.7, rois, props, *_ws(c, q, over))
        return st, q, (rois, props)

    def verify(o):
        np.testing.assert_array_equal(o[0].payload.cpu().numpy(), ref)
        if with_props:
            _, oprops = orpn.decode_clip(prob, deltas, im_info, base, 16)
            np.testing.assert_allclose(o[1].payload.cpu().numpy(), oprops, rtol=2e-6, atol=1e-4)
    assert guard_case(launch, verify) > 0


def _anchor_setup():
    from helpers import gt_set
    from oracle.boxes import generate_anchors
    from tlod.config import setup_training_cfg
    from tlod.rpn.anchor_target import rpn_cfg_struct
    setup_training_cfg("vgg16")
    B, H, W, G, seed = 2, 10, 12, 3, 41
    rng = np.random.default_rng(seed)
    gts = np.stack([gt_set(rng, G=G, pad=G, W=W * 16, H=H * 16) for _ in range(B)])
    im_info = np.array([[H * 16, W * 16, 1.0]] * B, np.float32)
    # 16 .. 64 pixel anchors: most lie inside the 160 x 192 image, so the sampler has more
    # than 256 candidates to draw from (the suite's 64 .. 512 pixel anchors mostly do not)
    base = np.ascontiguousarray(generate_anchors(scales=np.array([1, 2, 4]),
                                                 ratios=np.array([0.5, 1, 2])), np.float32)
    return B, H, W, G, seed, gts, im_info, base, rpn_cfg_struct()


@functools.lru_cache(maxsize=None)
def _anchor_reference():
    """The oracle fed the device RNG's draws: the sampler drops the m candidates with the
    smallest (rng key, anchor index) pairs, key = stream 2b (fg) / 2b + 1 (bg) of the seed
    (test_anchor_target_device_rng_exact_subset restates it); here that subset is handed to
    oracle.rpn.anchor_target as the leading entries of its permutation draws."""
    B, H, W, G, seed, gts, im_info, base, _ = _anchor_setup()
    ident = type("N", (), {"permutation": lambda self, n: np.arange(n)})()
    cfg = dict(orpn.DEFAULT_RPN)
    cfg["batch"] = 10 ** 9  # no subsampling: the candidates
    A, HW = base.shape[0], H * W
    cand = orpn.anchor_target(H, W, gts, im_info, base, 16, ident, cfg)[0].reshape(B, -1)
    p = np.arange(A * HW)
    idx = (p % HW) * A + p // HW  # output (a, h, w) -> the kernels' anchor index (h, w, a)
    inv = np.argsort(idx)         # anchor index -> output position
    draws = []  # in the oracle's call order: fg then bg per image, each only if it subsamples
    for b in range(B):
        lab = cand[b][inv]  # in anchor order, as the oracle's inside-anchor lists are
        fg, bg = np.nonzero(lab == 1)[0], np.nonzero(lab == 0)[0]
        if len(fg) > 128:
            draws.append((fg, 2 * b, len(fg) - 128))
        if len(bg) > 256 - min(len(fg), 128):
            draws.append((bg, 2 * b + 1, len(bg) - (256 - min(len(fg), 128))))
    assert any(stream % 2 for _, stream, _ in draws), "the case must subsample"

    class Draws:
        def permutation(self, n):
            ids, stream, m = draws.pop(0)
            assert n == len(ids)
            first = np.lexsort((ids, trp._rng_key(seed, stream, ids)))[:m]
            return np.concatenate([first, np.setdiff1d(np.arange(n), first)])
    ref = orpn.anchor_target(H, W, gts, im_info, base, 16, Draws())
    assert not draws
    return ref


def _anchor_launch(fused, starve_sample=False):
    """launch(c, over) of the anchor-target pair / fused form on the device RNG.  over is the
    ws_bytes claimed instead of the query; starve_sample: only the sample phase gets it (the
    label phase runs with the full size first), and launch returns the two statuses."""
    B, H, W, G, seed, gts, im_info, base, cs = _anchor_setup()
    L, A, t = lib(), base.shape[0], torch.from_numpy

    def launch(c, over):
        q = L.tlod_anchor_target_workspace_bytes(B, A, H, W, G)
        anc, gt, info = c.inp(t(base), "anchors"), c.inp(t(gts), "gt"), c.inp(t(im_info), "info")
        counts = c.out((2 * B,), i32, "counts")
        outs = [c.out((B, 1, A * H, W), f32, "labels")] + \
               [c.out((B, 4 * A, H, W), f32, n) for n in ("targets", "inside_w", "outside_w")]
        wsp, wsb = _ws(c, q, over)
        if fused:
            st = c.run(L.tlod_anchor_target_f32, anc, A, H, W, 16, gt, B, G, info,
                       ctypes.byref(cs), seed, counts, *outs, wsp, wsb)
            return st, q, outs
        st = c.run(L.tlod_anchor_target_label_f32, anc, A, H, W, 16, gt, B, G, info,
                   ctypes.byref(cs), counts, wsp, q if starve_sample else wsb)
        if st == 0 or starve_sample:
            st2 = c.run(L.tlod_anchor_target_sample_f32, anc, A, H, W, 16, gt, B, G,
                        ctypes.byref(cs), None, None, seed, *outs, wsp, wsb)
            if starve_sample:
                return (st, st2), q, (counts, outs)
            st = st2
        return st, q, outs
    return launch


@pytest.mark.parametrize("fused", [False, True])
def test_anchor_target_device_rng(fused):
    ref = _anchor_reference()
    assert (ref[0] == 1).sum() > 0

    def verify(outs):
        for name, g, r in zip(["labels", "targets", "inside", "outside"], outs, ref):
            g = g.payload.cpu().numpy()
            if name == "targets":
                np.testing.assert_allclose(g, r, rtol=2e-6, atol=2e-6, err_msg=name)
            else:
                np.testing.assert_array_equal(g, r, err_msg=name)
    assert guard_case(_anchor_launch(fused), verify) > 0


def _pair_equals_fused(factory):
    """The two-phase calls and the fused form draw the same device RNG: bit-identical outputs
    (both forms run here, so the claim does not depend on which other tests ran)."""
    res = []
    for fused in (False, True):
        c = Call()
        st, _, outs = factory(fused)(c, None)
        _ok(st)
        c.check()
        res.append([o.payload.clone() for o in outs])
    for x, y in zip(*res):
        assert torch.equal(x, y)


def _sample_phase_refuses(factory):
    """Case B for the second phase on its own: the first phase runs with the full workspace,
    then the sample call is given query - 1 and must refuse, its outputs still pure poison
    (with both phases starved the first one fails and the second is never reached)."""
    c = Call()
    (st1, st2), q, (counts, outs) = factory(False, starve_sample=True)(c, None)
    _ok(st1)
    _ok(st2)
    c.check()
    assert q > 0
    c2 = Call()
    (st1, st2), _, (counts, outs) = factory(False, starve_sample=True)(c2, q - 1)
    _ok(st1)
    assert st2 == TLOD_EWORKSPACE, st2
    c2.sync()
    for g in c2.bufs:
        if g in outs:
            g.check_pure_poison()
        else:
            g.check()  # inputs unchanged, counts written by the first phase, guards intact


def test_anchor_target_pair_equals_fused():
    _pair_equals_fused(_anchor_launch)


def test_anchor_target_sample_refuses_small_workspace():
    _sample_phase_refuses(_anchor_launch)


def _ptarget_setup():
    from helpers import gt_set, random_boxes
    from tlod.config import setup_training_cfg
    from tlod.rpn.proposal_target import rcnn_cfg_struct
    setup_training_cfg("vgg16")
    B, R, G = 2, 128, 2
    rng = np.random.default_rng(17)
    gt = np.stack([gt_set(rng, G=G, pad=G) for _ in range(B)])
    rois = np.zeros((B, R, 5), np.float32)
    for b in range(B):
        n_real = R - 11
        near = gt[b, rng.integers(0, G, n_real // 2), :4] + rng.normal(0, 20, (n_real // 2, 4))
        boxes = np.concatenate([near, random_boxes(rng, n_real - n_real // 2)]).astype(np.float32)
        boxes[:, 2:] = np.maximum(boxes[:, 2:], boxes[:, :2] + 1)
        rois[b, :n_real, 1:] = np.clip(boxes, 0, 999)
        rois[b, :, 0] = b
    return B, R, G, gt, rois, rcnn_cfg_struct()


def _ptarget_verify(outs, rois, gt, S):
    """Device-RNG sampling against the oracle's rules (oracle.rpn.proposal_target): every
    sampled row is a candidate of its image, fg rows first with the oracle's label and
    normalised target (rtol 2e-6, the family's bar), bg rows label 0 and zero target / weights."""
    from oracle.boxes import bbox_overlaps, bbox_transform
    ro, lab, tg, iw, ow = (o.payload.cpu().numpy() for o in outs)
    B = rois.shape[0]
    cfg = orpn.DEFAULT_RCNN
    for b in range(B):
        gta = np.zeros_like(gt[b])
        gta[:, 1:5] = gt[b, :, :4]
        allr = np.concatenate([rois[b], gta], 0)
        allr[:, 0] = b
        ov = bbox_overlaps(allr[:, 1:5], gt[b])
        mx, arg = ov.max(1), ov.argmax(1)
        assert (ro[b, :, 0] == b).all()
        nfg = int((lab[b] > 0).sum())
        assert 0 < nfg <= int(round(cfg["fg_frac"] * S)) and (lab[b, nfg:] == 0).all()
        for s in range(S):
            hit = np.nonzero((allr[:, 1:] == ro[b, s, 1:]).all(1))[0]
            assert len(hit), (b, s)
            j = hit[0]
            if s < nfg:
                assert mx[j] >= np.float32(cfg["fg_thresh"]) and lab[b, s] == gt[b, arg[j], 4]
                t = bbox_transform(allr[j:j + 1, 1:5], gt[b][arg[j:j + 1], :4])
                t = ((t - np.asarray(cfg["means"], np.float32)) /
                     np.asarray(cfg["stds"], np.float32)).astype(np.float32)
                np.testing.assert_allclose(tg[b, s], t[0], rtol=2e-6, atol=2e-6)
                assert (iw[b, s] == 1).all() and (ow[b, s] == 1).all()
            else:
                assert (mx[hit] < np.float32(cfg["bg_hi"])).any()
                assert (tg[b, s] == 0).all() and (iw[b, s] == 0).all() and (ow[b, s] == 0).all()


def _ptarget_launch(fused, starve_sample=False):
    """As _anchor_launch, for the proposal-target count + sample pair / fused form."""
    B, R, G, gt, rois, cs = _ptarget_setup()
    L, S, seed, t = lib(), int(cs.batch_size), 123, torch.from_numpy

    def launch(c, over):
        q = L.tlod_proposal_target_workspace_bytes(B, R, G)
        r, g = c.inp(t(rois), "rois"), c.inp(t(gt), "gt")
        counts = c.out((2 * B,), i32, "counts")
        outs = [c.out((B, S, 5), f32, "rois_out"), c.out((B, S), f32, "labels")] + \
               [c.out((B, S, 4), f32, n) for n in ("targets", "inside_w", "outside_w")]
        wsp, wsb = _ws(c, q, over)
        if fused:
            st = c.run(L.tlod_proposal_target_f32, r, B, R, g, G, ctypes.byref(cs), seed, counts,
                       *outs, wsp, wsb)
            return st, q, outs
        st = c.run(L.tlod_proposal_target_count_f32, r, B, R, g, G, ctypes.byref(cs), counts,
                   wsp, q if starve_sample else wsb)
        if st == 0 or starve_sample:
            st2 = c.run(L.tlod_proposal_target_sample_f32, r, B, R, g, G, ctypes.byref(cs),
                        None, None, None, None, seed, *outs, wsp, wsb)
            if starve_sample:
                return (st, st2), q, (counts, outs)
            st = st2
        return st, q, outs
    return launch


@pytest.mark.parametrize("fused", [False, True])
def test_proposal_target_device_rng(fused):
    B, R, G, gt, rois, cs = _ptarget_setup()
    S = int(cs.batch_size)
    assert guard_case(_ptarget_launch(fused),
                      lambda outs: _ptarget_verify(outs, rois, gt, S)) > 0


def test_proposal_target_pair_equals_fused():
    _pair_equals_fused(_ptarget_launch)


def test_proposal_target_sample_refuses_small_workspace():
    _sample_phase_refuses(_ptarget_launch)


# ===================================================================== RoI align / pool
RB, RC, RH, RW, RR = 2, 8, 12, 16, 9
SCALE = 1.0 / 16


@functools.lru_cache(maxsize=None)
def roi_data():
    """A (2, 8, 12, 16) map and 9 RoIs with the malformed / off-map ones of _rois(edge=True),
    all inside the left half of the image: the right quarter of the map takes no tap."""
    rng = np.random.default_rng(5)
    feat = top._feat(rng, RB, RC, RH, RW)
    rois = top._rois(rng, RR, RB, RW * 16 // 2, RH * 16, edge=True)
    P = rng.standard_normal((RB, RC, RH, RW)).astype(np.float32)
    return feat, rois, P


def _acc_np(got, P, ref):
    """Case C for the RoI backwards: P + oracle at rtol 1e-5 / atol 1e-5 (test_ops_gpu), bit-equal
    to P in the cells no RoI tap reaches, which are at least a quarter of the map."""
    got = got.payload.cpu().numpy()
    zero = ref == 0
    assert zero.mean() >= 0.25, zero.mean()
    np.testing.assert_allclose(got, P + ref, rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(got[zero], P[zero])


@pytest.mark.parametrize("kind", ["align", "avg"])
def test_roi_align_fwd(kind):
    feat, rois, _ = roi_data()
    L, t = lib(), torch.from_numpy
    ah, aw = (4, 6) if kind == "align" else (7, 7)
    fn = L.tlod_roi_align_fwd_f32 if kind == "align" else L.tlod_roi_align_avg_fwd_f32
    ref = (oroi.roi_align_fwd if kind == "align" else oroi.roi_align_avg_fwd)(feat, rois, ah, aw,
                                                                             SCALE)

    def launch(c, over):
        out = c.out((RR, RC, ah, aw), f32, "out")
        st = c.run(fn, c.inp(t(feat), "feat"), RB, RC, RH, RW, c.inp(t(rois), "rois"), RR, ah, aw,
                   SCALE, out)
        return st, 0, out
    guard_case(launch, lambda o: np.testing.assert_array_equal(o.payload.cpu().numpy(), ref))


def test_roi_align_bwd_accumulates():
    feat, rois, P = roi_data()
    L, t = lib(), torch.from_numpy
    ah, aw = 4, 6
    g = np.random.default_rng(6).standard_normal((RR, RC, ah, aw)).astype(np.float32)
    ref = oroi.roi_align_bwd(g, rois, RB, RC, RH, RW, SCALE)

    def launch(c, over):
        bg = c.acc(t(P), "bottom_grad")
        st = c.run(L.tlod_roi_align_bwd_f32, c.inp(t(g), "top_grad"), RB, RC, RH, RW,
                   c.inp(t(rois), "rois"), RR, ah, aw, SCALE, bg)
        return st, 0, bg
    guard_case(launch, lambda o: _acc_np(o, P, ref))


def test_roi_pool_fwd_bwd():
    feat, rois, P = roi_data()
    L, t = lib(), torch.from_numpy
    ro, ra = oroi.roi_pool_fwd(feat, rois, 7, 7, SCALE)
    g = np.random.default_rng(7).standard_normal(ro.shape).astype(np.float32)
    ref = oroi.roi_pool_bwd(g, ra, rois, RB, RC, RH, RW, SCALE)

    def fwd(c, over):
        out, arg = c.out(ro.shape, f32, "out"), c.out(ro.shape, i32, "argmax")
        st = c.run(L.tlod_roi_pool_fwd_f32, c.inp(t(feat), "feat"), RB, RC, RH, RW,
                   c.inp(t(rois), "rois"), RR, 7, 7, SCALE, out, arg)
        return st, 0, (out, arg)

    def verify(o):
        np.testing.assert_array_equal(o[0].payload.cpu().numpy(), ro)
        np.testing.assert_array_equal(o[1].payload.cpu().numpy(), ra)
    guard_case(fwd, verify)

    def bwd(c, over):
        bg = c.acc(t(P), "bottom_grad")
        st = c.run(L.tlod_roi_pool_bwd_f32, c.inp(t(g), "top_grad"),
                   c.inp(t(np.ascontiguousarray(ra, np.int32)), "argmax"), RR, RC, 7, 7, bg)
        return st, 0, bg
    guard_case(bwd, lambda o: _acc_np(o, P, ref))


def test_roi_pool_bwd_gather_accumulates():
    """include/tlod_roi.h: the backward with the reference gather's tests.  Two RoIs are
    replaced by ones whose rounded extent is inverted; the oracle passes no gradient there."""
    feat, rois, P = roi_data()
    rois = rois.copy()
    rois[0, 1:] = [16 * 6.0, 16 * 4.0, 16 * 2.0, 16 * 1.0]
    rois[1, 1:] = [16 * 5.0, 16 * 1.0, 16 * 1.0, 16 * 3.0]
    L, t = lib(), torch.from_numpy
    ro, ra = oroi.roi_pool_fwd(feat, rois, 7, 7, SCALE)
    assert (ra[:2] >= 0).all()
    g = np.random.default_rng(7).standard_normal(ro.shape).astype(np.float32)
    ref = oroi.roi_pool_bwd(g, ra, rois, RB, RC, RH, RW, SCALE)
    g0 = g.copy()
    g0[:2] = 0
    np.testing.assert_array_equal(ref, oroi.roi_pool_bwd(g0, ra, rois, RB, RC, RH, RW, SCALE))

    def bwd(c, over):
        bg = c.acc(t(P), "bottom_grad")
        st = c.run(L.tlod_roi_pool_bwd_gather_f32, c.inp(t(g), "top_grad"),
                   c.inp(t(np.ascontiguousarray(ra, np.int32)), "argmax"), RB, RC, RH, RW,
                   c.inp(t(rois), "rois"), RR, 7, 7, SCALE, bg)
        return st, 0, bg
    guard_case(bwd, lambda o: _acc_np(o, P, ref))


@pytest.mark.parametrize("tier", ["gather", "accumulator", "null"])
def test_roi_align_avg_bwd_tiers(tier):
    """The three tiers are chosen by ws_bytes, so there is no too-small case here."""
    feat, rois, P = roi_data()
    L, t = lib(), torch.from_numpy
    g = np.random.default_rng(8).standard_normal((RR, RC, 7, 7)).astype(np.float32)
    ref = oroi.roi_align_avg_bwd(g, rois, RB, RC, RH, RW, SCALE)
    qg = L.tlod_roi_align_avg_bwd_gather_workspace_bytes(RB, RC, RH, RW, RR, 7, 7)
    qa = L.tlod_roi_align_avg_bwd_workspace_bytes(RB, RC, RH, RW)
    assert qg > qa > 0
    q = {"gather": qg, "accumulator": qa, "null": 0}[tier]

    def launch(c, over):
        bg = c.acc(t(P), "bottom_grad")
        st = c.run(L.tlod_roi_align_avg_bwd_f32, c.inp(t(g), "top_grad"), RB, RC, RH, RW,
                   c.inp(t(rois), "rois"), RR, 7, 7, SCALE, bg, *_ws(c, q, None))
        return st, 0, bg
    guard_case(launch, lambda o: _acc_np(o, P, ref))


@pytest.mark.parametrize("P_", [7, 6])
def test_roi_align_avg_s2(P_):
    """Bins (2i, 2j) only, channels-last; even P leaves the last row / column without a bin."""
    feat, rois, P = roi_data()
    L, t = lib(), torch.from_numpy
    Q = (P_ + 1) // 2
    full = oroi.roi_align_avg_fwd(feat, rois, P_, P_, SCALE)
    ref = np.ascontiguousarray(full.transpose(0, 2, 3, 1)[:, ::2, ::2, :])
    g = np.random.default_rng(9).standard_normal((RR, Q, Q, RC)).astype(np.float32)
    gfull = np.zeros((RR, RC, P_, P_), np.float32)
    gfull[:, :, ::2, ::2] = g.transpose(0, 3, 1, 2)
    refb = oroi.roi_align_avg_bwd(gfull, rois, RB, RC, RH, RW, SCALE)

    def fwd(c, over):
        q = L.tlod_roi_align_avg_s2_workspace_bytes(RB, RC, RH, RW, RR, P_, P_)
        out = c.out((RR, Q, Q, RC), f32, "out")
        st = c.run(L.tlod_roi_align_avg_s2_nhwc_fwd_f32, c.inp(t(feat), "feat"), RB, RC, RH, RW,
                   c.inp(t(rois), "rois"), RR, P_, P_, SCALE, out, *_ws(c, q, over))
        return st, q, out
    guard_case(fwd, lambda o: np.testing.assert_array_equal(o.payload.cpu().numpy(), ref))

    def bwd(c, over):
        q = L.tlod_roi_align_avg_s2_workspace_bytes(RB, RC, RH, RW, RR, P_, P_)
        bg = c.acc(t(P), "bottom_grad")
        st = c.run(L.tlod_roi_align_avg_s2_nhwc_bwd_f32, c.inp(t(g), "top_grad"), RB, RC, RH, RW,
                   c.inp(t(rois), "rois"), RR, P_, P_, SCALE, bg, *_ws(c, q, over))
        return st, q, bg
    assert guard_case(bwd, lambda o: _acc_np(o, P, refb)) > 0


# ===================================================================== RoI crop
def _crop_case():
    import ref_roi_crop as ref
    import test_roi_crop_gpu as trc
    x, rois = trc.inputs(5)
    return ref, trc, np.array(x), np.array(rois)


@pytest.mark.parametrize("G", [7, 6])
def test_roi_crop_sampler(G):
    """fwd writes every output (0 where all four taps are off the map); bwd OVERWRITES grad_in."""
    ref, trc, x, rois = _crop_case()
    L, t = lib(), torch.from_numpy
    want, grid = trc.samples(5, G)
    grid = np.array(grid)
    R, C = len(rois), 5
    go = trc.grad_out_for((R, C, G, G), 5)
    x64 = t(x).double().requires_grad_()
    ref.sample_t(x64, t(grid)).backward(t(go).double())
    gwant = x64.grad.numpy()

    def fwd(c, over):
        out = c.out((R, C, G, G), f32, "out")
        st = c.run(L.tlod_roi_crop_fwd_f32, c.inp(t(x), "x"), trc.B, C, trc.H, trc.W,
                   c.inp(t(grid), "grid"), R, G, G, out)
        return st, 0, out

    def vf(o):
        got = o.payload.cpu().numpy()
        assert np.all(got[3] == 0) and np.all(got[9] == 0)  # RoIs entirely outside the map
        assert float(np.abs(got - want).max()) <= 16 * 2.0 ** -24 * float(np.abs(x).max())
    guard_case(fwd, vf)

    def bwd(c, over):
        gi = c.out((trc.B, C, trc.H, trc.W), f32, "grad_in")
        st = c.run(L.tlod_roi_crop_bwd_f32, c.inp(t(go), "grad_out"), c.inp(t(grid), "grid"), R, C,
                   G, G, trc.B, trc.H, trc.W, gi)
        return st, 0, gi
    guard_case(bwd, lambda o: np.testing.assert_array_less(
        np.abs(o.payload.cpu().numpy() - gwant).max(), 1e-5 * np.abs(gwant).max() + 1e-30))


@pytest.mark.parametrize("mp", [1, 0])
def test_roi_crop_pool(mp):
    """Two RoIs name an image outside [0, B): their outputs are 0 (argmax written too) and
    they add no gradient."""
    ref, trc, x, rois = _crop_case()
    L, t = lib(), torch.from_numpy
    C, P = 5, 7
    R = len(rois)
    bad = rois.copy()
    bad[0, 0], bad[5, 0] = 2.0, -1.0
    scale = float(np.abs(x).max())
    v, _ = trc.samples(C, 2 * P if mp else P)
    if mp:
        trc.assert_unambiguous(v, scale)
        want, want_idx = ref.max_pool_2x2(v)
        want_idx = np.array(want_idx)
        want_idx[[0, 5]] = 0
    else:
        want = v
    want = np.array(want)
    want[[0, 5]] = 0
    go = trc.grad_out_for((R, C, P, P), 6)
    go0 = go.copy()
    go0[[0, 5]] = 0
    x64 = t(x).double().requires_grad_()
    ref.crop_pool_t(x64, rois, P, mp).backward(t(go0).double())
    gwant = x64.grad.numpy()

    def fwd(c, over):
        out = c.out((R, C, P, P), f32, "out")
        am = c.out((R, C, P, P), u8, "argmax") if mp else None
        st = c.run(L.tlod_roi_crop_pool_fwd_f32, c.inp(t(x), "x"), trc.B, C, trc.H, trc.W,
                   c.inp(t(bad), "rois"), R, P, SCALE, mp, out, am)
        return st, 0, (out, am)

    def vf(o):
        got = o[0].payload.cpu().numpy()
        assert not got[0].any() and not got[5].any()
        assert float(np.abs(got - want).max()) <= 1e-5 * scale
        if mp:
            am = o[1].payload.cpu().numpy()
            keep = [i for i in range(R) if i not in (0, 5)]
            np.testing.assert_array_equal(am[keep], want_idx[keep])
            assert am.max() <= 3
    guard_case(fwd, vf)

    def bwd(c, over):
        gi = c.out((trc.B, C, trc.H, trc.W), f32, "grad_in")
        am = c.inp(t(want_idx.astype(np.uint8)), "argmax") if mp else None
        st = c.run(L.tlod_roi_crop_pool_bwd_f32, c.inp(t(go), "grad_out"), am, trc.B, C, trc.H,
                   trc.W, c.inp(t(bad), "rois"), R, P, SCALE, mp, gi)
        return st, 0, gi
    guard_case(bwd, lambda o: np.testing.assert_array_less(
        np.abs(o.payload.cpu().numpy() - gwant).max(), 1e-5 * np.abs(gwant).max() + 1e-30))


# ===================================================================== D: permutations, masks
def test_upsample2_zero_odd_map():
    L = lib()
    N, C, H, W = 2, 3, 7, 9
    dy = torch.randn(N, C, (H + 1) // 2, (W + 1) // 2, generator=torch.Generator().manual_seed(1))
    ref = torch.zeros(N, C, H, W)
    ref[:, :, ::2, ::2] = dy

    def launch(c, over):
        dx = c.out((N, C, H, W), f32, "dx")
        return c.run(L.tlod_upsample2_zero_f32, c.inp(dy, "dy"), N, C, H, W, dx), 0, dx
    guard_case(launch, _same(ref))


def test_depth_to_space_and_drm_relu_bwd_cropped_border():
    """H, W no multiples of s: the cropped-away border of dx / g must come out 0."""
    L = lib()
    B, C, H, W, s = 2, 3, 7, 11, 3
    Ho, Wo = H // s, W // s
    g = torch.Generator().manual_seed(2)
    dy = torch.randn(B, C * s * s, Ho, Wo, generator=g)
    y = torch.relu(torch.randn(B, C * s * s, Ho, Wo, generator=g))

    def ref_of(t):
        r = torch.zeros(B, C, H, W)
        r[:, :, :Ho * s, :Wo * s] = F.pixel_shuffle(t, s)
        return r

    def d2s(c, over):
        dx = c.out((B, C, H, W), f32, "dx")
        return c.run(L.tlod_depth_to_space_f32, c.inp(dy, "dy"), B, C, H, W, s, dx), 0, dx
    guard_case(d2s, _same(ref_of(dy)))

    def drm(c, over):
        gg = c.out((B, C, H, W), f32, "g")
        st = c.run(L.tlod_drm_relu_bwd_f32, c.inp(dy, "dy"), c.inp(y, "y"), B, C, H, W, s, gg)
        return st, 0, gg
    want = ref_of(dy * (y > 0))
    guard_case(drm, _same(want))


@pytest.mark.parametrize("R,H,W,C", [(3, 2, 7, 12), (2, 1, 1, 4), (5, 4, 4, 32)])
def test_col2im3x3_nhwc(R, H, W, C):
    """The family's own test and bar, test_resnet_gpu.test_im2col3x3_nhwc: the fp32 autograd of
    the torch composition (F.pad + 9 slices + cat) that col2im replaces, at
    torch.testing.assert_close(rtol=1e-6, atol=1e-6) — restated here because that test writes
    the bar inline; it is not a new one.  The masked form is held to what the family holds it
    to (test_head_fused_backward_bit_identical): bit-identical to the plain result times
    (mask > 0)."""
    L = lib()
    g = torch.Generator().manual_seed(R * 100 + C)
    col = torch.randn(R * H * W, 9 * C, generator=g)
    mask = torch.relu(torch.randn(R, H, W, C, generator=g))
    xr = torch.zeros(R, H, W, C, requires_grad=True)
    pad = F.pad(xr, (0, 0, 1, 1, 1, 1))
    torch.cat([pad[:, kh:kh + H, kw:kw + W, :] for kh in range(3) for kw in range(3)],
              3).reshape(R * H * W, 9 * C).backward(col)
    ref = xr.grad
    got = {}

    def plain(c, over):
        dx = c.out((R, H, W, C), f32, "dx")
        return c.run(L.tlod_col2im3x3_nhwc_f32, c.inp(col, "col"), R, H, W, C, dx), 0, dx

    def vplain(o):
        got["plain"] = o.payload.cpu().clone()
        torch.testing.assert_close(got["plain"], ref, rtol=1e-6, atol=1e-6)
    guard_case(plain, vplain)

    def masked(c, over):
        dx = c.out((R, H, W, C), f32, "dx")
        st = c.run(L.tlod_col2im3x3_nhwc_mask_f32, c.inp(col, "col"), R, H, W, C,
                   c.inp(mask, "mask"), dx)
        return st, 0, dx
    guard_case(masked, _same(got["plain"] * (mask > 0)))


@pytest.mark.parametrize("alias", [False, True])
def test_relu_bwd_bias_and_ex(alias):
    """db is written, not accumulated (poison in, sums out); g may alias dy."""
    L = lib()
    N, C, H, W = 2, 5, 7, 9
    gen = torch.Generator().manual_seed(3)
    dy = torch.randn(N, C, H, W, generator=gen)
    y = torch.relu(torch.randn(N, C, H, W, generator=gen))
    sc = torch.rand(C, generator=gen) + 0.5
    g0 = dy * (y > 0)

    def bias(c, over):
        if alias:
            g = c.acc(dy, "dy=g")
            src = g
        else:
            src, g = c.inp(dy, "dy"), c.out((N, C, H, W), f32, "g")
        db = c.out((C,), f32, "db")
        st = c.run(L.tlod_relu_bwd_bias_f32, src, c.inp(y, "y"), g, db, N, C, H * W)
        return st, 0, (g, db)

    def vb(o):
        assert torch.equal(o[0].payload.cpu(), g0)
        tcg._close(o[1].payload, g0.double().sum((0, 2, 3)))
    guard_case(bias, vb)
    if alias:
        return

    def ex(c, over):
        g, raw, db = (c.out((N, C, H, W), f32, "g"), c.out((N, C, H, W), f32, "g_raw"),
                      c.out((C,), f32, "db"))
        st = c.run(L.tlod_relu_bwd_ex_f32, c.inp(dy, "dy"), c.inp(y, "y"), c.inp(sc, "scale"), g,
                   raw, db, N, C, H * W)
        return st, 0, (g, raw, db)

    def ve(o):
        assert torch.equal(o[0].payload.cpu(), g0 * sc.view(1, -1, 1, 1))
        assert torch.equal(o[1].payload.cpu(), g0)
        tcg._close(o[2].payload, g0.double().sum((0, 2, 3)))
    guard_case(ex, ve)


def test_maxpool2x2_relu_bwd_odd_map():
    """Odd H, W: the last row and column belong to no window and must come out 0."""
    L = lib()
    N, C, H, W = 2, 5, 7, 9
    gen = torch.Generator().manual_seed(4)
    z = torch.randn(N, C, H, W, generator=gen)
    z[z.abs() < 0.3] = 0.0
    zr = z.clone().requires_grad_(True)
    yr = F.relu(zr)
    p = F.max_pool2d(yr, 2, 2)
    dp = torch.randn(p.shape, generator=gen)
    p.backward(dp)
    ref = zr.grad
    assert not ref[:, :, -1].any() and not ref[:, :, :, -1].any()

    def launch(c, over):
        g, db = c.out((N, C, H, W), f32, "g"), c.out((C,), f32, "db")
        st = c.run(L.tlod_maxpool2x2_relu_bwd_f32, c.inp(dp, "dp"), c.inp(yr.detach(), "y"), N, C,
                   H, W, g, db)
        return st, 0, (g, db)

    def verify(o):
        assert torch.equal(o[0].payload.cpu(), ref)
        r = ref.double().sum((0, 2, 3))  # the bound of test_maxpool_fwd_bwd_exact
        bound = 1e-6 * ref.double().abs().sum((0, 2, 3)) + 1e-7
        assert bool(((o[1].payload.cpu().double() - r).abs() <= bound).all())
    guard_case(launch, verify)


# ===================================================================== D: losses
def _exact_zeros(got, ref):
    """Where the reference gradient is exactly 0 (padding rows, other classes' columns) the
    kernel must have written an exact 0."""
    z = ref == 0
    assert bool(z.any()) and not bool(got[z].any())


def test_rpn_loss_bwd_extra_image():
    from tlod.detector.losses import masked_cross_entropy, smooth_l1_loss
    from tlod.rpn.rpn_head import _RPN
    L = lib()
    B, A, H, W = 2, 9, 5, 7
    score, bbox, lab, tgt, inside, outside = (x.cpu() for x in tlo.rpn_inputs(B, A, H, W, 2005))
    gen = torch.Generator().manual_seed(5)
    score2 = torch.cat([score, torch.randn(1, 2 * A, H, W, generator=gen)], 0)
    bbox2 = torch.cat([bbox, torch.randn(1, 4 * A, H, W, generator=gen)], 0)
    s2, b2 = score.clone().requires_grad_(True), bbox.clone().requires_grad_(True)
    scores = _RPN.reshape(s2, 2).permute(0, 2, 3, 1).contiguous().view(-1, 2)
    rc = masked_cross_entropy(scores, lab.view(B, -1).view(-1))
    rb = smooth_l1_loss(b2, tgt, inside, outside, sigma=3, dim=[1, 2, 3])
    (2.0 * rc + 0.5 * rb).backward()
    count = torch.tensor([max(float((lab != -1).sum()), 1.0)])

    def launch(c, over):
        ds, dbx = c.out(score2.shape, f32, "dscore"), c.out(bbox2.shape, f32, "dbbox")
        st = c.run(L.tlod_rpn_loss_bwd_f32, c.inp(score2, "score"), c.inp(lab, "labels"),
                   c.inp(bbox2, "bbox"), c.inp(tgt, "targets"), c.inp(inside, "inside"),
                   c.inp(outside, "outside"), B, B + 1, A, H, W, 3.0,
                   c.inp(torch.tensor([2.0, 0.5]), "grad_loss"), c.inp(count, "count"), ds, dbx)
        return st, 0, (ds, dbx)

    def verify(o):
        ds, dbx = o[0].payload.cpu(), o[1].payload.cpu()
        tlo.close(ds[:B], s2.grad)
        tlo.close(dbx[:B], b2.grad)
        assert not ds[B:].any() and not dbx[B:].any()  # zero past image B
        _exact_zeros(dbx[:B], b2.grad)
    guard_case(launch, verify)


@pytest.mark.parametrize("agnostic", [0, 1])
def test_rcnn_loss_bwd_extra_rows(agnostic):
    from tlod.detector.losses import smooth_l1_loss
    L = lib()
    R, C = 37, 9
    Rt = R + 3
    gen = torch.Generator().manual_seed(R + C + agnostic)
    cls = torch.randn(Rt, C, generator=gen) * 2
    box = torch.randn(Rt, 4 if agnostic else 4 * C, generator=gen)
    lab = torch.randint(0, C, (R,), generator=gen)
    lab[: R // 4] = 0
    tgt = torch.randn(R, 4, generator=gen) * 0.5
    inside = (lab > 0).float()[:, None].expand(R, 4).contiguous()
    c2, b2 = cls[:R].clone().requires_grad_(True), box[:R].clone().requires_grad_(True)
    bp = b2 if agnostic else torch.gather(b2.view(R, C, 4), 1,
                                          lab.view(-1, 1, 1).expand(-1, 1, 4)).squeeze(1)
    (F.cross_entropy(c2, lab) + 3.0 * smooth_l1_loss(bp, tgt, inside, inside)).backward()
    prob = F.softmax(cls[:R], 1)

    def launch(c, over):
        dc, dbx = c.out((Rt, C), f32, "dcls"), c.out(box.shape, f32, "dbbox")
        st = c.run(L.tlod_rcnn_loss_bwd_f32, c.inp(prob, "cls_prob"), c.inp(box, "bbox_pred"),
                   c.inp(lab, "labels"), c.inp(tgt, "targets"), c.inp(inside, "inside"),
                   c.inp(inside.clone(), "outside"), R, Rt, C, agnostic, 1.0,
                   c.inp(torch.tensor([1.0, 3.0]), "grad_loss"), dc, dbx)
        return st, 0, (dc, dbx)

    def verify(o):
        dc, dbx = o[0].payload.cpu(), o[1].payload.cpu()
        tlo.close(dc[:R], c2.grad)
        tlo.close(dbx[:R], b2.grad)
        assert not dc[R:].any() and not dbx[R:].any()  # zeros past row R
        _exact_zeros(dbx[:R], b2.grad)                 # and off the label's columns
    guard_case(launch, verify)


def test_da_loss_fwd_bwd():
    L = lib()
    Bs, Bt, Hs, Ws, Ht, Wt, n_s, n_t = 2, 1, 9, 11, 5, 6, 512, 300
    gen = torch.Generator().manual_seed(Bs * 7 + n_t)
    ss = torch.randn(Bs, 2, Hs, Ws, generator=gen) * 2
    st_ = torch.randn(Bt, 2, Ht, Wt, generator=gen) * 2
    ins_s, ins_t = torch.rand(n_s, 1, generator=gen), torch.rand(n_t, 1, generator=gen)
    ins_t[0, 0], ins_t[1, 0] = 1.0, 0.0
    need_s, need_t = torch.tensor([1.0, 0.0]), torch.zeros(Bt)
    w = torch.tensor([1.0, 0.5, 2.0, 0.25, 3.0, 0.125])
    ys = [t.clone().requires_grad_(True) for t in (ss, st_, ins_s, ins_t)]
    ref = tlo.da_reference(*ys, need_s, need_t)  # img_s, ins_s, img_t, ins_t, cst_s, cst_t
    (torch.stack(ref) @ w).backward()
    order = [0, 1, 4, 2, 3, 5]  # the ABI's loss layout: source (img, ins, cst), then target
    aux = {}

    def fwd(c, over):
        loss, cons = c.out((6,), f32, "loss"), c.out((2,), f32, "cons")
        st = c.run(L.tlod_da_loss_f32, c.inp(ss, "score_s"), c.inp(st_, "score_t"),
                   c.inp(need_s, "need_s"), c.inp(need_t, "need_t"), c.inp(ins_s, "ins_s"),
                   c.inp(ins_t, "ins_t"), Bs, Bt, Hs, Ws, Ht, Wt, n_s, n_t, loss, cons)
        return st, 0, (loss, cons)

    def vf(o):
        loss = o[0].payload.cpu()
        for k, j in enumerate(order):
            tlo.close(loss[k].reshape(1), ref[j].detach().reshape(1))
        aux["cons"] = o[1].payload.cpu().clone()
    guard_case(fwd, vf)

    def bwd(c, over):
        outs = [c.out(t.shape, f32, n) for t, n in ((ss, "dscore_s"), (st_, "dscore_t"),
                                                    (ins_s, "dins_s"), (ins_t, "dins_t"))]
        st = c.run(L.tlod_da_loss_bwd_f32, c.inp(ss, "score_s"), c.inp(st_, "score_t"),
                   c.inp(need_s, "need_s"), c.inp(need_t, "need_t"), c.inp(ins_s, "ins_s"),
                   c.inp(ins_t, "ins_t"), Bs, Bt, Hs, Ws, Ht, Wt, n_s, n_t,
                   c.inp(w[order].contiguous(), "grad_loss"), c.inp(aux["cons"], "cons"), *outs)
        return st, 0, outs

    def vb(o):
        for got, y in zip(o, ys):
            tlo.close(got.payload.cpu(), y.grad)
    guard_case(bwd, vb)


def _ptrs(gs):
    return (ctypes.c_void_p * len(gs))(*[g.ptr.value for g in gs])


def test_masked_nll2_empty_map():
    """An empty map: loss 0 and an all-zero gradient buffer, written in full."""
    import test_pt_maf_ops_gpu as tpm
    L = lib()
    B, H, W, K = 2, 5, 7, 3
    scores, maps, need = tpm._nll_inputs(B, H, W, 105)
    scores = [s.detach().cpu() for s in scores]
    maps = [m.cpu() for m in maps]
    need = need.cpu()
    maps[1].zero_()
    refs = [tpm._nll_ref(s, m, need) for s, m in zip(scores, maps)]
    gw = torch.arange(1, K * B + 1, dtype=torch.float32).view(K, B) / 7
    for k, (s64, r) in enumerate(refs):
        (r * gw[k].double()).sum().backward()
    aux = {}

    def fwd(c, over):
        gs, gm = [c.inp(s, "score") for s in scores], [c.inp(m, "map") for m in maps]
        loss, count = c.out((K, B), f32, "loss"), c.out((K, B), f32, "count")
        st = c.run(L.tlod_masked_nll2_f32, _ptrs(gs), _ptrs(gm), K, c.inp(need, "need"), B, H, W,
                   loss, count)
        return st, 0, (loss, count)

    def vf(o):
        loss, count = o[0].payload.cpu(), o[1].payload.cpu()
        for k in range(K):
            tlo.close(loss[k], refs[k][1].detach())
        assert (loss[1] == 0).all()
        assert torch.equal(count, torch.stack([m.sum((1, 2)) for m in maps]))
        aux["count"] = count.clone()
    guard_case(fwd, vf)

    def bwd(c, over):
        gs, gm = [c.inp(s, "score") for s in scores], [c.inp(m, "map") for m in maps]
        d = [c.out((B, 2, H, W), f32, f"dscores[{k}]") for k in range(K)]
        st = c.run(L.tlod_masked_nll2_bwd_f32, _ptrs(gs), _ptrs(gm), K, c.inp(need, "need"), B, H,
                   W, c.inp(gw, "grad_loss"), c.inp(aux["count"], "count"), _ptrs(d))
        return st, 0, d

    def vb(o):
        for k in range(K):
            tlo.close(o[k].payload.cpu(), refs[k][0].grad)
        assert not o[1].payload.any()
    guard_case(bwd, vb)


def test_kd_kl_strided_rpn_layout():
    import test_pt_maf_ops_gpu as tpm
    L = lib()
    A, H, W, T = 3, 5, 7, 3.0
    gen = torch.Generator().manual_seed(A + H + W)
    s = torch.randn(1, 2, A * H, W, generator=gen) * 2
    t = torch.randn(1, 2, A * H, W, generator=gen) * 2
    cells = (torch.rand(H, W, generator=gen) < 0.3).float()
    s64, ref = tpm._kd_ref(s, t, cells, T, (A, H, W))
    (ref * 1.5).backward()
    R = A * H * W
    aux = {}

    def fwd(c, over):
        out = c.out((2,), f32, "out")
        st = c.run(L.tlod_kd_kl_f32, c.inp(s, "student"), c.inp(t, "teacher"),
                   c.inp(cells, "weight"), R, 2, 1, R, H * W, T, out)
        return st, 0, out

    def vf(o):
        out = o.payload.cpu()
        tlo.close(out[:1], ref.detach().reshape(1))
        assert float(out[1]) == float(cells.sum()) + 1
        aux["out"] = out.clone()
    guard_case(fwd, vf)

    def bwd(c, over):
        d = c.out(s.shape, f32, "dstudent")
        st = c.run(L.tlod_kd_kl_bwd_f32, c.inp(s, "student"), c.inp(t, "teacher"),
                   c.inp(cells, "weight"), R, 2, 1, R, H * W, T,
                   c.inp(torch.tensor([1.5]), "grad_loss"), c.inp(aux["out"], "aux"), d)
        return st, 0, d
    guard_case(bwd, lambda o: tlo.close(o.payload.cpu(), s64.grad))


def test_us_daf_calls():
    """Scale labels, the four losses with s / gates written out, and the backward; the two
    domains' maps have different shapes, so nothing is packed."""
    import test_us_daf_ops_gpu as tus
    from ref_us_daf import scale_labels
    L = lib()
    (Bs, Hs, Ws), (Bt, Ht, Wt), n_s, n_t = (2, 5, 7), (1, 3, 4), 19, 11
    z_img, z_ins, rois = tus._inputs((Bs, Hs, Ws), (Bt, Ht, Wt), n_s, n_t, seed=12)
    G = torch.tensor([float(g) for g in tus.G])
    aux = {}

    def labels(c, over):
        lab = c.out((n_s, 3), f32, "labels")
        return c.run(L.tlod_roi_scale_labels_f32, c.inp(rois[0], "rois"), n_s, lab), 0, lab
    guard_case(labels, _same(scale_labels(rois[0].numpy())))

    def fwd(c, over):
        zi = [c.inp(z, "z_img") for z in z_img]
        zn = [c.inp(z, "z_ins") for z in z_ins]
        rr = [c.inp(r, "rois") for r in rois]
        s_i = [c.out(z.shape, f32, "s_img") for z in z_img]
        s_n = [c.out(z.shape, f32, "s_ins") for z in z_ins]
        gate = [c.out((n,), f32, "gate") for n in (n_s, n_t)]
        loss = c.out((4,), f32, "loss")
        st = c.run(L.tlod_us_daf_loss_f32, *zi, *zn, *rr, None, None, Bs, Bt, Hs, Ws, Ht, Wt, n_s,
                   n_t, *s_i, *s_n, *gate, loss)
        return st, 0, (s_i, s_n, gate, loss)

    def vf(o):
        s_i, s_n, gate, loss = o
        s = [g.payload.cpu() for g in s_i + s_n]
        for got, z in zip(s, z_img + z_ins):
            assert tus._ulp_diff(got, torch.sigmoid(z)) <= 2
        ref_l, ref_di, ref_dn, own, col0 = tus._reference(s[:2], s[2:], rois)
        for k in range(2):
            assert torch.equal(gate[k].payload.cpu(), own[k].float())
        for k in range(4):
            tlo.close(loss.payload.cpu()[k].reshape(1), ref_l[k].reshape(1))
        aux.update(s=s, gate=[g.payload.cpu().clone() for g in gate], di=ref_di, dn=ref_dn)
    guard_case(fwd, vf)

    def bwd(c, over):
        s = [c.inp(x, "s") for x in aux["s"]]
        rr = [c.inp(r, "rois") for r in rois]
        gate = [c.inp(g, "gate") for g in aux["gate"]]
        d = [c.out(z.shape, f32, "dz") for z in z_img + z_ins]
        st = c.run(L.tlod_us_daf_loss_bwd_f32, *s, *rr, *gate, Bs, Bt, Hs, Ws, Ht, Wt, n_s, n_t,
                   c.inp(G, "grad_loss"), *d)
        return st, 0, d

    def vb(o):
        for k in range(2):
            tlo.close(o[k].payload.cpu(), aux["di"][k])
            tlo.close(o[2 + k].payload.cpu(), aux["dn"][k])
    guard_case(bwd, vb)


# ===================================================================== D: blob, detections
def test_image_blob_zero_padding():
    """Hd < Ho, Wd < Wo: out is the kept region of the resized image, zeros around it."""
    from oracle import blob as oblob
    from tlod.data.blob import linear_taps, pixel_lut, resized_size
    L = lib()
    H, W, fx = 23, 31, 1.37
    means = np.array([[[102.9801, 115.9465, 122.7717]]])
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    Hr, Wr = resized_size(H, fx), resized_size(W, fx)
    y0, x0, Hd, Wd, Ho, Wo = 2, 3, 10, 12, 14, 17
    im = src[:, :, ::-1].astype(np.float32, copy=True)
    im -= means
    res = oblob.cv2_resize_linear(im, fx)
    assert res.shape[:2] == (Hr, Wr)
    ref = np.zeros((3, Ho, Wo), np.float32)
    ref[:, :Hd, :Wd] = res[y0:y0 + Hd, x0:x0 + Wd].transpose(2, 0, 1)

    def raw(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy())

    def launch(c, over):
        out = c.out((3, Ho, Wo), f32, "out")
        st = c.run(L.tlod_image_blob_u8, c.inp(torch.from_numpy(src), "src"), H, W,
                   c.inp(torch.from_numpy(pixel_lut(means.reshape(3))), "lut"),
                   c.inp(raw(linear_taps(W, Wr, fx)), "xtab"),
                   c.inp(raw(linear_taps(H, Hr, fx)), "ytab"), Hr, Wr, y0, x0, Hd, Wd, Ho, Wo, out)
        return st, 0, out
    guard_case(launch, lambda o: np.testing.assert_array_equal(o.payload.cpu().numpy(), ref))


@pytest.mark.parametrize("agnostic", [False, True])
def test_detect_with_boxes_out(agnostic):
    """dets rows past counts[j] are not specified by the header: guards only."""
    import test_eval_gpu as tev
    from oracle import detect as odet
    L = lib()
    R, C, thresh = 300, 9, 0.05
    rng = np.random.default_rng(R + C)
    rois, prob, bp = tev._inputs(rng, R, C, agnostic)
    info = np.array([600, 1000, 1.6], np.float32)
    f4 = ctypes.c_float * 4
    stds, means = f4(0.1, 0.1, 0.2, 0.2), f4(0.0, 0.0, 0.0, 0.0)
    ref_boxes = odet.decode(rois, bp, info, C, agnostic)
    t = torch.from_numpy

    def launch(c, over):
        dets = c.acc(torch.full((C, R, 5), -7.0), "dets")  # (partly written: guards only)
        counts, boxes = c.out((C,), i32, "counts"), c.out((R, C, 4), f32, "boxes_out")
        st = c.run(L.tlod_detect_f32, c.inp(t(rois), "rois"), c.inp(t(prob), "cls_prob"),
                   c.inp(t(bp), "bbox_pred"), R, C, int(agnostic), stds, means, 600.0, 1000.0, 1.6,
                   thresh, 0.3, dets, counts, boxes)
        return st, 0, (dets, counts, boxes)

    def verify(o):
        d, n, boxes = (x.payload.cpu().numpy() for x in o)
        # every box, the background column too (it has no workgroup of its own)
        np.testing.assert_allclose(boxes, ref_boxes, rtol=2e-6, atol=1e-4)
        ref = odet.postprocess(boxes, prob, thresh, 0.3, max_per_image=0)
        assert n[0] == 0 and sum(int(x) for x in n[1:]) > 0
        for j in range(1, C):
            np.testing.assert_array_equal(d[j, :n[j]], ref[j], err_msg=f"class {j}")
    guard_case(launch, verify)


# ===================================================================== E: plain full writes
@pytest.mark.parametrize("Cout,Cin", [(20, 13), (36, 8)])
def test_weight_packs(Cout, Cin):
    """The four pack functions; the split-bf16 buffer is exactly tlod_conv_pack_bs_bytes (the
    padded c*80 + s*8 layout with ragged Cin = 13 reaches its last byte and no further)."""
    L = lib()
    gen = torch.Generator().manual_seed(Cout * 1000 + Cin)
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) * torch.exp(torch.randn(Cout, Cin, 3, 3,
                                                                            generator=gen))
    sc = torch.rand(Cout, generator=gen) + 0.5
    wk = w.reshape(Cout, Cin * 9).t().contiguous()
    wd = w.reshape(Cout, Cin, 9).flip(2).permute(0, 2, 1).reshape(Cout * 9, Cin).contiguous()

    def fwd(c, over):
        o = c.out(wk.shape, f32, "wk")
        return c.run(L.tlod_conv_pack_fwd_f32, c.inp(w, "weight"), Cout, Cin, 3, o), 0, o
    guard_case(fwd, _same(wk))

    def dgr(c, over):
        o = c.out(wd.shape, f32, "wd")
        return c.run(L.tlod_conv_pack_dgrad_f32, c.inp(w, "weight"), Cout, Cin, 3, o), 0, o
    guard_case(dgr, _same(wd))

    for dgrad in (0, 1):
        nbytes = L.tlod_conv_pack_bs_bytes(Cout, Cin, 3, dgrad)
        ref = tcb._ref_pack(w, bool(dgrad))
        refs = tcb._ref_pack(w * sc.view(-1, 1, 1, 1), bool(dgrad))
        assert ref.numel() * 2 == nbytes

        def bs(c, over):
            o = c.out((nbytes // 2,), torch.int16, "packed")
            return c.run(L.tlod_conv_pack_bs, c.inp(w, "weight"), Cout, Cin, 3, dgrad, o), 0, o
        guard_case(bs, _same(ref))

        def bsx(c, over):
            o = c.out((nbytes // 2,), torch.int16, "packed")
            st = c.run(L.tlod_conv_pack_bs_ex, c.inp(w, "weight"), c.inp(sc, "scale"), Cout, Cin, 3,
                       dgrad, o)
            return st, 0, o
        guard_case(bsx, _same(refs))


def test_small_forward_convs():
    """tlod_conv3x3_direct_f32 (Cin <= 4), tlod_conv1x1_small_fwd_f32, tlod_stem_conv7x7s2_f32,
    tlod_conv_fwd_bs_pool_f32 at odd map sizes."""
    import test_resnet_gpu as trn
    L = lib()
    gen = torch.Generator().manual_seed(8)
    N, Cin, Cout, H, W = 3, 4, 20, 9, 7
    x = torch.randn(N, Cin, H, W, generator=gen) * 50
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) * 0.2
    b = torch.randn(Cout, generator=gen)

    def direct(c, over):
        y = c.out((N, Cout, H, W), f32, "y")
        st = c.run(L.tlod_conv3x3_direct_f32, c.inp(x, "x"), c.inp(w, "weight"), c.inp(b, "bias"),
                   y, N, Cin, H, W, Cout, 1)
        return st, 0, y

    def vd(y):  # the bar of test_conv3x3_direct
        ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=1))
        assert float((y.payload.double().cpu() - ref).norm() / ref.norm()) < 1e-6
    guard_case(direct, vd)

    n1, c1, h1, w1, co1 = 3, 33, 5, 7, 4
    x1 = torch.randn(n1, c1, h1, w1, generator=gen)
    wt1 = torch.randn(co1, c1, generator=gen) * 0.05
    b1 = torch.randn(co1, generator=gen)

    def small(c, over):
        y = c.out((n1, co1, h1, w1), f32, "y")
        st = c.run(L.tlod_conv1x1_small_fwd_f32, c.inp(x1, "x"), n1, c1, h1, w1, c.inp(wt1, "w"),
                   c.inp(b1, "bias"), co1, y)
        return st, 0, y
    guard_case(small, lambda y: tcs._close(y.payload, F.conv2d(
        x1.double(), wt1.double().view(co1, c1, 1, 1), b1.double())))

    Hs, Ws = 37, 51
    xs = torch.randn(2, 3, Hs, Ws, generator=gen) * 50
    wsm = torch.randn(64, 3, 7, 7, generator=gen) * 0.05
    scs, bss = torch.rand(64, generator=gen) + 0.5, torch.randn(64, generator=gen) * 0.1
    Ho, Wo = (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1

    def stem(c, over):
        y = c.out((2, 64, Ho, Wo), f32, "y")
        st = c.run(L.tlod_stem_conv7x7s2_f32, c.inp(xs, "x"), c.inp(wsm, "weight"),
                   c.inp(scs, "scale"), c.inp(bss, "bias"), y, 2, Hs, Ws, 1)
        return st, 0, y

    def vs(y):
        ref = F.relu(F.conv2d(xs.double(), wsm.double(), stride=2, padding=3)
                     * scs.double().view(1, -1, 1, 1) + bss.double().view(1, -1, 1, 1))
        assert tuple(ref.shape) == y.shape
        trn._close(y.payload, ref)
    guard_case(stem, vs)

    d = conv_data(1, 130, 132, 9, 33, 3)

    def pool(c, over):
        y = c.out((1, 132, 4, 16), f32, "y_pooled")
        st = c.run(L.tlod_conv_fwd_bs_pool_f32, c.inp(d["x"], "x"), c.inp(d["wp_fwd"], "wp"), None,
                   c.inp(d["b"], "bias"), y, 1, 130, 9, 33, 132, 3, 1, 6)
        return st, 0, y

    def vp(y):  # the bar of test_conv_epilogue_pool
        ref = F.max_pool2d(F.relu(d["y"] + d["b"].double().view(1, -1, 1, 1)), 2, 2)
        assert float((y.payload.double().cpu() - ref).norm() / ref.norm()) < 1e-5
    guard_case(pool, vp)


def test_plain_permutations():
    """maxpool2x2, subsample2, im2col3x3_nhwc, space_to_depth: bit-exact, odd / ragged maps."""
    L = lib()
    gen = torch.Generator().manual_seed(9)
    N, C, H, W = 2, 5, 7, 9
    x = torch.randn(N, C, H, W, generator=gen)

    def mp(c, over):
        y = c.out((N, C, H // 2, W // 2), f32, "y")
        return c.run(L.tlod_maxpool2x2_f32, c.inp(x, "x"), N, C, H, W, y), 0, y
    guard_case(mp, _same(F.max_pool2d(x, 2, 2)))

    def sub(c, over):
        y = c.out((N, C, (H + 1) // 2, (W + 1) // 2), f32, "y")
        return c.run(L.tlod_subsample2_f32, c.inp(x, "x"), N, C, H, W, y), 0, y
    guard_case(sub, _same(x[:, :, ::2, ::2].contiguous()))

    s = 3
    Ho, Wo = H // s, W // s

    def s2d(c, over):
        y = c.out((N, C * s * s, Ho, Wo), f32, "y")
        return c.run(L.tlod_space_to_depth_f32, c.inp(x, "x"), N, C, H, W, s, y), 0, y
    guard_case(s2d, _same(F.pixel_unshuffle(x[:, :, :Ho * s, :Wo * s], s)))

    R, Hm, Wm, Cm = 3, 2, 7, 12
    xm = torch.randn(R, Hm, Wm, Cm, generator=gen)
    pad = F.pad(xm, (0, 0, 1, 1, 1, 1))
    ref = torch.cat([pad[:, kh:kh + Hm, kw:kw + Wm, :] for kh in range(3) for kw in range(3)],
                    3).reshape(R * Hm * Wm, 9 * Cm)

    def i2c(c, over):
        col = c.out((R * Hm * Wm, 9 * Cm), f32, "col")
        return c.run(L.tlod_im2col3x3_nhwc_f32, c.inp(xm, "x"), R, Hm, Wm, Cm, col), 0, col
    guard_case(i2c, _same(ref))


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_relu_dropout(p):
    """n is no multiple of the float4 width; the claims of test_relu_dropout_fused."""
    L = lib()
    n = 4099
    gen = torch.Generator().manual_seed(10)
    y = torch.randn(n, generator=gen)
    dout = torch.randn(n, generator=gen)
    aux = {}

    def fwd(c, over):
        out = c.out((n,), f32, "out")
        return c.run(L.tlod_relu_dropout_f32, c.inp(y, "y"), out, n, p, 123), 0, out

    def vf(o):
        out = o.payload.cpu()
        pos, kept = y > 0, out > 0
        if p == 0.0:
            assert torch.equal(out, torch.relu(y))
        else:
            assert not bool((kept & ~pos).any()) and not bool(out[~kept].any())
            assert torch.equal(out[kept], y[kept] * 2.0)
            assert 0.4 < float(kept.sum()) / float(pos.sum()) < 0.6
        aux["out"] = out.clone()
    guard_case(fwd, vf)

    def bwd(c, over):
        g = c.out((n,), f32, "g")
        st = c.run(L.tlod_relu_dropout_bwd_f32, c.inp(dout, "dout"), c.inp(aux["out"], "out"), g,
                   n, p)
        return st, 0, g
    want = torch.where(aux["out"] > 0, dout / (1 - p) if p else dout, torch.zeros(n))
    guard_case(bwd, _same(want))


def test_forward_losses():
    """tlod_rpn_loss_f32 and tlod_rcnn_loss_f32 write loss, count, cls_prob and bbox_sel."""
    from tlod.detector.losses import masked_cross_entropy, smooth_l1_loss
    from tlod.rpn.rpn_head import _RPN
    L = lib()
    B, A, H, W = 2, 9, 5, 7
    score, bbox, lab, tgt, inside, outside = (x.cpu() for x in tlo.rpn_inputs(B, A, H, W, 2005))
    scores = _RPN.reshape(score, 2).permute(0, 2, 3, 1).contiguous().view(-1, 2)
    rc = masked_cross_entropy(scores, lab.view(B, -1).view(-1))
    rb = smooth_l1_loss(bbox, tgt, inside, outside, sigma=3, dim=[1, 2, 3])

    def rpn(c, over):
        loss, count = c.out((2,), f32, "loss"), c.out((1,), f32, "count")
        st = c.run(L.tlod_rpn_loss_f32, c.inp(score, "score"), c.inp(lab, "labels"),
                   c.inp(bbox, "bbox"), c.inp(tgt, "targets"), c.inp(inside, "inside"),
                   c.inp(outside, "outside"), B, A, H, W, 3.0, loss, count)
        return st, 0, (loss, count)

    def vr(o):
        loss = o[0].payload.cpu()
        tlo.close(loss[:1], rc.reshape(1))
        tlo.close(loss[1:], rb.reshape(1))
        assert float(o[1].payload.cpu()) == max(float((lab != -1).sum()), 1.0)
    guard_case(rpn, vr)

    R, C = 37, 9
    gen = torch.Generator().manual_seed(R + C)
    cls = torch.randn(R, C, generator=gen) * 2
    box = torch.randn(R, 4 * C, generator=gen)
    rl = torch.randint(0, C, (R,), generator=gen)
    rl[: R // 4] = 0
    rt = torch.randn(R, 4, generator=gen) * 0.5
    iw = (rl > 0).float()[:, None].expand(R, 4).contiguous()
    bp = torch.gather(box.view(R, C, 4), 1, rl.view(-1, 1, 1).expand(-1, 1, 4)).squeeze(1)

    def rcnn(c, over):
        prob, sel, loss = c.out((R, C), f32, "cls_prob"), c.out((R, 4), f32, "bbox_sel"), \
            c.out((2,), f32, "loss")
        st = c.run(L.tlod_rcnn_loss_f32, c.inp(cls, "cls_score"), c.inp(box, "bbox_pred"),
                   c.inp(rl, "labels"), c.inp(rt, "targets"), c.inp(iw, "inside"),
                   c.inp(iw.clone(), "outside"), R, C, 0, 1.0, prob, sel, loss)
        return st, 0, (prob, sel, loss)

    def vc(o):
        tlo.close(o[0].payload.cpu(), F.softmax(cls, 1))
        assert torch.equal(o[1].payload.cpu(), bp)
        loss = o[2].payload.cpu()
        tlo.close(loss[:1], F.cross_entropy(cls, rl).reshape(1))
        tlo.close(loss[1:], smooth_l1_loss(bp, rt, iw, iw).reshape(1))
    guard_case(rcnn, vc)


def test_pt_maf_maps_and_masks():
    import test_pt_maf_ops_gpu as tpm
    L = lib()
    B, A, H, W = 2, 3, 5, 7
    prob = tpm._prob(B, A, H, W, "structured")

    def maps(c, over):
        f, b, stats = c.out((B, H, W), f32, "f"), c.out((B, H, W), f32, "b"), \
            c.out((B, 5), f32, "stats")
        st = c.run(L.tlod_fgbg_maps_f32, c.inp(prob, "prob"), B, A, H, W, tpm.HIGH, tpm.LOW, f, b,
                   stats)
        return st, 0, (f, b, stats)

    def vm(o):
        f, b, stats = (x.payload.cpu() for x in o)
        for i in range(B):
            rf, rb, m, ratio_f, ratio_b = tpm.ref_maps(prob[i:i + 1], A, tpm.HIGH, tpm.LOW)
            assert torch.equal(f[i], rf[0]) and torch.equal(b[i], rb[0])
            assert torch.equal(stats[i], torch.stack([m, rf.sum(), rb.sum(), ratio_f, ratio_b]))
    guard_case(maps, vm)

    rows, num = tpm.MASK_CASES["last"]  # the last row and column of the map
    gt = tpm._boxes(rows)
    Hm, Wm = 12, 20

    def mask(c, over):
        g = c.out((Hm, Wm), f32, "g")
        st = c.run(L.tlod_gt_cell_mask_f32, c.inp(gt, "gt_boxes"),
                   c.inp(torch.tensor([num], dtype=i64), "num_boxes"), gt.shape[1], Hm, Wm, g)
        return st, 0, g
    guard_case(mask, _same(tpm.ref_mask(gt, num, Hm, Wm)))


# ===================================================================== TLOD_WS_GUARD=1
def test_ws_guard_mode_wrappers(monkeypatch):
    """tlod._lib.workspace under TLOD_WS_GUARD=1: every wrapper that takes scratch runs once with
    an exact-length view between canaries (one call per workspace name), then the canaries are
    checked."""
    from tlod import _lib
    from tlod.conv import Conv1x1SmallFunction, conv_dgrad, conv_fwd, conv_wgrad
    from tlod.linear import gemm, gemm_nhwc3
    from tlod.nms import nms
    from tlod.roi_align import RoIAlignAvg, roi_align_avg_s2_nhwc
    from tlod.rpn.anchor_target import anchor_target
    from tlod.rpn.proposal import proposal
    from tlod.rpn.proposal_target import proposal_target
    from helpers import clustered_boxes, rpn_outputs, sorted_dets
    monkeypatch.setenv("TLOD_WS_GUARD", "1")
    assert _lib.check_workspace_guards() >= 0  # start from an empty list
    cu = lambda a: (torch.from_numpy(a) if isinstance(a, np.ndarray) else a).cuda()
    d = conv_data(*SPLIT, 3)
    conv_fwd(cu(d["x"]), cu(d["w"]), cu(d["b"]), math="bf16x6")          # "conv"
    conv_dgrad(cu(d["gy"]), cu(d["w"]), math="f32")
    conv_wgrad(cu(d["gy"]), cu(d["x"]), 3, math="bf16x6")                # "wgrad"
    conv_wgrad(cu(d["gy"]), cu(d["x"]), 3, math="f32")
    g = gemm_data(*GEMM_SPLIT)
    gemm(cu(g["A"]), cu(g["B"]), *GEMM_SPLIT, 1, 1, cu(g["bias"]))        # "gemm"
    n3 = nhwc3_data(*NHWC3_SHAPES[0])
    gemm_nhwc3(0, cu(n3["x"]), cu(n3["wm"]), *NHWC3_SHAPES[0])
    xs = torch.randn(2, 64, 8, 12, device="cuda", requires_grad=True)
    ws_ = torch.randn(3, 64, 1, 1, device="cuda", requires_grad=True)
    Conv1x1SmallFunction.apply(xs, ws_, None).sum().backward()            # "conv1x1_small"
    rng = np.random.default_rng(0)
    nms(cu(sorted_dets(clustered_boxes(rng, 300), rng)), 0.5)             # "nms"
    A = trp.BASE.shape[0]
    prob, deltas = rpn_outputs(rng, 2, A, 5, 7)
    info = np.array([[80, 112, 1.0]] * 2, np.float32)
    base = np.ascontiguousarray(trp.BASE, np.float32)
    proposal(cu(prob), cu(deltas), cu(info), cu(base), 16, 600, 300, 0.7)  # "proposal"
    B, H, W, G, seed, gts, im_info, abase, cs = _anchor_setup()
    anchor_target(cu(abase), H, W, 16, cu(gts), cu(im_info), cs, seed=seed)  # "anchor_target"
    pB, pR, pG, pgt, prois, pcs = _ptarget_setup()
    proposal_target(cu(prois), cu(pgt), pcs, seed=1)                      # "proposal_target"
    feat, rois, _ = roi_data()
    f = cu(feat).requires_grad_(True)
    RoIAlignAvg(7, 7, SCALE)(f, cu(rois)).sum().backward()                # "roi_align_bwd"
    f2 = cu(feat).requires_grad_(True)
    roi_align_avg_s2_nhwc(f2, cu(rois), 7, 7, SCALE).sum().backward()     # "roi_align_s2"
    names = {name for name, _, _ in _lib._ws_guarded}
    assert {"conv", "wgrad", "gemm", "conv1x1_small", "nms", "proposal", "anchor_target",
            "proposal_target", "roi_align_bwd", "roi_align_s2"} <= names, names
    for name, buf, n in _lib._ws_guarded:
        assert buf.numel() == n + 2 * _lib.WS_CANARY_BYTES
    assert _lib.check_workspace_guards() >= 12
    assert not _lib._ws_guarded
