"""The 16-B epilogue of the warp-specialised 3x3 kernel, bit for bit, on both of its store
paths, and the GEMM shapes that were measured with the same epilogue.

The kernel passes the pixel fragment as the MFMA's A operand, so a lane's four accumulator
registers are four consecutive pixels of one channel.  A whole ("direct") tile stores a group
that is a run with one 16-B store and a group that straddles a tile-row end, the tile's end or
the map's right edge per element (`ws_group`); a split-K piece stores 16 B per lane into its
slab and `fwd_tail_reduce_kernel` writes the map.  Which of the two a launch takes is the
planner's choice (`plan_schedule`): a grid of fewer tiles than the chip has workgroup slots is
split over K entirely.  So every map runs twice (tiles as ws_tile picks them):

  map       tiles                                       slab cases      direct cases (fwd)
  16 x 35   13 x 35: TW % 4 = 3, ragged second row      (1, 64, 72)     (1, 64, 8136)
  20 x 39   13 x 39: groups straddling tile-row ends    (1, 64, 64)     (1, 64, 8192)
  9 x 34    one 9 x 34 tile: TW % 4 = 2                 (1, 128, 80)    (1, 64, 16328)
  7 x 75    7 x 73: two column tiles, a 2-pixel one     (2, 64, 64)     (2, 64, 4096)
  30 x 3    narrower than a group: all groups partial   (1, 64, 64)     (1, 64, 8192)

(N, Cin, Cout; the input-gradient cases swap the channel counts.)  The slab cases are small
grids (2-4 tiles): the planner splits every tile, so they pin the 16-B slab stores, ragged
Cout included.  The direct cases have exactly 256 tiles of 64 output channels — one per
workgroup slot of the MI355X, the smallest grid the planner leaves whole — so every tile runs
the direct epilogue: the run / partial stores, and in the masked and the scale + bias +
residual + ReLU cases the 16-B and per-element operand loads.  8136 and 16328 leave 8
channels in the last 16-channel block.  run_ws asserts the route either way, by the
workspace query the planner answers (0 bytes: no tile is split).
The pool case (1, 64, 128, 33, 31) runs the pooling epilogue (never split): the 8-B pooled
stores at an odd pooled width (15).

The GEMM (gemm.hip) keeps its per-element epilogue: the same operand swap measured slower
there.  Its cases stay as a pin of the shapes that swap was tried on —
N % 4 != 0 and N % 4 == 0, ragged M, with bias / residual / ReLU / mask — in every layout.

Operands from tests/exact_inputs.py (every sum exact in 24 bits): the result must be
torch.equal to the fp64 reference, no tolerance.  Every conv case writes into an output carved
out of a poisoned, guard-banded buffer (tests/abi_guard.py): a store past the tensor damages a
guard, an element never stored keeps its poison.  tests/test_wide_epilogue_cpu.py proves the
exactness conditions of these cases and, on the kernel's own store plan, that the direct
epilogue writes every element exactly once.
"""
import pytest
import torch
import torch.nn.functional as F

import abi_guard as ag
import exact_inputs as E
from test_gemm_exact_gpu import LAYOUTS, run_gemm, run_gemm_mask

pytestmark = pytest.mark.gpu
dev = "cuda"

MODES = E.BS_MODES[:3]  # 24x8 and 16x16 under bf16x6, 16x8 under bf16x3
# N, Cin, Cout, H, W
WS = [(1, 64, 72, 16, 35), (1, 64, 64, 20, 39), (1, 128, 80, 9, 34), (2, 64, 64, 7, 75),
      (1, 64, 64, 30, 3)]
# the same maps with 256 tiles (tiles per image x N x ceil(Cout / 64)): whole tiles only
WS_DIRECT = [(1, 64, 8136, 16, 35), (1, 64, 8192, 20, 39), (1, 64, 16328, 9, 34),
             (2, 64, 4096, 7, 75), (1, 64, 8192, 30, 3)]
POOL = (1, 64, 128, 33, 31)
GEMMS = [(70, 130, 96), (200, 260, 64), (77, 132, 48)]  # N % 4 != 0 first: the fallback


def _pool(v):
    return F.max_pool2d(v, 2, 2)


CASES = []
for _s in WS:
    CASES += [E.Case("ws_fwd", E.conv_op, ("fwd",) + _s, modes=MODES),
              E.Case("ws_dgrad", E.conv_op, ("dgrad",) + _s, modes=MODES)]
CASES += [E.Case("ws_dgrad", E.conv_op, ("dgrad",) + WS[0], epi="m", modes=MODES),
          E.Case("ws_fwd", E.conv_op, ("fwd",) + WS[2], epi="sbra", modes=MODES),
          E.Case("ws_pool", E.conv_op, ("fwd",) + POOL, epi="ba", post=_pool, modes=MODES)]


def _swap(s):  # the input gradient's kernel writes the layer's Cin channels
    return (s[0], s[2], s[1]) + s[3:]


for _s in WS_DIRECT:
    CASES += [E.Case("wsd_fwd", E.conv_op, ("fwd",) + _s, modes=MODES),
              E.Case("wsd_dgrad", E.conv_op, ("dgrad",) + _swap(_s), modes=MODES)]
CASES += [E.Case("wsd_dgrad", E.conv_op, ("dgrad",) + _swap(WS_DIRECT[0]), epi="m", modes=MODES),
          E.Case("wsd_fwd", E.conv_op, ("fwd",) + WS_DIRECT[2], epi="sbra", modes=MODES)]
CASES += [E.Case("gemm", E.gemm_op, s, arg=l, modes=MODES) for s in GEMMS for l in LAYOUTS]
# the 16-B bias / residual / mask loads (N % 4 == 0) and their per-element form
CASES += [E.Case("gemm", E.gemm_op, s, epi="bra", arg=(1, 1), modes=MODES) for s in GEMMS]
CASES += [E.Case("gemm_mask", E.gemm_op, s, epi="rm", arg=(1, 0), modes=MODES) for s in GEMMS[:2]]

PARAMS, IDS = E.expand(CASES)


def _p(t):
    from tlod import _lib
    return None if t is None else _lib.ptr(t)


def _d(t):
    return None if t is None else t.to(dev).contiguous()


def run_ws(case, A, B, epi, op, math):
    """tlod_conv_fwd_bs_f32 / tlod_conv_dgrad_bs_mask_f32 / tlod_conv_fwd_bs_pool_f32 through
    the raw ABI into a guarded output.  The input gradient is the forward form over dy with
    the transposed, flipped pack (Cin := the layer's Cout)."""
    from tlod import _lib
    from tlod.conv import _gemm_conv, pack_bs
    kind, N, Cin, Cout, H, W = case.key
    dgrad = kind == "dgrad"
    cin, cout = (Cout, Cin) if dgrad else (Cin, Cout)
    assert cin >= 64 and not _gemm_conv(3, math, cout)  # the warp-specialised kernel's range
    L = _lib.lib()
    nprod = 6 if math == "bf16x6" else 3
    x, wp = _d(A), pack_bs(B.to(dev), dgrad)
    sc, b, res, mask = (_d(getattr(epi, k, None)) for k in ("scale", "bias", "residual", "mask"))
    relu = int(bool(epi and epi.relu))
    c = ag.Call()
    if case.path == "ws_pool":
        y = c.out((N, cout, H // 2, W // 2), name="y_pooled")
        st = c.run(L.tlod_conv_fwd_bs_pool_f32, _p(x), _p(wp), _p(sc), _p(b), y, N, cin, H, W, cout,
                   3, relu, nprod)
    else:
        q = L.tlod_conv_fwd_bs_workspace_bytes(N, cin, H, W, cout, 3, nprod)
        # the route: a direct case splits no tile, a slab case splits (all of) them
        assert (q == 0) if case.path.startswith("wsd_") else (q > 0), (case.id, q)
        ws = c.ws(q)
        wsp = ws.ptr if ws is not None else None
        y = c.out((N, cout, H, W), name="y")
        if mask is not None:
            st = c.run(L.tlod_conv_dgrad_bs_mask_f32, _p(x), _p(wp), _p(mask), y, N, cin, H, W,
                       cout, nprod, wsp, q)
        else:
            st = c.run(L.tlod_conv_fwd_bs_f32, _p(x), _p(wp), _p(sc), _p(b), _p(res), y, N, cin, H,
                       W, cout, 3, relu, nprod, wsp, q)
    assert st == 0, L.tlod_last_error()
    c.check()  # guards intact, no poison left
    return y.payload.clone()


RUN = {"ws_fwd": run_ws, "ws_dgrad": run_ws, "wsd_fwd": run_ws, "wsd_dgrad": run_ws,
       "ws_pool": run_ws, "gemm": run_gemm,
       "gemm_mask": run_gemm_mask}


@pytest.mark.parametrize("case,math,cls,side", PARAMS, ids=IDS)
def test_wide_epilogue_exact(case, math, cls, side):
    E.run_case(case, math, cls, side,
               lambda A, B, epi, op: RUN[case.path](case, A, B, epi, op, math))
