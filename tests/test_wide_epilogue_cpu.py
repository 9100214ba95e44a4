"""The store plan of the warp-specialised 3x3 kernel's 16-B epilogue, checked without a GPU,
and the exactness conditions of tests/test_wide_epilogue_gpu.py's cases.

tlod_conv_ws_store_map (include/tlod_plan.h) replays the whole-tile epilogue on one channel
plane with the kernel's own classification functions and address arithmetic: the direct
epilogue's 16-B / 4-B stores on the H x W map, or (pool) the pooling epilogue's 8-B / 4-B
stores on the (H / 2) x (W / 2) pooled map, the only thing a pooling launch writes.  On the
GPU a wrong wide store can hide behind a later correct store to the same element (a race the
value comparison may not see); here every element must be written exactly once, by one kind
of store, and no store may leave the map or, for a wide store, the row of its first element.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import exact_inputs as E
import test_wide_epilogue_gpu as wide_cases
from conftest import ROOT

# the headline step's maps (600 x 1200 image), the GPU file's shapes, and every small map
BENCH = [(600, 1200, 1), (300, 600, 1), (300, 600, 0), (150, 300, 0), (75, 150, 0), (37, 75, 0)]
SMALL = [(s[3], s[4], 0) for s in wide_cases.WS] + [wide_cases.POOL[3:] + (1,)]
TINY = [(h, w, p) for h in range(1, 13) for w in range(1, 13) for p in (0, 1)
        if not p or (h >= 2 and w >= 2)]


def store_map(H, W, pool):
    from tlod import _lib
    L = _lib.lib()
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)  # the map the epilogue writes
    wide = np.full(Ho * Wo, -1, np.int32)
    single = np.full(Ho * Wo, -1, np.int32)
    tile = np.zeros(2, np.int32)
    stray = ctypes.c_int32(-1)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    st = L.tlod_conv_ws_store_map(H, W, pool, p(wide), p(single), p(tile),
                                  ctypes.cast(ctypes.byref(stray), ctypes.c_void_p))
    assert st == 0, L.tlod_last_error()
    return wide.reshape(Ho, Wo), single.reshape(Ho, Wo), tuple(tile), stray.value


def _check(H, W, pool):
    wide, single, (th, tw), stray = store_map(H, W, pool)
    assert th >= 1 and tw >= 8 and th * tw <= 512
    if pool:
        assert (th, tw) == (16, 32)
    assert stray == 0, f"{H}x{W}: {stray} floats stored outside the map or their run's row"
    total = wide + single
    assert total.min() == 1 and total.max() == 1, \
        f"{H}x{W} tile {th}x{tw}: write counts {np.unique(total)} (first bad at " \
        f"{tuple(np.argwhere(total != 1)[0])})"
    return wide, single, (th, tw)


@pytest.mark.parametrize("H,W,pool", BENCH + SMALL, ids=lambda v: str(v))
def test_every_element_written_once(H, W, pool):
    wide, single, (th, tw) = _check(H, W, pool)
    # a wide store lies in one map row and one tile row: the wide elements of a row come in
    # whole groups of four (pooled map: two) inside each tile's columns
    n, twp = (2, tw // 2) if pool else (4, tw)
    for w0 in range(0, wide.shape[1], twp):
        cols = wide[:, w0:w0 + twp].sum(1)
        assert (cols % n == 0).all()
    if W >= 8:  # the point of the layout: most of the map leaves in wide stores
        assert wide.sum() > single.sum()
    else:
        assert wide.sum() == 0 or W >= 4
    if pool:  # 4-B stores only in an odd pooled width's last column
        assert single[:, :-1].sum() == 0 and single[:, -1].sum() == (H // 2) * ((W // 2) % 2)


def test_every_small_map():
    for H, W, pool in TINY:
        _check(H, W, pool)


def test_map_narrower_than_a_group_has_no_wide_store():
    wide, single, _ = _check(30, 3, 0)
    assert wide.sum() == 0 and single.sum() == 90


def test_query_rejects_bad_arguments():
    from tlod import _lib
    L = _lib.lib()
    buf = (ctypes.c_int32 * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.tlod_conv_ws_store_map(0, 4, 0, p, p, None, p) != 0
    assert L.tlod_conv_ws_store_map(1, 4, 0, None, p, None, p) != 0
    assert L.tlod_conv_ws_store_map(1, 4, 0, p, p, None, None) != 0
    assert L.tlod_conv_ws_store_map(1, 4, 1, p, p, None, p) != 0  # no 2 x 2 window


def test_plan_header_matches_its_table():
    """include/tlod_plan.h == tlod._lib.PLAN_SIGNATURES, disjoint from the other tables, every
    name exported and bound by lib()."""
    from tlod import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tlod_plan.h")).read(),
                 flags=re.S)
    syms = sorted(set(re.findall(r"\b(tlod_[a-z0-9_]+)\s*\(", src)))
    assert syms and sorted(_lib.PLAN_SIGNATURES) == syms
    for other in (_lib.SIGNATURES, _lib.EXT_SIGNATURES, _lib.PA_ATF_SIGNATURES,
                  _lib.ROI_SIGNATURES, _lib.SELFTRAIN_SIGNATURES):
        assert not set(syms) & set(other)
    bound = _lib.lib()
    for s in syms:
        assert getattr(bound, s).argtypes == _lib.PLAN_SIGNATURES[s][1]


# ---------------------------------------------------------------- exactness conditions
def _dedup(key):
    seen, out, ids = set(), [], []
    for p, i in zip(wide_cases.PARAMS, wide_cases.IDS):
        k = key(p)
        if k not in seen:
            seen.add(k)
            out.append(p)
            ids.append(i)
    return out, ids


_COND = _dedup(lambda p: (p[0].id, p[2], p[3]))  # operands: (case, class, dense side)


@pytest.mark.parametrize("case,math,cls,side", _COND[0], ids=_COND[1])
def test_exactness_conditions(case, math, cls, side):
    op, epi = case.build()
    E.check_conditions(op, case.rounds(side), cls, side, case.seed, epi, case.q_extra,
                       case.eff(op))
