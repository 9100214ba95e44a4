"""The guard-band harness (tests/abi_guard.py) must be able to fail: on CPU tensors, with plain
torch writes standing in for a kernel, check() raises for each kind of miswrite and passes
for a correct one.  Plus the ledger: every C ABI entry point is guarded, host-only or
deferred with a reason, so a new one cannot ship unguarded unnoticed; and the split / no-split
shapes of tests/test_abi_guard_gpu.py really query > 0 / == 0 on the CPU build.
"""
import os

import pytest
import torch

import abi_guard as ag
from abi_guard import Call, GuardError

HERE = os.path.dirname(os.path.abspath(__file__))


def _call():
    c = Call(device="cpu")
    x = c.inp(torch.arange(12, dtype=torch.float32).view(3, 4), "x")
    y = c.out((3, 4), torch.float32, "y")
    k = c.out((5,), torch.int32, "keep")
    acc = c.acc(torch.ones(7), "acc")
    ws = c.ws(100)
    return c, x, y, k, acc, ws


def _good(x, y, k, acc, ws):
    y.payload.copy_(x.payload * 2)
    k.payload.copy_(torch.arange(5, dtype=torch.int32))
    acc.payload.add_(1.0)
    ws.payload.fill_(3)


def test_layout():
    c, x, y, k, acc, ws = _call()
    for g in (x, y, k, acc, ws):
        assert (g.buf.data_ptr() + g.off) % 256 == 0
        assert g.end - g.off == g.numel * g.itemsize  # no rounding: the back guard is next
        assert g.off >= 1 << 20 and g.buf.numel() - g.end >= 1 << 20
        assert g.off >= g.nbytes and g.buf.numel() - g.end >= g.nbytes
        assert bool((g.buf[:g.off] == ag.GUARD_BYTE).all())
        assert bool((g.buf[g.end:] == ag.GUARD_BYTE).all())
    assert ws.nbytes == 100 and c.ws(0) is None
    assert torch.isnan(y.payload).all() and bool(y.poisoned().all())
    assert bool((k.payload < -1).all()) and bool(k.poisoned().all())
    big = ag.guarded((600, 1000), torch.float32, "out", device="cpu")
    assert big.off >= big.nbytes > 1 << 20


def test_correct_write_passes():
    c, x, y, k, acc, ws = _call()
    _good(x, y, k, acc, ws)
    c.check()
    assert torch.equal(y.payload, x.initial * 2)


def test_write_one_past_the_payload():
    c, x, y, k, acc, ws = _call()
    _good(x, y, k, acc, ws)
    y.window(after=1)[-1] = 1.0
    with pytest.raises(GuardError, match="y .*back guard"):
        c.check()


def test_write_one_before_the_payload():
    c, x, y, k, acc, ws = _call()
    _good(x, y, k, acc, ws)
    k.window(before=1)[0] = 7
    with pytest.raises(GuardError, match="keep .*front guard"):
        c.check()


def test_workspace_overrun_is_seen_without_rounding():
    c, x, y, k, acc, ws = _call()
    _good(x, y, k, acc, ws)
    ws.window(after=1)[-1] = 0  # byte 100 of a 100-byte workspace
    with pytest.raises(GuardError, match="ws .*back guard, nearest 0 B"):
        c.check()


def test_one_output_element_left_unwritten():
    c, x, y, k, acc, ws = _call()
    _good(x, y, k, acc, ws)
    y.poison()
    y.payload.view(-1)[:11] = 0.0
    with pytest.raises(GuardError, match="y .*1 output elements never written"):
        c.check()


def test_one_input_element_changed():
    c, x, y, k, acc, ws = _call()
    _good(x, y, k, acc, ws)
    x.payload[1, 2] = -0.0 if float(x.payload[1, 2]) == 0.0 else float(x.payload[1, 2]) + 1
    with pytest.raises(GuardError, match="x .*const input changed .1 elements"):
        c.check()


def test_must_stay_untouched_region_written():
    c, x, y, k, acc, ws = _call()
    _good(x, y, k, acc, ws)
    k.poison()
    k.payload[:3] = torch.arange(3, dtype=torch.int32)
    k.untouched = torch.arange(5) >= 3  # keep[num_keep:] of tlod_nms_f32
    c.check()
    k.payload[4] = 0
    with pytest.raises(GuardError, match="keep .*not written were written"):
        c.check()


def test_rejected_call_must_leave_pure_poison():
    c, x, y, k, acc, ws = _call()
    c.check_rejected()
    y.payload[0, 0] = 0.0
    with pytest.raises(GuardError, match="must fail first"):
        c.check_rejected()


# ------------------------------------------------------------------------------ ledger
def test_ledger_covers_every_entry_point():
    from tlod import _lib
    names = set(_lib.SIGNATURES)
    lists = {"GUARDED": ag.GUARDED, "HOST_ONLY": ag.HOST_ONLY, "DEFERRED": list(ag.DEFERRED)}
    seen = {}
    for which, lst in lists.items():
        assert len(lst) == len(set(lst)), which
        for n in lst:
            assert n in names, f"{which}: {n} is not in tlod._lib.SIGNATURES"
            assert n not in seen, f"{n} is in both {seen.get(n)} and {which}"
            seen[n] = which
    missing = sorted(names - set(seen))
    assert not missing, f"entry points in no ledger list (guard them): {missing}"
    host = {n for n in names if n.endswith("_workspace_bytes")} | {
        "tlod_abi_version", "tlod_last_error", "tlod_set_cu_reserve", "tlod_conv_pack_bs_bytes"}
    assert set(ag.HOST_ONLY) == host
    assert set(ag.DEFERRED) <= set(ag.DEFERRABLE)
    for n, why in ag.DEFERRED.items():
        assert isinstance(why, str) and len(why.strip()) > 10 and "\n" not in why, n
    print("DEFERRED:")
    for n, why in sorted(ag.DEFERRED.items()):
        print(f"  {n}: {why}")
    # every GUARDED name is the entry point of a guarded call in the GPU file
    uncalled = sorted(set(ag.GUARDED) - _guarded_calls())
    assert not uncalled, uncalled


def _guarded_calls():
    """Entry points that tests/test_abi_guard_gpu.py passes to Call.run: from its syntax tree,
    L.<name> as the first argument of a .run(...) call, directly or through a local variable
    assigned from L.<name> expressions in the same test (a name in a comment, a string or an
    unused expression does not count)."""
    import ast
    tree = ast.parse(open(os.path.join(HERE, "test_abi_guard_gpu.py")).read())

    def entry_points(node):
        return {n.attr for n in ast.walk(node) if isinstance(n, ast.Attribute)
                and isinstance(n.value, ast.Name) and n.value.id == "L"
                and n.attr.startswith("tlod_")}

    def names(node):
        return {n.id for n in ast.walk(node) if isinstance(n, ast.Name)}

    called = set()
    for fn in tree.body:
        if not isinstance(fn, ast.FunctionDef):
            continue
        assigned = {}
        for n in ast.walk(fn):
            if isinstance(n, ast.Assign):
                for t in n.targets:
                    for v in names(t):
                        assigned.setdefault(v, set()).update(entry_points(n.value))
        for n in ast.walk(fn):
            if (isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)
                    and n.func.attr == "run" and n.args):
                first = n.args[0]
                called |= entry_points(first)
                if isinstance(first, ast.Name):
                    called |= assigned.get(first.id, set())
    return called


def test_split_shapes_split_on_the_cpu_build():
    """Without a device the planners assume 256 slots: the shapes the GPU file runs as "splits"
    query > 0 and the "no split" ones == 0 (run there with NULL, 0)."""
    from tlod import _lib
    import test_abi_guard_gpu as tg
    L = _lib.lib()
    assert L.tlod_set_cu_reserve(0) == 0
    split, nosplit = tg.planner_queries(L)
    assert all(v > 0 for v in split.values()), split
    assert all(v == 0 for v in nosplit.values()), nosplit
    # and the split-tail shape under 248 reserved CUs (8 slots here)
    assert L.tlod_set_cu_reserve(248) == 0
    try:
        tg.tail_plan_query(L)
    finally:
        assert L.tlod_set_cu_reserve(0) == 0


def test_ws_guard_mode_hands_out_exact_views(monkeypatch):
    from tlod import _lib
    monkeypatch.setenv("TLOD_WS_GUARD", "1")
    try:
        a = _lib.workspace(1000, "cpu", "conv")
        b = _lib.workspace(10, "cpu", "nms")
        assert a.numel() == 1000 and b.numel() == 256
        assert a.data_ptr() != _lib.workspace(1000, "cpu", "conv").data_ptr()  # no cache
        a.fill_(0)
        assert _lib.check_workspace_guards() == 3
        c = _lib.workspace(64, "cpu", "wgrad")
        c.fill_(1)
        whole = next(buf for name, buf, n in _lib._ws_guarded if name == "wgrad")
        whole[_lib.WS_CANARY_BYTES + 256] = 0  # the byte right after the view
        with pytest.raises(RuntimeError, match="wgrad .*1 bytes past"):
            _lib.check_workspace_guards()
        assert _lib.check_workspace_guards() == 0  # forgotten
    finally:
        del _lib._ws_guarded[:]
