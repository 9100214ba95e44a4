"""The fused SGD and Adam steps (csrc/optim.hip, tlod.optim) pinned bit for bit to
tests/fused_optim.py.

After each step of every case: the per-chunk partials, the gradient norm and the clip scale
(norm_scale[0:2]), the norm step() returns, and every parameter, momentum buffer, exp_avg,
exp_avg_sq and step count equal the numpy restatement exactly (np.array_equal over every
element).  The one value held to 1 float32 ulp instead is Adam's corr pair, which the device
forms with its own double pow; the expected update is then computed from the device's corr.

  kernel level   descriptor tables handed to tlod_sgd_clip_f32 / tlod_adam_clip_f32: counts
                 around every path boundary (1 .. 65536, the one-, two- and four-element
                 second chunks of 65537, 65538, 65540), gradient and state pointers off the
                 16-byte boundary, grad_scale 1, 0.125 and 1/3, every clip regime, norm-only
                 rows, the device-side active flag, two (lr, weight_decay) groups;
  optimizer      FusedSGDClip / FusedAdamClip with and without the gradient arena: the lr and
                 the weight decay changed between steps, a parameter without a gradient, a
                 step without zero_grad, the 3x3 weights the pack tiles update, a resume from
                 a checkpoint at step 1000.

The cases and their inputs are built in numpy without a GPU (Case, Replay below);
tests/test_fused_optim_cpu.py imports them to hold the restatement to the fp64 truth and to
show that every plausible defect changes some expectation.
"""
import math
import zlib
from collections import namedtuple

import numpy as np
import pytest
import torch

import fused_optim as F

CHUNK = 65536
GROUPS = ((0.01, 5e-4), (0.02, 0.0))  # (lr, weight_decay) of group 0 and group 1
MOMENTUM = 0.9
f32 = np.float32

# One parameter: n elements (shape when the optimizer needs one), its group, the float offsets
# of its gradient and of its state tensors from a 16-byte boundary, norm_only: its rows carry
# negative counts.
T = namedtuple("T", "n group goff soff norm_only shape", defaults=(0, 0, (0, 0), False, None))


class Case:
    """clip: ("abs", c) | ("over", r): the first step's gradient norm is about r times the
    clip | ("hot", c): every gradient is zero but one element equal to c.
    inactive / nograd: {step: parameter indices}; lr_mul / wd_set: {step: ...} applied before
    that step; keep_grad: steps taken without zero_grad (the gradients accumulate); gmul: a
    factor on each step's gradients; warm: start from nonzero state at step count t0."""

    def __init__(self, name, tensors, gs=1.0, clip=("abs", 10.0), level="kernel", nsteps=3,
                 inactive=None, nograd=None, lr_mul=None, wd_set=None, keep_grad=(),
                 gmul=None, warm=False, t0=0, packs=False):
        self.name, self.tensors, self.level, self.nsteps = name, tensors, level, nsteps
        assert [t.group for t in tensors] == sorted(t.group for t in tensors)
        self.gs = float(f32(gs))
        self.inactive, self.nograd = inactive or {}, nograd or {}
        self.lr_mul, self.wd_set, self.keep_grad = lr_mul or {}, wd_set or {}, keep_grad
        self.warm, self.t0, self.packs = warm, t0, packs
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.params = [(0.05 * rng.standard_normal(t.n)).astype(np.float32) for t in tensors]
        self.state0 = [[np.zeros(t.n, np.float32)] * 2 for t in tensors]
        if warm:
            self.state0 = [[(1e-3 * rng.standard_normal(t.n)).astype(np.float32),
                            (1e-6 * rng.standard_normal(t.n) ** 2 + 1e-12).astype(np.float32)]
                           for t in tensors]
        gmul = gmul or [1.0] * nsteps
        self.raw = []  # what each step's backward produces
        for s in range(nsteps):
            row = []
            for i, t in enumerate(tensors):
                g = rng.standard_normal(t.n) * np.logspace(-6, 1, t.n) * gmul[s]
                if clip[0] == "hot":
                    g = np.zeros(t.n)
                    if i == s % len(tensors):
                        g[(7 * s) % t.n] = clip[1]
                if i in self.inactive.get(s, ()):
                    g = np.zeros(t.n)  # no rank produced it: the slot holds zeros
                row.append(None if i in self.nograd.get(s, ()) else g.astype(np.float32))
            self.raw.append(row)
        if clip[0] == "over":
            tot = math.sqrt(sum(float(((g.astype(np.float64) * self.gs) ** 2).sum())
                                for g in self.raw[0] if g is not None))
            self.clip = float(f32(tot / clip[1]))
        else:
            self.clip = float(f32(clip[1]))

    def grads(self, s):
        """The gradients step s reads: the step's own, added in float32 to what the earlier
        step left when no zero_grad came in between (AccumulateGrad's in-place add)."""
        if s in self.keep_grad:
            return [b if a is None else a if b is None else a + b
                    for a, b in zip(self.grads(s - 1), self.raw[s])]
        return self.raw[s]

    def __repr__(self):
        return self.name


def group_hparams(case, s):
    """[(lr, weight_decay)] of the groups at step s."""
    out = [list(g) for g in GROUPS]
    for k in range(s + 1):
        for g in out:
            g[0] *= case.lr_mul.get(k, 1.0)
        for gi, wd in case.wd_set.get(k, {}).items():
            out[gi][1] = wd
    return out


def table_layout(case, s):
    """[(parameter index, float offset, signed count, vec of the norm)] in table order: every
    parameter that has a gradient, chunk after chunk."""
    rows = []
    grads = case.grads(s)
    for i, t in enumerate(case.tensors):
        if grads[i] is None:
            continue
        for off in range(0, t.n, CHUNK):
            c = min(CHUNK, t.n - off)
            rows.append((i, off, -c if t.norm_only else c, t.goff % 4 == 0 and c % 4 == 0))
    return rows


class Replay:
    """The restatement run over a case, one step at a time."""

    def __init__(self, case, kind):
        self.case, self.kind = case, kind
        self.nstate = 1 if kind == "sgd" else 2
        self.params = [p.copy() for p in case.params]
        self.state = [[a.copy() for a in st[:self.nstate]] for st in case.state0]
        self.counts = {i: case.t0 for i in range(len(case.tensors))} if case.t0 else {}
        self.corr = {}

    def step(self, s, corr_given=None):
        """Advance by step s; returns (fused_optim.Result, table layout)."""
        case = self.case
        hp, grads, layout = group_hparams(case, s), case.grads(s), table_layout(case, s)
        dead = case.inactive.get(s, ())
        rows = []
        for i, off, c, vec in layout:
            sl = slice(off, off + abs(c))
            lr, wd = hp[case.tensors[i].group]
            active = None if not case.inactive else 0.0 if i in dead else 1.0
            rows.append(F.Row(i, self.params[i][sl], grads[i][sl],
                              tuple(a[sl] for a in self.state[i]), c, lr, wd, active, vec))
        res = F.step(self.kind, rows, case.gs, case.clip, momentum=MOMENTUM, counts=self.counts,
                     corr=self.corr, corr_given=corr_given)
        for (i, off, c, _), new in zip(layout, res.rows):
            sl = slice(off, off + abs(c))
            self.params[i][sl] = new[0]
            for a, b in zip(self.state[i], new[1:]):
                a[sl] = b
        self.counts, self.corr = res.counts, res.corr
        return res, layout

    def snapshot(self):
        out = [p.copy() for p in self.params] + [a.copy() for st in self.state for a in st]
        if self.kind == "adam":
            out.append(np.array([self.counts.get(i, 0) for i in range(len(self.params))]))
        return out


def run_expected(case, kind):
    """Everything the GPU test compares, step after step, as a flat list of arrays."""
    rp, out = Replay(case, kind), []
    for s in range(case.nsteps):
        res, _ = rp.step(s)
        out += [res.partials, np.array([res.total, res.scale])] + rp.snapshot()
        if kind == "adam":
            out.append(np.array([res.corr.get(i, (0, 0)) for i in range(len(rp.params))],
                                dtype=np.float32))
    return out


# ------------------------------------------------------------------ the cases
def _alt(ns):
    """Parameters of the given sizes, the first half in group 0, the rest in group 1."""
    return [T(n, int(i >= (len(ns) + 1) // 2)) for i, n in enumerate(ns)]


KERNEL_CASES = [
    # every count at which a path begins or ends: 1 .. 4 (the vector path starts at 4), one
    # round of 256 threads and one element either side, one round of float4s and one float4
    # more, a full chunk and one element either side, a second chunk of 1, 2 and 4 elements
    Case("counts", [T(n, g) for n, g in [(1, 0), (4, 0), (256, 0), (1024, 0), (65535, 0),
                                         (65537, 0), (65540, 0), (3, 1), (255, 1), (257, 1),
                                         (1028, 1), (65536, 1), (65538, 1)]],
         gs=1 / 3, clip=("over", 1.5)),
    Case("grad_misaligned", [T(1024, 0, 1), T(1024, 0, 2), T(8, 0, 3), T(1024, 1, 3),
                             T(1024, 1, 0)], gs=0.125, clip=("over", 1e4)),
    Case("state_misaligned", [T(1024, 0, 0, (1, 0)), T(1024, 0, 0, (0, 2)), T(8, 1, 0, (3, 3)),
                              T(1024, 1, 0, (2, 1))], gs=1.0, clip=("abs", 1e4)),
    Case("total_eq_clip", _alt([1000, 1028, 257]), gs=1.0, clip=("hot", 0.75)),
    Case("norm_only", [T(4096, 0, norm_only=True), T(65540, 0, norm_only=True), T(1000, 0),
                       T(300, 1), T(1027, 1, norm_only=True)], gs=1 / 3, clip=("over", 1.5)),
    Case("inactive", [T(5000, 0), T(300, 0), T(1028, 0), T(257, 1)], gs=1 / 3,
         clip=("over", 1.5), inactive={0: (1,), 1: (2,)}),
]
# grad_scale x clip regime on a vector and a scalar chunk per group
for _gs, _gn in ((1.0, "1"), (0.125, "8th"), (1 / 3, "3rd")):
    for _clip, _cn in ((("abs", 1e4), "under"), (("over", 1.5), "over1.5"),
                       (("over", 1e4), "over1e4"), (("abs", 0.0), "off")):
        KERNEL_CASES.append(Case(f"gs_{_gn}_clip_{_cn}", _alt([1000, 257, 260, 127]), gs=_gs,
                                 clip=_clip))

OPTIM_CASES = [
    # lr decayed before the second step, parameter 1 (2310 elements: not a multiple of 4)
    # without a gradient in it, the third taken without zero_grad; clip = 10 bites in the
    # first step (norm ~ 100) and not in the second (gradients 100 times smaller)
    Case("schedule", [T(1200, 0, shape=(40, 30)), T(2310, 0, shape=(70, 33)),
                      T(30, 1, shape=(30,)), T(33, 1, shape=(33,))], level="optim",
         nograd={1: (1,)}, lr_mul={1: 0.1}, keep_grad=(2,), gmul=[1.0, 0.01, 1.0]),
    Case("wd_change", [T(1200, 0, shape=(40, 30)), T(30, 1, shape=(30,))], level="optim",
         wd_set={1: {0: 1e-3, 1: 1e-4}}),
    Case("packs", [T(432, 0, shape=(16, 3, 3, 3)), T(19305, 0, shape=(33, 65, 3, 3)),
                   T(8640, 0, shape=(40, 24, 3, 3)), T(40, 1, shape=(40,))], level="optim",
         packs=True),
    Case("resume_t1000", [T(1200, 0, shape=(40, 30)), T(33, 1, shape=(33,))], level="optim",
         nsteps=2, warm=True, t0=1000),
]
CASES = KERNEL_CASES + OPTIM_CASES
KINDS = ("sgd", "adam")


def ulps(a, b):
    """|a - b| in float32 ulps, for finite values of one sign."""
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


# ------------------------------------------------------------------ on the device
dev = "cuda"


def _same(got, want, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got.ravel() != want.ravel())
        raise AssertionError(f"{what}: {bad.size} of {got.size} elements differ, first at "
                             f"{bad[0]}: device {got.ravel()[bad[0]]!r} restatement "
                             f"{want.ravel()[bad[0]]!r}")


def _view(arr, off):
    """A device copy of arr that starts off floats past a 16-byte boundary."""
    base = torch.zeros(arr.size + 4, dtype=torch.float32, device=dev)
    assert base.data_ptr() % 16 == 0
    v = base[off:off + arr.size]
    v.copy_(torch.from_numpy(arr))
    return v


def _check_corr(corr_dev, res, live, what):
    """The device's corr pairs of the parameters that advanced: within 1 ulp of adam_corr."""
    worst = 0
    for i in live:
        worst = max(worst, int(ulps(corr_dev[i], np.array(res.corr[i], np.float32)).max()))
    print(f"{what}: corr within {worst} ulp of the host's")
    assert worst <= 1, what


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", KERNEL_CASES, ids=repr)
def test_kernel_level(case, kind):
    """A descriptor table through tlod_sgd_clip_f32 / tlod_adam_clip_f32, three calls."""
    from tlod import _lib
    from tlod.optim import _ADAM_DESC, _ADAM_STATE, _DESC
    rp = Replay(case, kind)
    ts = case.tensors
    P = [_view(p, 0) for p in case.params]
    G = [_view(np.zeros(t.n, np.float32), t.goff) for t in ts]
    S = [[_view(a, t.soff[j]) for j, a in enumerate(st[:rp.nstate])]
         for t, st in zip(ts, case.state0)]
    active = torch.ones(len(ts), device=dev)
    steps = torch.zeros(len(ts), dtype=torch.int32, device=dev)
    corr = torch.zeros(len(ts), 2, device=dev)
    layout = table_layout(case, 0)
    hp = group_hparams(case, 0)
    rows = []
    for i, off, c, vec in layout:
        lr, wd = hp[ts[i].group]
        ap = active.data_ptr() + 4 * i if case.inactive else 0
        ptrs = [P[i].data_ptr() + 4 * off, G[i].data_ptr() + 4 * off] + \
            [s.data_ptr() + 4 * off for s in S[i]]
        # the restatement is told the path the pointers imply
        assert vec == (ptrs[1] % 16 == 0 and abs(c) % 4 == 0)
        tail = (c, lr, wd, ap) + ((corr.data_ptr() + 8 * i,) if kind == "adam" else ())
        rows.append(tuple(ptrs) + tail)
    up = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to(dev)
    chunks = up(np.array(rows, dtype=_DESC if kind == "sgd" else _ADAM_DESC))
    states = up(np.array([(steps.data_ptr() + 4 * i,
                           active.data_ptr() + 4 * i if case.inactive else 0,
                           corr.data_ptr() + 8 * i) for i in range(len(ts))], dtype=_ADAM_STATE))
    partials = torch.empty(len(rows), device=dev)
    norm_scale = torch.zeros(2, device=dev)
    L = _lib.lib()
    scales = []
    for s in range(case.nsteps):
        assert table_layout(case, s) == layout
        for g, a in zip(G, case.grads(s)):
            g.copy_(torch.from_numpy(a))
        active.fill_(1.0)
        for i in case.inactive.get(s, ()):
            active[i] = 0.0
        before = corr.cpu().numpy().copy()
        if kind == "sgd":
            _lib.check(L.tlod_sgd_clip_f32(
                _lib.ptr(chunks), len(rows), case.gs, MOMENTUM, case.clip, _lib.ptr(partials),
                _lib.ptr(norm_scale), _lib.stream_of(partials)), "sgd_clip")
            given = None
        else:
            _lib.check(L.tlod_adam_clip_f32(
                _lib.ptr(chunks), len(rows), _lib.ptr(states), len(ts), case.gs, F.B1, F.B2,
                F.EPS, case.clip, _lib.ptr(partials), _lib.ptr(norm_scale),
                _lib.stream_of(partials)), "adam_clip")
            cd = corr.cpu().numpy()
            given = {i: (cd[i, 0], cd[i, 1]) for i in range(len(ts))}
        res, _ = rp.step(s, corr_given=given)
        what = f"{case.name} {kind} step {s}"
        _same(partials, res.partials, what + " partials")
        _same(norm_scale, np.array([res.total, res.scale]), what + " norm_scale")
        scales.append(float(res.scale))
        for i in range(len(ts)):
            _same(P[i], rp.params[i], f"{what} param {i}")
            for j, st in enumerate(S[i]):
                _same(st, rp.state[i][j], f"{what} state {j} of param {i}")
        if kind == "adam":
            _same(steps, [rp.counts.get(i, 0) for i in range(len(ts))], what + " steps")
            dead = case.inactive.get(s, ())
            _check_corr(cd, res, [i for i in range(len(ts)) if i not in dead], what)
            for i in dead:  # untouched, whatever it held
                assert np.array_equal(cd[i], before[i]), what
    # the regime the case is named for
    if case.clip == 0.0 or case.name.endswith("under") or case.name == "total_eq_clip":
        assert scales == [1.0] * case.nsteps
    if "over" in case.name:
        assert scales[0] < 1.0
    for i, t in enumerate(ts):  # a norm-only row is left to the tiles: untouched here
        if t.norm_only:
            _same(P[i], case.params[i], f"{case.name} norm-only param {i}")


def _optim_run(case, kind, arena, monkeypatch):
    """The case through FusedSGDClip / FusedAdamClip; every step against the restatement."""
    from tlod import conv
    from tlod import optim
    from tlod.optim import FusedAdamClip, FusedSGDClip
    assert optim.CHUNK == CHUNK
    monkeypatch.setenv("TLOD_GRAD_ARENA", "1" if arena else "0")
    monkeypatch.setenv("TLOD_SGD_PACK", "1")
    ts = case.tensors
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy()).view(t.shape).to(dev))
          for p, t in zip(case.params, ts)]
    hp = group_hparams(case, -1)
    groups = [{"params": [p for p, t in zip(ps, ts) if t.group == gi], "lr": lr,
               "weight_decay": wd} for gi, (lr, wd) in enumerate(hp)]
    opt = FusedSGDClip(groups, momentum=MOMENTUM, clip_norm=case.clip) if kind == "sgd" else \
        FusedAdamClip(groups, clip_norm=case.clip)
    assert (opt.arena is not None) == arena
    if case.warm:  # a checkpoint in torch's layout, taken at step t0
        sd = opt.state_dict()
        tt = lambda a, t: torch.from_numpy(a.copy()).view(t.shape)
        sd["state"] = {i: ({"momentum_buffer": tt(st[0], t)} if kind == "sgd" else
                           {"step": torch.tensor(float(case.t0)), "exp_avg": tt(st[0], t),
                            "exp_avg_sq": tt(st[1], t)})
                       for i, (st, t) in enumerate(zip(case.state0, ts))}
        opt.load_state_dict(sd)
    if case.packs:
        for p in ps:
            if p.dim() == 4:
                conv.pack_bs(p, False), conv.pack_bs(p, True)
    rp = Replay(case, kind)
    state = [opt.bufs] if kind == "sgd" else [opt.exp_avg, opt.exp_avg_sq]
    scales = []
    for s in range(case.nsteps):
        for g, (lr, wd) in zip(opt.param_groups, group_hparams(case, s)):
            g["lr"], g["weight_decay"] = lr, wd  # as adjust_learning_rate does
        if s not in case.keep_grad:
            opt.zero_grad()
        rs = [(p, torch.from_numpy(r).view(t.shape).to(dev))
              for p, r, t in zip(ps, case.raw[s], ts) if r is not None]
        sum((p * r).sum() for p, r in rs).backward()  # d/dp = r exactly
        for p, want in zip(ps, case.grads(s)):
            assert (p.grad is None) == (want is None)
        norm = opt.step(case.gs)
        given = None
        if kind == "adam":
            cd = opt.corr.cpu().numpy()
            given = {i: (cd[i, 0], cd[i, 1]) for i in range(len(ts))}
        res, layout = rp.step(s, corr_given=given)
        what = f"{case.name} {kind} arena {arena} step {s}"
        _same(opt.partials[:len(layout)], res.partials, what + " partials")
        _same(opt.norm_scale, np.array([res.total, res.scale]), what + " norm_scale")
        assert float(norm) == float(res.total), what
        scales.append(float(res.scale))
        for i, t in enumerate(ts):
            _same(ps[i].detach().reshape(-1), rp.params[i], f"{what} param {i}")
            for j, st in enumerate(state):
                _same(st[i].reshape(-1), rp.state[i][j], f"{what} state {j} of param {i}")
        if kind == "adam":
            _same(opt.steps, [rp.counts.get(i, 0) for i in range(len(ts))], what + " steps")
            _check_corr(cd, res, sorted({i for i, *_ in layout}), what)
        if case.packs:
            # the 3x3 weights went through the tiles: one per 32 x 32 channels
            want = sum(-(-t.shape[0] // 32) * -(-t.shape[1] // 32) for t in ts
                       if len(t.shape) == 4)
            assert opt._last_hit[4] == want
    return scales


@pytest.mark.gpu
@pytest.mark.parametrize("arena", [True, False], ids=["arena", "no_arena"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [c for c in OPTIM_CASES if c.name != "wd_change"], ids=repr)
def test_optimizer_level(case, kind, arena, monkeypatch):
    """FusedSGDClip / FusedAdamClip over two groups against the restatement: the lr schedule,
    a missing gradient, a step without zero_grad, the pack tiles, a resume at step 1000."""
    scales = _optim_run(case, kind, arena, monkeypatch)
    if case.name == "schedule":  # clip = 10 bites in the first step and not in the second
        assert scales[0] < 1.0 and scales[1] == 1.0, scales


@pytest.mark.gpu
@pytest.mark.parametrize("arena", [True, False], ids=["arena", "no_arena"])
@pytest.mark.parametrize("kind", KINDS)
def test_weight_decay_change_takes_effect(kind, arena, monkeypatch):
    """param_group['weight_decay'] changed between two steps holds from the next step on, as
    in torch.optim: the cached descriptor table of the unchanged gradient pointers must not be
    reused."""
    case = next(c for c in OPTIM_CASES if c.name == "wd_change")
    _optim_run(case, kind, arena, monkeypatch)
