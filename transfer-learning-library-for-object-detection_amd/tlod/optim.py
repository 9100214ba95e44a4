"""Fused clip_gradient + SGD(momentum) or Adam on libtlod (tlod_sgd_clip_pack_f32,
tlod_adam_clip_pack_f32).

Same update as ``clip_gradient(model, 10.)`` (lib/model/utils/net_utils.py:38-49) followed
by ``torch.optim.SGD(params, momentum=0.9)`` with the reference's param groups
(methods/DAF/DAF_train.py:311-325: biases lr*(DOUBLE_BIAS+1) and no weight decay unless
BIAS_DECAY; weights lr and WEIGHT_DECAY) — three launches, no host wait: the gradients
live in the persistent arena (tlod.grads), so the descriptor table is built and uploaded
once per (arena layout, set of parameters with a gradient, learning rates and weight
decays).

3x3 conv weights are updated by tiles that also write their split-bf16 packs (the conv
kernels' operand layouts, tlod_sgd_clip_pack_f32): the optimizer marks them as owned
(`_tlod_pack_owner`), tlod.conv.pack_bs then caches their packs, and the next forward and
backward use the packs this step wrote instead of re-packing every weight.  TLOD_SGD_PACK=0
turns that off (every trainable 3x3 weight re-packed per use, as before; such an optimizer
also takes back the ownership an earlier one claimed, and drops the cached packs of weights a
later one claimed after each of its plain updates, so no pack outlives its weight).  Weight
writes outside these optimizers that bypass the version counter (``p.data.*_()``, a direct
tlod_sgd_clip_f32 call) must call tlod.conv.weights_updated(), as the data-parallel broadcast
does.

FusedAdamClip is the reference's ``--o adam`` (``torch.optim.Adam(params)`` with its defaults
over the same groups, DAF_train.py:320-325) on the same machinery: the same clip, arena,
table keys and pack ownership; exp_avg / exp_avg_sq in place of the momentum buffer, and each
parameter's step count and bias corrections kept on the device (a parameter without a
gradient — None on the host, or no producer rank under data parallelism — does not advance
its count).  Both optimizers save and load ``state_dict()`` in torch's layout, so a checkpoint
moves between them and torch.optim.SGD / torch.optim.Adam over the same groups.
"""
import os

import numpy as np
import torch

from . import _lib
from . import conv as _conv
from .grads import GradArena, arena_of

CHUNK = 65536
_DESC = np.dtype([("param", np.uint64), ("grad", np.uint64), ("buf", np.uint64),
                  ("count", np.int64), ("lr", np.float32), ("wd", np.float32),
                  ("active", np.uint64)])
assert _DESC.itemsize == 48  # sizeof(tlod_sgd_chunk), include/tlod.h
_TILE = np.dtype([("param", np.uint64), ("grad", np.uint64), ("buf", np.uint64),
                  ("active", np.uint64), ("pack_fwd", np.uint64), ("pack_dgrad", np.uint64),
                  ("pack_dgrad_scaled", np.uint64), ("scale", np.uint64), ("lr", np.float32),
                  ("wd", np.float32), ("cout", np.int32), ("cin", np.int32), ("o0", np.int32),
                  ("i0", np.int32), ("reserved", np.int32, 2)])
assert _TILE.itemsize == 96  # sizeof(tlod_sgd_pack_tile), include/tlod.h
TILE = 32  # channels per tile side (optim.hip kPT)
_ADAM_DESC = np.dtype([("param", np.uint64), ("grad", np.uint64), ("exp_avg", np.uint64),
                       ("exp_avg_sq", np.uint64), ("count", np.int64), ("lr", np.float32),
                       ("wd", np.float32), ("active", np.uint64), ("corr", np.uint64)])
assert _ADAM_DESC.itemsize == 64  # sizeof(tlod_adam_chunk), include/tlod.h
_ADAM_TILE = np.dtype([("param", np.uint64), ("grad", np.uint64), ("exp_avg", np.uint64),
                       ("exp_avg_sq", np.uint64), ("active", np.uint64), ("corr", np.uint64),
                       ("pack_fwd", np.uint64), ("pack_dgrad", np.uint64),
                       ("pack_dgrad_scaled", np.uint64), ("scale", np.uint64),
                       ("lr", np.float32), ("wd", np.float32), ("cout", np.int32),
                       ("cin", np.int32), ("o0", np.int32), ("i0", np.int32)])
assert _ADAM_TILE.itemsize == 104  # sizeof(tlod_adam_pack_tile), include/tlod.h
_ADAM_STATE = np.dtype([("step", np.uint64), ("active", np.uint64), ("corr", np.uint64)])
assert _ADAM_STATE.itemsize == 24  # sizeof(tlod_adam_state), include/tlod.h


def _packs_of(p):
    """(fwd pack, dgrad pack, scaled dgrad pack, its scale) the fused update can keep
    current, or None when the weight has none yet."""
    packs = getattr(p, "_tlod_packs", None)
    if not packs:
        return None
    pf = pd = pds = sc = None
    for (dgrad, skey), (_, pk, scale) in packs.items():
        if skey is None:
            if dgrad:
                pd = pk
            else:
                pf = pk
        elif dgrad:
            pds, sc = pk, scale
    return (pf, pd, pds, sc) if (pf is not None or pd is not None or pds is not None) else None


class FusedClipOptimizer:
    """What FusedSGDClip and FusedAdamClip share: the parameter groups, the gradient arena,
    the cached descriptor tables (fast and slow keys), the ownership of the 3x3 weights'
    packs, and the checkpoint layout.  A subclass supplies its state tensors, its table rows
    and its launch."""

    _DESC = _TILE = None  # numpy dtypes of a chunk row and a tile row

    def __init__(self, param_groups, clip_norm=10.0):
        self.param_groups = [dict(g, params=[p for p in g["params"] if p.requires_grad])
                             for g in param_groups]
        self.clip_norm = float(clip_norm)
        self.params = [p for g in self.param_groups for p in g["params"]]
        for p in self.params:
            _lib.require_cuda(p)
        self.fused_packs = os.environ.get("TLOD_SGD_PACK", "1") != "0"
        for p in self.params:
            if p.dim() == 4 and tuple(p.shape[2:]) == (3, 3):
                if self.fused_packs:
                    p._tlod_pack_owner = True
                elif getattr(p, "_tlod_pack_owner", False):
                    # this optimizer's plain update would leave an earlier owner's cached
                    # packs stale: the weight goes back to a repack per use (round-5 advisor)
                    p._tlod_pack_owner = False
                    p._tlod_packs = {}
                    _conv.PACK_GEN[0] += 1
        dev = self.params[0].device
        n_chunks = sum((p.numel() + CHUNK - 1) // CHUNK for p in self.params)
        self.partials = torch.empty(n_chunks, dtype=torch.float32, device=dev)
        self.norm_scale = torch.zeros(2, dtype=torch.float32, device=dev)
        # gradient arena: reuse the one the parameters already belong to (e.g. the DP
        # reducer's), else create one in registration order
        a = arena_of(self.params[0])
        if a is None or any(arena_of(p) is not a for p in self.params):
            a = GradArena(self.params) if os.environ.get("TLOD_GRAD_ARENA", "1") != "0" else None
        self.arena = a
        # descriptor tables per gradient-pointer set; with the arena the key is stable and
        # the (blocking, tiny) upload happens on the first step only
        self._tables = {}
        self.table_builds = 0  # descriptor-table (re)builds: each is a blocking upload
        self._stepped = set()  # indices of the parameters a step has had rows for
        self._last_hit = None

    def zero_grad(self, set_to_none=True):
        if set_to_none and self.arena is not None:
            self.arena.zero_grad()
            return
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def _upload(self, arr):
        table = torch.empty(max(arr.nbytes, 1), dtype=torch.uint8, device=self.partials.device)
        if arr.nbytes:
            host = torch.empty(arr.nbytes, dtype=torch.uint8, pin_memory=True)
            host.numpy()[:] = arr.view(np.uint8)
            table.copy_(host)
        return table

    # --- what a subclass supplies
    def _row(self, idx, off, p_ptr, g_ptr, count, lr, wd, ap):
        """One chunk row (a tuple for _DESC): count elements of parameter idx from float
        offset off."""
        raise NotImplementedError

    def _tile_row(self, idx, p_ptr, g_ptr, ap, pf, pd, pds, sc, lr, wd, cout, cin, o0, i0):
        raise NotImplementedError

    def _extra_tables(self, idxs, act):
        """Further device tables over the parameters (indices) that have rows."""
        return None

    def _launch(self, hit, grad_scale):
        raise NotImplementedError

    def _chunk_table(self, fast=True):
        """Descriptor rows for every parameter that has a gradient (torch.optim skips the
        others entirely: no weight decay, no state update): (chunk table, tile table, rows
        updated by chunks, rows, tiles, packs kept alive, the subclass's extra tables, the
        parameters' indices).  The 3x3 weights with packs get tiles; their chunk rows
        (negative counts) only enter the gradient norm."""
        a = self.arena
        act = a.active if a is not None and a.active is not None else None
        # (the rows bake in lr and weight decay: either changed in a group means a new table)
        tail = tuple(g["lr"] for g in self.param_groups) + \
            tuple(g.get("weight_decay", 0.0) for g in self.param_groups) + \
            (0 if act is None else act.data_ptr(), _conv.PACK_GEN[0] if self.fused_packs else 0)
        # fast key: with the arena, a step in which every parameter's gradient arrived has
        # every gradient in its fixed slot (GradArena._on_grad), so the table depends only on
        # the arena, the learning rates and the packs (no per-parameter host work: ~0.6 ms
        # of Python per ResNet101 step, the GPU idling at the end of the backward)
        if fast and a is not None and a.n_seen == len(a.params) and \
                all(arena_of(p) is a for p in self._fast_ok()):
            # (the layout generation, not the buffer address: a relayout's new buffer may
            # land where an earlier one was freed)
            key = ("all", id(a), a.layout_gen) + tail
        else:
            key = tuple(0 if p.grad is None else p.grad.data_ptr() for p in self.params) + tail
        hit = self._tables.get(key)
        if hit is not None:
            return hit
        self.table_builds += 1
        rows, tiles, keep, idxs = [], [], [], []
        idx = -1
        for g in self.param_groups:
            for p in g["params"]:
                idx += 1
                gr = p.grad
                if gr is None:
                    continue
                assert gr.is_contiguous() and p.is_contiguous()
                idxs.append(idx)
                n = p.numel()
                lr, wd = g["lr"], g.get("weight_decay", 0.0)
                # data parallel: skipped on the device when no rank produced the gradient
                ap = 0 if act is None else act.data_ptr() + 4 * a.index[p]
                packs = _packs_of(p) if self.fused_packs and getattr(p, "_tlod_pack_owner",
                                                                     False) else None
                # every parameter's chunk rows in parameter order (the norm's summation order
                # does not depend on TLOD_SGD_PACK); a negative count marks a norm-only row,
                # whose elements the pack tiles update
                sign = 1 if packs is None else -1
                for off in range(0, n, CHUNK):
                    rows.append(self._row(idx, off, p.data_ptr() + 4 * off,
                                          gr.data_ptr() + 4 * off, sign * min(CHUNK, n - off),
                                          lr, wd, ap))
                if packs is None:
                    continue
                keep.append(packs)  # the table holds their pointers
                pf, pd, pds, sc = (0 if t is None else t.data_ptr() for t in packs)
                cout, cin = p.shape[0], p.shape[1]
                for o0 in range(0, cout, TILE):
                    for i0 in range(0, cin, TILE):
                        tiles.append(self._tile_row(idx, p.data_ptr(), gr.data_ptr(), ap, pf, pd,
                                                    pds, sc, lr, wd, cout, cin, o0, i0))
        chunks = self._upload(np.array(rows, dtype=self._DESC))
        tile_t = self._upload(np.array(tiles, dtype=self._TILE))
        extra = self._extra_tables(idxs, act)
        if len(self._tables) >= 8:
            self._tables.pop(next(iter(self._tables)))
        hit = (chunks, tile_t, len(rows), len(rows), len(tiles), keep, extra, idxs)
        self._tables[key] = hit
        return hit

    def _fast_ok(self):
        """() once the optimizer's parameters are known to be exactly the arena's (checked
        once), else the parameters (the fast key then requires each to be in the arena)."""
        if getattr(self, "_fast_checked", None) is None:
            a = self.arena
            self._fast_checked = (a is not None and set(a.params) == set(self.params))
        return () if self._fast_checked else self.params

    @torch.no_grad()
    def step(self, grad_scale=1.0):
        """grad_scale: factor applied to every gradient as it is read (data parallel: 1/world
        of the all-reduced sums, tlod.dist.GradBucketReducer.grad_scale).  Returns the
        gradient norm (a device scalar)."""
        # the fast key needs a zero_grad (a new arena generation) since the last step
        gen = self.arena.gen if self.arena is not None else None
        fast = gen is not None and gen != getattr(self, "_last_gen", None)
        self._last_gen = gen
        hit = self._chunk_table(fast)
        if hit[3] == 0:
            return self.norm_scale[0]
        self._launch(hit, float(grad_scale))
        if hit is not self._last_hit:
            self._last_hit = hit
            self._stepped.update(hit[7])
        if not self.fused_packs:
            # the plain update writes weights without a version bump: packs cached for a
            # weight that a pack-writing optimizer claimed after this one was built are stale
            for p in self.params:
                if getattr(p, "_tlod_pack_owner", False) and getattr(p, "_tlod_packs", None):
                    p._tlod_packs = {}
                    _conv.PACK_GEN[0] += 1
        return self.norm_scale[0]

    # --- checkpoints, in torch.optim's layout
    def _torch_defaults(self):
        """The group entries torch's optimizer of the same kind carries."""
        raise NotImplementedError

    def _state_of(self):
        """{parameter index: state dict} of the parameters that have state."""
        raise NotImplementedError

    def _load_state(self, state, groups):
        raise NotImplementedError

    def state_dict(self):
        """torch.optim.Optimizer.state_dict()'s layout: groups refer to parameters by index
        (group after group), state per index; loads into the torch optimizer of the same
        kind built over the same groups."""
        groups, start = [], 0
        defaults = self._torch_defaults()
        for g in self.param_groups:
            d = dict(defaults)
            d.update({k: v for k, v in g.items() if k != "params"})
            d["params"] = list(range(start, start + len(g["params"])))
            start += len(g["params"])
            groups.append(d)
        return {"state": self._state_of(), "param_groups": groups}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Accepts what state_dict() or the torch optimizer of the same kind over the same
        groups saved.  lr and weight_decay come from the saved groups."""
        saved = state_dict["param_groups"]
        if len(saved) != len(self.param_groups) or any(
                len(s["params"]) != len(g["params"]) for s, g in zip(saved, self.param_groups)):
            raise ValueError("loaded state dict's parameter groups do not match the optimizer's")
        ids = [i for s in saved for i in s["params"]]
        index = {sid: idx for idx, sid in enumerate(ids)}
        state = {index[sid]: st for sid, st in state_dict["state"].items()}
        self._load_state(state, saved)
        for s, g in zip(saved, self.param_groups):
            for k in ("lr", "weight_decay"):
                if k in s:
                    g[k] = s[k]
        self._stepped = set(state)
        self._tables.clear()
        self._last_hit = None


class FusedSGDClip(FusedClipOptimizer):
    """param_groups: list of dicts {params, lr, weight_decay} (torch.optim.SGD layout)."""

    _DESC, _TILE = _DESC, _TILE

    def __init__(self, param_groups, momentum=0.9, clip_norm=10.0):
        super().__init__(param_groups, clip_norm)
        self.momentum = float(momentum)
        self.bufs = [torch.zeros_like(p) for p in self.params]

    def _row(self, idx, off, p_ptr, g_ptr, count, lr, wd, ap):
        return (p_ptr, g_ptr, self.bufs[idx].data_ptr() + 4 * off, count, lr, wd, ap)

    def _tile_row(self, idx, p_ptr, g_ptr, ap, pf, pd, pds, sc, lr, wd, cout, cin, o0, i0):
        return (p_ptr, g_ptr, self.bufs[idx].data_ptr(), ap, pf, pd, pds, sc, lr, wd, cout, cin,
                o0, i0, (0, 0))

    def _launch(self, hit, grad_scale):
        chunks, tiles, n_update, n, n_tiles = hit[:5]
        _lib.check(_lib.lib().tlod_sgd_clip_pack_f32(
            _lib.ptr(chunks), n, n_update, _lib.ptr(tiles), n_tiles, grad_scale,
            self.momentum, self.clip_norm, _lib.ptr(self.partials), _lib.ptr(self.norm_scale),
            _lib.stream_of(self.partials)), "sgd_clip")

    def _torch_defaults(self):
        d = dict(torch.optim.SGD([torch.zeros(1)], lr=0.0).defaults)
        d["momentum"] = self.momentum
        return d

    def _state_of(self):
        return {i: {"momentum_buffer": self.bufs[i]} for i in sorted(self._stepped)}

    def _load_state(self, state, groups):
        for s in groups:
            if s.get("nesterov") or s.get("maximize") or s.get("dampening"):
                raise ValueError("FusedSGDClip: nesterov / maximize / dampening are not supported")
        moms = {float(s["momentum"]) for s in groups if "momentum" in s}
        if len(moms) > 1:
            raise ValueError("FusedSGDClip: one momentum for all groups")
        if moms:
            self.momentum = moms.pop()
        for i, b in enumerate(self.bufs):
            mb = state.get(i, {}).get("momentum_buffer")
            if mb is None:
                b.zero_()
            else:
                b.copy_(mb)


class FusedAdamClip(FusedClipOptimizer):
    """clip_gradient + torch.optim.Adam (defaults: L2 weight decay, no amsgrad) over
    param_groups of {params, lr, weight_decay} (tlod_adam_clip_pack_f32)."""

    _DESC, _TILE = _ADAM_DESC, _ADAM_TILE

    def __init__(self, param_groups, betas=(0.9, 0.999), eps=1e-8, clip_norm=10.0):
        param_groups = list(param_groups)
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        if not (0.0 <= self.betas[0] < 1.0 and 0.0 <= self.betas[1] < 1.0):
            raise ValueError(f"FusedAdamClip: betas {betas} outside [0, 1)")
        if not self.eps > 0.0:
            raise ValueError(f"FusedAdamClip: eps {eps} must be > 0")
        self._check_groups(param_groups)
        super().__init__(param_groups, clip_norm)
        dev = self.params[0].device
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]
        # per parameter, on the device: its step count and the bias corrections of that count
        # (written by the step's norm launch, read by the chunk and tile rows)
        self.steps = torch.zeros(len(self.params), dtype=torch.int32, device=dev)
        self.corr = torch.zeros(len(self.params), 2, dtype=torch.float32, device=dev)

    def _check_groups(self, groups):
        for g in groups:
            for k in ("amsgrad", "maximize", "decoupled_weight_decay"):
                if g.get(k):
                    raise ValueError(f"FusedAdamClip: {k} is not supported")
            if "betas" in g and tuple(map(float, g["betas"])) != self.betas or \
                    "eps" in g and float(g["eps"]) != self.eps:
                raise ValueError("FusedAdamClip: betas / eps are the optimizer's, one value "
                                 "for all groups")

    def _row(self, idx, off, p_ptr, g_ptr, count, lr, wd, ap):
        return (p_ptr, g_ptr, self.exp_avg[idx].data_ptr() + 4 * off,
                self.exp_avg_sq[idx].data_ptr() + 4 * off, count, lr, wd, ap,
                self.corr.data_ptr() + 8 * idx)

    def _tile_row(self, idx, p_ptr, g_ptr, ap, pf, pd, pds, sc, lr, wd, cout, cin, o0, i0):
        return (p_ptr, g_ptr, self.exp_avg[idx].data_ptr(), self.exp_avg_sq[idx].data_ptr(), ap,
                self.corr.data_ptr() + 8 * idx, pf, pd, pds, sc, lr, wd, cout, cin, o0, i0)

    def _extra_tables(self, idxs, act):
        a = self.arena
        rows = [(self.steps.data_ptr() + 4 * i,
                 0 if act is None else act.data_ptr() + 4 * a.index[self.params[i]],
                 self.corr.data_ptr() + 8 * i) for i in idxs]
        return self._upload(np.array(rows, dtype=_ADAM_STATE))

    def _launch(self, hit, grad_scale):
        chunks, tiles, n_update, n, n_tiles, _, states, idxs = hit
        _lib.check(_lib.lib().tlod_adam_clip_pack_f32(
            _lib.ptr(chunks), n, n_update, _lib.ptr(tiles), n_tiles, _lib.ptr(states), len(idxs),
            grad_scale, self.betas[0], self.betas[1], self.eps, self.clip_norm,
            _lib.ptr(self.partials), _lib.ptr(self.norm_scale), _lib.stream_of(self.partials)),
            "adam_clip")

    def _torch_defaults(self):
        d = dict(torch.optim.Adam([torch.zeros(1)]).defaults)
        d["betas"], d["eps"] = self.betas, self.eps
        return d

    def _state_of(self):
        steps = self.steps.tolist()  # (a host sync: checkpoints only)
        return {i: {"step": torch.tensor(float(t), dtype=torch.float32),
                    "exp_avg": self.exp_avg[i], "exp_avg_sq": self.exp_avg_sq[i]}
                for i, t in enumerate(steps) if t > 0}

    def _load_state(self, state, groups):
        for s in groups:
            for k in ("amsgrad", "maximize", "decoupled_weight_decay"):
                if s.get(k):
                    raise ValueError(f"FusedAdamClip: {k} is not supported")
        betas = {tuple(map(float, s["betas"])) for s in groups if "betas" in s}
        eps = {float(s["eps"]) for s in groups if "eps" in s}
        if len(betas) > 1 or len(eps) > 1:
            raise ValueError("FusedAdamClip: one betas / eps for all groups")
        if betas:
            self.betas = betas.pop()
        if eps:
            self.eps = eps.pop()
        steps = [0] * len(self.params)
        for i, (m, v) in enumerate(zip(self.exp_avg, self.exp_avg_sq)):
            st = state.get(i)
            if st is None:
                m.zero_()
                v.zero_()
            else:
                m.copy_(st["exp_avg"])
                v.copy_(st["exp_avg_sq"])
                steps[i] = int(round(float(st["step"])))
        self.steps.copy_(torch.tensor(steps, dtype=torch.int32))
