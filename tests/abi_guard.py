"""Guard bands and poisoned outputs around raw C ABI calls (include/tlod.h).

The value tests compare what a kernel computes; this harness checks *where* it writes.  Every
buffer of a call is one uint8 allocation laid out as [front guard | payload | back guard]:
the payload starts 256-byte aligned and is exactly numel * itemsize bytes long, the back guard
starts at the very next byte, and each guard is at least as large as the payload and at least
1 MiB (an out-of-tile row / column store or a -1 halo store lands inside it).  Payloads are
filled by role:

  input        the test's data; a clone is kept and must be bit-equal after the call
  output       poison (a NaN bit pattern for floats, a sentinel no valid result takes for
               integers, 0xEE for one-byte outputs); none may remain where the header promises
               a full write, and all of it must remain where it promises "not written"
  accumulator  finite values the kernel adds into (the caller keeps them as `.initial`)
  workspace    poison, exactly *_workspace_bytes long; its contents are not checked

`Call.check()` synchronises once and verifies every guard byte of every buffer, every input
and every output.  The harness works on CPU tensors too (tests/test_abi_guard_cpu.py makes it
fail on purpose with plain torch writes).
"""
import ctypes

import numpy as np
import torch

GUARD_BYTE = 0xA5
MIN_GUARD = 1 << 20
ALIGN = 256
TLOD_EWORKSPACE = -3

# one element of poison per dtype, as little-endian bytes
_POISON = {
    torch.float32: np.array([0x7FFA5A5A], np.uint32).view(np.uint8),       # a quiet NaN
    torch.float64: np.array([0x7FFA5A5A5A5A5A5A], np.uint64).view(np.uint8),
    torch.int32: np.array([0x9E9E9E9E], np.uint32).view(np.uint8),         # -1633771874
    torch.int64: np.array([0x9E9E9E9E9E9E9E9E], np.uint64).view(np.uint8),
    torch.int16: np.array([0x9E9E], np.uint16).view(np.uint8),
    torch.uint8: np.array([0xEE], np.uint8),
}

# the ledger (tests/test_abi_guard_cpu.py): every name of tlod._lib.SIGNATURES is in exactly
# one of GUARDED (a case in tests/test_abi_guard_gpu.py), HOST_ONLY or DEFERRED
HOST_ONLY = [
    "tlod_abi_version", "tlod_last_error", "tlod_set_cu_reserve", "tlod_conv_pack_bs_bytes",
    "tlod_nms_workspace_bytes", "tlod_roi_align_avg_bwd_workspace_bytes",
    "tlod_roi_align_avg_bwd_gather_workspace_bytes", "tlod_roi_align_avg_s2_workspace_bytes",
    "tlod_proposal_workspace_bytes", "tlod_anchor_target_workspace_bytes",
    "tlod_proposal_target_workspace_bytes", "tlod_conv_fwd_workspace_bytes",
    "tlod_conv_dgrad_workspace_bytes", "tlod_conv_wgrad_workspace_bytes",
    "tlod_conv_fwd_bs_workspace_bytes", "tlod_conv_wgrad_bs_workspace_bytes",
    "tlod_gemm_bs_workspace_bytes", "tlod_conv3x3_gemm_bs_workspace_bytes",
    "tlod_conv1x1_gemm_bs_workspace_bytes", "tlod_conv1x1_small_wgrad_workspace_bytes",
    "tlod_gemm_nhwc3_bs_workspace_bytes",
]

GUARDED = [
    # A: workspace-bearing (exact-size workspace, too-small workspace refused)
    "tlod_nms_f32", "tlod_proposal_f32",
    "tlod_anchor_target_label_f32", "tlod_anchor_target_sample_f32", "tlod_anchor_target_f32",
    "tlod_proposal_target_count_f32", "tlod_proposal_target_sample_f32",
    "tlod_proposal_target_f32",
    "tlod_roi_align_avg_bwd_f32", "tlod_roi_align_avg_s2_nhwc_fwd_f32",
    "tlod_roi_align_avg_s2_nhwc_bwd_f32",
    "tlod_conv_fwd_f32", "tlod_conv_fwd_ex_f32", "tlod_conv_dgrad_f32", "tlod_conv_wgrad_f32",
    "tlod_conv_fwd_bs_f32", "tlod_conv_dgrad_bs_mask_f32",
    "tlod_conv_wgrad_bs_f32", "tlod_conv_wgrad_bs_ex_f32",
    "tlod_conv3x3_gemm_bs_f32", "tlod_conv1x1_gemm_bs_f32", "tlod_conv1x1_gemm_bs_ex_f32",
    "tlod_gemm_bs_f32", "tlod_gemm_bs_ex_f32", "tlod_gemm_bs_mask_f32", "tlod_gemm_nhwc3_bs_f32",
    "tlod_conv1x1_small_wgrad_f32", "tlod_drm_fwd_f32",
    # C: accumulate contracts without a workspace
    "tlod_roi_align_bwd_f32", "tlod_roi_pool_bwd_f32",
    # D: full-write, zero-fill and padding contracts
    "tlod_roi_align_fwd_f32", "tlod_roi_align_avg_fwd_f32", "tlod_roi_pool_fwd_f32",
    "tlod_roi_crop_fwd_f32", "tlod_roi_crop_bwd_f32", "tlod_roi_crop_pool_fwd_f32",
    "tlod_roi_crop_pool_bwd_f32",
    "tlod_upsample2_zero_f32", "tlod_depth_to_space_f32", "tlod_drm_relu_bwd_f32",
    "tlod_col2im3x3_nhwc_f32", "tlod_col2im3x3_nhwc_mask_f32",
    "tlod_relu_bwd_bias_f32", "tlod_relu_bwd_ex_f32", "tlod_maxpool2x2_relu_bwd_f32",
    "tlod_conv1x1_small_dgrad_f32",
    "tlod_rpn_loss_bwd_f32", "tlod_rcnn_loss_bwd_f32", "tlod_da_loss_f32", "tlod_da_loss_bwd_f32",
    "tlod_masked_nll2_f32", "tlod_masked_nll2_bwd_f32", "tlod_kd_kl_f32", "tlod_kd_kl_bwd_f32",
    "tlod_roi_scale_labels_f32", "tlod_us_daf_loss_f32", "tlod_us_daf_loss_bwd_f32",
    "tlod_image_blob_u8", "tlod_detect_f32",
    # E: plain full-write entry points
    "tlod_conv3x3_direct_f32", "tlod_conv_fwd_bs_pool_f32", "tlod_maxpool2x2_f32",
    "tlod_stem_conv7x7s2_f32", "tlod_subsample2_f32", "tlod_im2col3x3_nhwc_f32",
    "tlod_space_to_depth_f32", "tlod_conv1x1_small_fwd_f32",
    "tlod_conv_pack_fwd_f32", "tlod_conv_pack_dgrad_f32", "tlod_conv_pack_bs",
    "tlod_conv_pack_bs_ex", "tlod_relu_dropout_f32", "tlod_relu_dropout_bwd_f32",
    "tlod_rpn_loss_f32", "tlod_rcnn_loss_f32", "tlod_fgbg_maps_f32", "tlod_gt_cell_mask_f32",
]

# what DEFERRED may hold at all: the plain full-write entry points and the four optimisers
DEFERRABLE = GUARDED[GUARDED.index("tlod_conv3x3_direct_f32"):] + [
    "tlod_sgd_clip_f32", "tlod_sgd_clip_pack_f32", "tlod_adam_clip_f32", "tlod_adam_clip_pack_f32"]

_OPTIM = ("writes through device descriptor tables, not output pointers; its \"untouched when "
          "inactive\" rule is covered by ")
DEFERRED = {
    "tlod_sgd_clip_f32": _OPTIM + "tests/test_optim_gpu.py",
    "tlod_sgd_clip_pack_f32": _OPTIM + "tests/test_optim_gpu.py",
    "tlod_adam_clip_f32": _OPTIM + "tests/test_adam_gpu.py",
    "tlod_adam_clip_pack_f32": _OPTIM + "tests/test_adam_gpu.py",
}


class GuardError(AssertionError):
    pass


class Guarded:
    """One guarded buffer.  `payload` is the tensor a kernel sees; `ptr` its address."""

    def __init__(self, shape, dtype, role, data=None, device="cuda", name=""):
        assert role in ("in", "out", "acc", "ws")
        self.shape = tuple(int(s) for s in (shape if hasattr(shape, "__len__") else (shape,)))
        self.dtype, self.role, self.name = dtype, role, name or role
        self.itemsize = torch.empty((), dtype=dtype).element_size()
        self.numel = int(np.prod(self.shape)) if self.shape else 1
        self.nbytes = self.numel * self.itemsize
        g = max(MIN_GUARD, self.nbytes)
        self.guard = g + (-g) % ALIGN
        total = 2 * self.guard + self.nbytes + ALIGN
        self.buf = torch.full((total,), GUARD_BYTE, dtype=torch.uint8, device=device)
        self.off = self.guard + (-(self.buf.data_ptr() + self.guard)) % ALIGN
        assert (self.buf.data_ptr() + self.off) % ALIGN == 0 and self.off >= self.guard
        assert total - (self.off + self.nbytes) >= self.guard
        self.end = self.off + self.nbytes  # first byte of the back guard: no rounding
        self.untouched = None  # bool mask over the payload: poison must REMAIN there
        self.initial = None
        if role in ("out", "ws"):
            self.poison()
        else:
            assert data is not None and tuple(data.shape) == self.shape and data.dtype == dtype
            self.payload.copy_(data)
            self.initial = self.payload.clone()

    # ---- views
    @property
    def raw(self):
        return self.buf[self.off:self.end]

    @property
    def payload(self):
        if self.nbytes == 0:
            return torch.empty(self.shape, dtype=self.dtype, device=self.buf.device)
        return self.raw.view(self.dtype).view(self.shape)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + self.off)

    def window(self, before=0, after=0):
        """1-D view of the payload with `before` / `after` elements of the guards on each side
        (only the self-test writes through it: a kernel never gets this view)."""
        lo, hi = self.off - before * self.itemsize, self.end + after * self.itemsize
        return self.buf[lo:hi].view(self.dtype)

    # ---- poison
    def _pattern(self):
        return torch.from_numpy(_POISON[self.dtype].copy()).to(self.buf.device)

    def poison(self):
        if self.nbytes:
            self.raw.view(self.numel, self.itemsize).copy_(
                self._pattern().expand(self.numel, self.itemsize))

    def poisoned(self):
        """bool tensor of the payload's shape: True where the element still is the poison."""
        if self.nbytes == 0:
            return torch.zeros(self.shape, dtype=torch.bool, device=self.buf.device)
        m = (self.raw.view(self.numel, self.itemsize) == self._pattern()).all(1)
        return m.view(self.shape)

    # ---- checks (the caller has synchronised)
    def guards_intact(self):
        front, back = self.buf[:self.off], self.buf[self.end:]
        bad_f, bad_b = int((front != GUARD_BYTE).sum()), int((back != GUARD_BYTE).sum())
        if bad_f or bad_b:
            where = []
            if bad_f:
                i = int(torch.nonzero(front != GUARD_BYTE)[-1])
                where.append(f"{bad_f} bytes of the front guard, nearest {self.off - i} B "
                             f"before the payload")
            if bad_b:
                i = int(torch.nonzero(back != GUARD_BYTE)[0])
                where.append(f"{bad_b} bytes of the back guard, nearest {i} B past the payload")
            raise GuardError(f"{self.name} {self.shape}: write outside the buffer: "
                             + "; ".join(where))

    def check(self):
        self.guards_intact()
        if self.role == "in":
            if self.nbytes:
                kept = self.initial.reshape(-1).view(torch.uint8)  # bytes: NaN-safe, -0 != +0
                if not torch.equal(self.raw, kept):
                    n = int((self.raw != kept).view(self.numel, self.itemsize).any(1).sum())
                    raise GuardError(f"{self.name} {self.shape}: const input changed "
                                     f"({n} elements)")
        elif self.role == "out":
            p = self.poisoned()
            if self.untouched is None:
                left = p
            else:
                left = p & ~self.untouched
                gone = self.untouched & ~p
                if bool(gone.any()):
                    raise GuardError(f"{self.name} {self.shape}: {int(gone.sum())} elements the "
                                     "header says are not written were written")
            if bool(left.any()):
                idx = torch.nonzero(left)[0].tolist()
                raise GuardError(f"{self.name} {self.shape}: {int(left.sum())} output elements "
                                 f"never written (first at {idx})")

    def check_pure_poison(self):
        self.guards_intact()
        if not bool(self.poisoned().all()):
            raise GuardError(f"{self.name} {self.shape}: written by a call that must fail first")


def guarded(shape, dtype, fill, device="cuda", name=""):
    """[front guard | payload | back guard] with the payload filled by role: fill = "out" /
    "ws" (poison), or ("in", tensor) / ("acc", tensor)."""
    if isinstance(fill, str):
        return Guarded(shape, dtype, fill, device=device, name=name)
    role, data = fill
    return Guarded(shape, dtype, role, data=data, device=device, name=name)


class Call:
    """The buffers of one (or a few chained) C ABI calls."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.bufs = []

    def _add(self, g):
        self.bufs.append(g)
        return g

    def inp(self, t, name="in"):
        if t is None:
            return None
        t = torch.as_tensor(t)
        return self._add(Guarded(t.shape, t.dtype, "in", t.contiguous(), self.device, name))

    def acc(self, t, name="acc"):
        t = torch.as_tensor(t)
        return self._add(Guarded(t.shape, t.dtype, "acc", t.contiguous(), self.device, name))

    def out(self, shape, dtype=torch.float32, name="out"):
        return self._add(Guarded(shape, dtype, "out", device=self.device, name=name))

    def ws(self, nbytes, name="ws"):
        """Exactly nbytes of guarded scratch; None (pass NULL, 0) when the query says 0."""
        nbytes = int(nbytes)
        if nbytes == 0:
            return None
        return self._add(Guarded((nbytes,), torch.uint8, "ws", device=self.device, name=name))

    def run(self, fn, *args):
        """fn(*args, stream) with Guarded -> its payload address; returns the status."""
        from tlod import _lib
        conv = [a.ptr if isinstance(a, Guarded) else a for a in args]
        return fn(*conv, _lib.stream_of())

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize()

    def check(self):
        self.sync()
        for g in self.bufs:
            g.check()

    def check_rejected(self):
        """After a call that must fail before launching anything: guards intact, inputs
        unchanged, every output still pure poison."""
        self.sync()
        for g in self.bufs:
            if g.role == "out":
                g.check_pure_poison()
            elif g.role == "acc":
                g.guards_intact()
                if not torch.equal(g.payload, g.initial):
                    raise GuardError(f"{g.name}: accumulator changed by a rejected call")
            else:
                g.check()
