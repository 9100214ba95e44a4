"""ctypes wrapper over the reference's own kernels, compiled for gfx950 by oracle/ref_build.py
into oracle/_ref/libtlod_ref.so (test infrastructure only; nothing in tlod/ loads this).

Functions take and return torch CUDA tensors.  The reference launches on the null stream and
copies with blocking calls, so every call synchronises the device before and after.

The kernels are foreign code without guards of their own.  Every function therefore validates
its inputs on the host *before* the library is loaded or anything is launched and raises
ValueError otherwise.  The preconditions come from reading the kernels:

  * float32, contiguous, one device;
  * every RoI / grid / box value finite: a NaN coordinate passes ``h < 0 || h >= height``
    (roi_align_kernel.cu:54) as valid and then indexes with floor(NaN);
  * batch indices integral and in [0, B): they offset the feature pointer unchecked
    (roi_align_kernel.cu:51, roi_pooling_kernel.cu:75);
  * H, W >= 2: ``hstart = fminf(floor(h), height - 2)`` (roi_align_kernel.cu:48) is -1 on a
    valid sample of a 1-row map;
  * aligned_h, aligned_w >= 2: the bin size divides by ``aligned - 1.`` (:42-43);
  * |roi * scale| <= 2^20, so the int conversions of round() / floor() cannot overflow
    (roi_pooling_kernel.cu:46-66);
  * |grid| <= 8, the same for getTopLeft's floor (roi_crop_cuda_kernel.cu:19-20);
  * R % B == 0 for crop: ``roiPerImage = ob / ib`` (:217) maps grid r to image r / roiPerImage;
  * every element count below 2^31 (all indices are int), and B*C*H*W <= 2^24 for RoIAlign,
    whose image offset is computed in float (roi_align_kernel.cu:51).
"""
import ctypes
import os
from ctypes import c_float, c_int, c_void_p

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(HERE, "_ref")
LIBS = {"off": "libtlod_ref.so", "fma": "libtlod_ref_fma.so"}
COUNT_LIMIT = 2 ** 31  # every element count must stay below it (int indices)
MAX_COORD = float(2 ** 20)
MAX_GRID = 8.0

P, I, F = c_void_p, c_int, c_float
SIGNATURES = {
    # nms_cuda_kernel.cu:87
    "nms_cuda_compute": (None, [P, P, P, I, I, F]),
    # roi_align_kernel.cu:73, :145
    "ROIAlignForwardLaucher": (I, [P, F, I, I, I, I, I, I, P, P, P]),
    "ROIAlignBackwardLaucher": (I, [P, F, I, I, I, I, I, I, I, P, P, P]),
    # roi_pooling_kernel.cu:95, :205
    "ROIPoolForwardLaucher": (I, [P, F, I, I, I, I, I, I, P, P, P, P]),
    "ROIPoolBackwardLaucher": (I, [P, F, I, I, I, I, I, I, I, P, P, P, P]),
    # roi_crop_cuda_kernel.cu:201, :257: 8 sizes, then (pointer, 4 strides) per tensor, stream
    "BilinearSamplerBHWD_updateOutput_cuda_kernel": (I, [I] * 8 + [P, I, I, I, I] * 3 + [P]),
    "BilinearSamplerBHWD_updateGradInput_cuda_kernel": (I, [I] * 8 + [P, I, I, I, I] * 5 + [P]),
}

_loaded = {}


def lib_path(variant="off"):
    return os.path.join(REF_DIR, LIBS[variant])


def available(variant=None):
    """True when the reference libraries were built (both, or the one named)."""
    names = LIBS if variant is None else (variant,)
    return all(os.path.isfile(lib_path(v)) for v in names)


def bind(path):
    """Load a reference library and set the seven entry points' signatures."""
    L = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    return L


def _load(variant):
    if variant not in _loaded:
        path = lib_path(variant)
        if not os.path.isfile(path):
            raise RuntimeError(f"{path} not built: run build() with a reference checkout "
                               "(oracle/ref_build.py)")
        _loaded[variant] = bind(path)
    return _loaded[variant]


# ------------------------------------------------------------------ validation (host only)
def _check_tensors(**tensors):
    dev = None
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: not a torch tensor")
        if t.dtype != torch.float32 and name != "argmax":
            raise ValueError(f"{name}: dtype {t.dtype}, need float32")
        if name == "argmax" and t.dtype != torch.int32:
            raise ValueError(f"argmax: dtype {t.dtype}, need int32")
        if not t.is_contiguous():
            raise ValueError(f"{name}: not contiguous")
        if t.numel() >= COUNT_LIMIT:
            raise ValueError(f"{name}: {t.numel()} elements, need < 2^31")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"{name}: on {t.device}, the others on {dev}")
    return dev


def _check_count(what, n):
    if n >= COUNT_LIMIT:
        raise ValueError(f"{what}: {n} elements, need < 2^31")


def _check_feat(feat):
    if feat.dim() != 4:
        raise ValueError("features: need (B, C, H, W)")
    B, C, H, W = feat.shape
    if min(B, C) < 1 or H < 2 or W < 2:
        raise ValueError(f"features: shape {tuple(feat.shape)}, need B, C >= 1 and H, W >= 2")
    return B, C, H, W


def _check_rois(rois, B, scale):
    if rois.dim() != 2 or rois.shape[1] != 5 or rois.shape[0] < 1:
        raise ValueError("rois: need (R >= 1, 5)")
    r = rois.detach().cpu().numpy()
    if not np.isfinite(r).all():
        raise ValueError("rois: every value must be finite")
    if not np.isfinite(scale) or np.abs(r[:, 1:].astype(np.float64) * scale).max() > MAX_COORD:
        raise ValueError("rois: |coordinate * spatial_scale| must be <= 2^20")
    b = r[:, 0]
    if (b != np.floor(b)).any() or (b < 0).any() or (b >= B).any():
        raise ValueError(f"rois: batch indices must be integers in [0, {B})")
    return rois.shape[0]


def _check_cuda(dev):
    # last, so that every other rejection is reachable (and testable) without a GPU
    if dev.type != "cuda":
        raise ValueError("the reference kernels need CUDA tensors")


def _ptr(t):
    return c_void_p(t.data_ptr())


class _synced:
    """Device of the tensors current, and synchronised around the null-stream launch."""

    def __init__(self, dev):
        self.dev = dev
        self.ctx = torch.cuda.device(dev)

    def __enter__(self):
        self.ctx.__enter__()
        torch.cuda.synchronize(self.dev)

    def __exit__(self, *exc):
        try:
            torch.cuda.synchronize(self.dev)
        finally:
            self.ctx.__exit__(*exc)


# ------------------------------------------------------------------ NMS
def nms_with_count(dets_sorted, thresh, variant="off"):
    """nms_cuda_compute on score-sorted (N, 5) dets.  Returns (keep buffer (N,) int32 on the
    device, the kernel's own count): the first ``count`` entries are the keep list.

    Pointer kinds as the function's copy kinds say (nms_cuda_kernel.cu:97-100, :147, :154):
    the boxes come from a host pointer, keep_out / num_out are device pointers."""
    dev = _check_tensors(dets=dets_sorted)
    if dets_sorted.dim() != 2 or dets_sorted.shape[1] != 5 or dets_sorted.shape[0] < 1:
        raise ValueError("dets: need (N >= 1, 5)")
    n = dets_sorted.shape[0]
    host = np.ascontiguousarray(dets_sorted.detach().cpu().numpy(), dtype=np.float32)
    if not np.isfinite(host).all() or not np.isfinite(thresh):
        raise ValueError("dets / thresh: every value must be finite")
    _check_count("nms mask", n * ((n + 63) // 64) * 8)
    _check_cuda(dev)
    L = _load(variant)
    keep = torch.full((n,), -1, dtype=torch.int32, device=dev)
    num = torch.zeros(1, dtype=torch.int32, device=dev)
    with _synced(dev):
        L.nms_cuda_compute(_ptr(keep), _ptr(num), host.ctypes.data_as(c_void_p), n, 5,
                           float(thresh))
    count = int(num.item())
    if not 0 <= count <= n:
        raise RuntimeError(f"reference NMS returned count {count} for {n} boxes")
    return keep, count


def nms(dets_sorted, thresh, variant="off"):
    """The reference's keep list: int32 indices into the score-sorted dets."""
    keep, count = nms_with_count(dets_sorted, thresh, variant)
    return keep[:count]


# ------------------------------------------------------------------ RoIAlign
def _check_align(feat, rois, ah, aw, scale):
    B, C, H, W = _check_feat(feat)
    R = _check_rois(rois, B, scale)
    ah, aw = int(ah), int(aw)
    if ah < 2 or aw < 2:
        raise ValueError(f"aligned size {ah} x {aw}: need >= 2 (the bin size divides by aligned - 1)")
    if B * C * H * W > 2 ** 24:
        raise ValueError("features: B*C*H*W must be <= 2^24 (float image offset)")
    _check_count("RoIAlign output", R * C * ah * aw)
    return B, C, H, W, R, ah, aw


def roi_align_fwd(feat, rois, aligned_h, aligned_w, scale, variant="off"):
    """ROIAlignForwardLaucher: (B,C,H,W), (R,5) -> (R, C, ah, aw)."""
    dev = _check_tensors(features=feat, rois=rois)
    B, C, H, W, R, ah, aw = _check_align(feat, rois, aligned_h, aligned_w, scale)
    _check_cuda(dev)
    L = _load(variant)
    out = torch.full((R, C, ah, aw), float("nan"), dtype=torch.float32, device=dev)
    with _synced(dev):
        L.ROIAlignForwardLaucher(_ptr(feat), float(scale), R, H, W, C, ah, aw, _ptr(rois),
                                 _ptr(out), None)
    return out


def roi_align_bwd(top_grad, rois, B, C, H, W, scale, variant="off"):
    """ROIAlignBackwardLaucher into a zeroed (B, C, H, W) gradient (float atomicAdd)."""
    dev = _check_tensors(top_grad=top_grad, rois=rois)
    if top_grad.dim() != 4 or top_grad.shape[0] != rois.shape[0] or top_grad.shape[1] != C:
        raise ValueError("top_grad: need (R, C, ah, aw)")
    _, _, _, _, R, ah, aw = _check_align(torch.empty((B, C, H, W), device="meta"), rois,
                                         top_grad.shape[2], top_grad.shape[3], scale)
    _check_count("bottom_grad", B * C * H * W)
    _check_cuda(dev)
    L = _load(variant)
    grad = torch.zeros((B, C, H, W), dtype=torch.float32, device=dev)
    with _synced(dev):
        L.ROIAlignBackwardLaucher(_ptr(top_grad), float(scale), B, R, H, W, C, ah, aw,
                                  _ptr(rois), _ptr(grad), None)
    return grad


# ------------------------------------------------------------------ RoIPool
def _check_pool(feat, rois, ph, pw, scale):
    B, C, H, W = _check_feat(feat)
    R = _check_rois(rois, B, scale)
    ph, pw = int(ph), int(pw)
    if ph < 1 or pw < 1:
        raise ValueError("pooled size: need >= 1")
    _check_count("RoIPool output", R * C * ph * pw)
    return B, C, H, W, R, ph, pw


def roi_pool_fwd(feat, rois, pooled_h, pooled_w, scale, variant="off"):
    """ROIPoolForwardLaucher -> (values (R,C,ph,pw) float32, argmax int32 flat index, -1 empty)."""
    dev = _check_tensors(features=feat, rois=rois)
    B, C, H, W, R, ph, pw = _check_pool(feat, rois, pooled_h, pooled_w, scale)
    _check_cuda(dev)
    L = _load(variant)
    out = torch.full((R, C, ph, pw), float("nan"), dtype=torch.float32, device=dev)
    arg = torch.full((R, C, ph, pw), -2, dtype=torch.int32, device=dev)
    with _synced(dev):
        L.ROIPoolForwardLaucher(_ptr(feat), float(scale), R, H, W, C, ph, pw, _ptr(rois),
                                _ptr(out), _ptr(arg), None)
    return out, arg


def roi_pool_bwd(top_grad, argmax, rois, B, C, H, W, scale, variant="off"):
    """ROIPoolBackwardLaucher: the per-input-element gather (it writes every element)."""
    dev = _check_tensors(top_grad=top_grad, argmax=argmax, rois=rois)
    if top_grad.dim() != 4 or top_grad.shape[0] != rois.shape[0] or top_grad.shape[1] != C \
            or argmax.shape != top_grad.shape:
        raise ValueError("top_grad / argmax: need (R, C, ph, pw) each")
    _, _, _, _, R, ph, pw = _check_pool(torch.empty((B, C, H, W), device="meta"), rois,
                                        top_grad.shape[2], top_grad.shape[3], scale)
    _check_count("bottom_grad", B * C * H * W)
    _check_cuda(dev)
    L = _load(variant)
    grad = torch.full((B, C, H, W), float("nan"), dtype=torch.float32, device=dev)
    with _synced(dev):
        L.ROIPoolBackwardLaucher(_ptr(top_grad), float(scale), B, R, H, W, C, ph, pw,
                                 _ptr(rois), _ptr(grad), _ptr(argmax), None)
    return grad


# ------------------------------------------------------------------ RoICrop sampler
def _check_crop(x, grid):
    B, C, H, W = _check_feat(x)
    if grid.dim() != 4 or grid.shape[3] != 2 or min(grid.shape[:3]) < 1:
        raise ValueError("grid: need (R, gh, gw, 2) in (y, x) order")
    R, gh, gw = grid.shape[:3]
    if R % B != 0:
        raise ValueError(f"grid: R = {R} is no multiple of B = {B} (roiPerImage = R / B)")
    g = grid.detach().cpu().numpy()
    if not np.isfinite(g).all():
        raise ValueError("grid: every value must be finite")
    if np.abs(g).max() > MAX_GRID:
        raise ValueError(f"grid: |value| must be <= {MAX_GRID}")
    _check_count("RoICrop output", R * C * gh * gw)
    return B, C, H, W, R, gh, gw


def _bchw(shape):
    """Strides of a contiguous 4-d tensor, in elements."""
    _, c, h, w = shape
    return (c * h * w, h * w, w, 1)


def roi_crop_fwd(x, grid_yx, variant="off"):
    """BilinearSamplerBHWD_updateOutput_cuda_kernel with the sizes and strides that
    roi_crop_cuda.c:22-45 passes: sizes (oc, ow, oh, ob, ic, ih, iw, ib); input / output
    strides 0..3 of contiguous BCHW; grid strides (0, 3, 1, 2) of contiguous (R, gh, gw, 2).
    The output is zeroed first: the kernel skips samples with no tap inside (:93-94)."""
    dev = _check_tensors(input=x, grid=grid_yx)
    B, C, H, W, R, gh, gw = _check_crop(x, grid_yx)
    _check_cuda(dev)
    L = _load(variant)
    out = torch.zeros((R, C, gh, gw), dtype=torch.float32, device=dev)
    gs = (gh * gw * 2, 1, gw * 2, 2)
    with _synced(dev):
        ok = L.BilinearSamplerBHWD_updateOutput_cuda_kernel(
            C, gw, gh, R, C, H, W, B, _ptr(x), *_bchw(x.shape), _ptr(grid_yx), *gs,
            _ptr(out), *_bchw(out.shape), None)
    if ok != 1:
        raise RuntimeError("reference RoICrop forward reported a launch error")
    return out


def roi_crop_bwd(x, grid_yx, grad_out, variant="off"):
    """BilinearSamplerBHWD_updateGradInput_cuda_kernel (roi_crop_cuda.c:65-98).  Returns
    (grad_input, grad_grid); both start zeroed, and the kernel never writes grad_grid."""
    dev = _check_tensors(input=x, grid=grid_yx, grad_out=grad_out)
    B, C, H, W, R, gh, gw = _check_crop(x, grid_yx)
    if tuple(grad_out.shape) != (R, C, gh, gw):
        raise ValueError("grad_out: need (R, C, gh, gw)")
    _check_cuda(dev)
    L = _load(variant)
    gin = torch.zeros_like(x)
    ggrid = torch.zeros_like(grid_yx)
    gs = (gh * gw * 2, 1, gw * 2, 2)
    with _synced(dev):
        ok = L.BilinearSamplerBHWD_updateGradInput_cuda_kernel(
            C, gw, gh, R, C, H, W, B, _ptr(x), *_bchw(x.shape), _ptr(grid_yx), *gs,
            _ptr(gin), *_bchw(gin.shape), _ptr(ggrid), *gs, _ptr(grad_out),
            *_bchw(grad_out.shape), None)
    if ok != 1:
        raise RuntimeError("reference RoICrop backward reported a launch error")
    return gin, ggrid
