"""Drop-ins for ``model.roi_crop`` (lib/model/roi_crop/{functions,modules}/roi_crop.py) and
``net_utils._affine_grid_gen`` — POOLING_MODE 'crop'.

``_RoICrop()(input, grid)`` is the reference's bilinear sampler over a (R, gh, gw, 2) grid in
(y, x) order (``tlod_roi_crop_*_f32``); ``affine_grid_gen`` builds that grid the reference's
way.  ``RoICropPool`` is what the detectors call: theta, grid, sampler and the 2x2 max-pool
(faster_rcnn.py:73-81) in one kernel each way (``tlod_roi_crop_pool_*_f32``), with no grid and
no (R, C, 2P, 2P) map in memory.  The reference's CPU path (roi_crop.c) is not reproduced:
inputs must be CUDA tensors.
"""
import torch
import torch.nn.functional as F
from torch.nn import Module

from . import _lib


class RoICropFunction(torch.autograd.Function):
    """functions/roi_crop.py:7-21 as a static autograd Function.  The backward returns the
    input gradient; the grid's gradient is zeros, as the CUDA kernel leaves it
    (roi_crop_cuda_kernel.cu:111-194 never writes gradGrids)."""

    @staticmethod
    def forward(ctx, input1, input2):
        _lib.require_cuda(input1, input2)
        x = input1.contiguous()
        grid = input2.contiguous().float()
        B, C, H, W = x.shape
        R, gh, gw = grid.shape[0], grid.shape[1], grid.shape[2]
        out = torch.empty((R, C, gh, gw), dtype=x.dtype, device=x.device)
        _lib.check(_lib.lib().tlod_roi_crop_fwd_f32(
            _lib.ptr(x), B, C, H, W, _lib.ptr(grid), R, gh, gw, _lib.ptr(out),
            _lib.stream_of(x)), "roi_crop_fwd")
        ctx.save_for_backward(grid)
        ctx.meta = (B, C, H, W)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        (grid,) = ctx.saved_tensors
        B, C, H, W = ctx.meta
        g = grad_output.contiguous()
        R, gh, gw = grid.shape[0], grid.shape[1], grid.shape[2]
        grad_in = torch.empty((B, C, H, W), dtype=g.dtype, device=g.device)
        _lib.check(_lib.lib().tlod_roi_crop_bwd_f32(
            _lib.ptr(g), _lib.ptr(grid), R, C, gh, gw, B, H, W, _lib.ptr(grad_in),
            _lib.stream_of(g)), "roi_crop_bwd")
        return grad_in, (torch.zeros_like(grid) if ctx.needs_input_grad[1] else None)


class _RoICrop(Module):
    """modules/roi_crop.py:4-8."""

    def __init__(self, layout="BHWD"):
        super().__init__()

    def forward(self, input1, input2):
        return RoICropFunction.apply(input1, input2)


def affine_grid_gen(rois, input_size, grid_size):
    """net_utils.py:142-164: the (R, grid_size, grid_size, 2) sampling grid in (x, y) order.
    The reference's F.affine_grid predates the align_corners argument; its base grid spans
    [-1, 1] inclusive, which is align_corners=True."""
    rois = rois.detach()
    x1 = rois[:, 1::4] / 16.0
    y1 = rois[:, 2::4] / 16.0
    x2 = rois[:, 3::4] / 16.0
    y2 = rois[:, 4::4] / 16.0
    height, width = input_size[0], input_size[1]
    zero = rois.new_zeros(rois.size(0), 1)
    theta = torch.cat([
        (x2 - x1) / (width - 1),
        zero,
        (x1 + x2 - width + 1) / (width - 1),
        zero,
        (y2 - y1) / (height - 1),
        (y1 + y2 - height + 1) / (height - 1)], 1).view(-1, 2, 3)
    return F.affine_grid(theta, torch.Size((rois.size(0), 1, grid_size, grid_size)),
                         align_corners=True)


class RoICropPoolFunction(torch.autograd.Function):
    """faster_rcnn.py:73-81 fused: affine grid + (y, x) swap + _RoICrop (+ max_pool2d(2, 2))."""

    @staticmethod
    def forward(ctx, features, rois, pooled_size, spatial_scale, max_pool):
        _lib.require_cuda(features, rois)
        feat = features.contiguous()
        rois_c = rois.contiguous().float()
        B, C, H, W = feat.shape
        R = rois_c.shape[0]
        P, sc, mp = int(pooled_size), float(spatial_scale), int(bool(max_pool))
        out = torch.empty((R, C, P, P), dtype=feat.dtype, device=feat.device)
        argmax = torch.empty((R, C, P, P), dtype=torch.uint8, device=feat.device) if mp else None
        _lib.check(_lib.lib().tlod_roi_crop_pool_fwd_f32(
            _lib.ptr(feat), B, C, H, W, _lib.ptr(rois_c), R, P, sc, mp, _lib.ptr(out),
            _lib.ptr(argmax), _lib.stream_of(feat)), "roi_crop_pool_fwd")
        ctx.save_for_backward(rois_c, argmax)
        ctx.meta = (B, C, H, W, P, sc, mp)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        rois_c, argmax = ctx.saved_tensors
        B, C, H, W, P, sc, mp = ctx.meta
        g = grad_output.contiguous()
        grad_in = torch.empty((B, C, H, W), dtype=g.dtype, device=g.device)
        _lib.check(_lib.lib().tlod_roi_crop_pool_bwd_f32(
            _lib.ptr(g), _lib.ptr(argmax), B, C, H, W, _lib.ptr(rois_c), rois_c.shape[0], P, sc,
            mp, _lib.ptr(grad_in), _lib.stream_of(g)), "roi_crop_pool_bwd")
        return grad_in, None, None, None, None


class RoICropPool(Module):
    """POOLING_MODE 'crop' as one module: ``forward(features, rois)`` -> (R, C, P, P).  The
    image of a RoI is ``rois[:, 0]`` (the reference's sampler assumes R / B RoIs per image, in
    order; equal whenever that holds)."""

    def __init__(self, pooled_size, spatial_scale, max_pool=True):
        super().__init__()
        self.pooled_size = int(pooled_size)
        self.spatial_scale = float(spatial_scale)
        self.max_pool = bool(max_pool)

    def forward(self, features, rois, max_pool=None):
        """max_pool: this call's 2x2 max-pool switch (default: the constructor's)."""
        return RoICropPoolFunction.apply(features, rois, self.pooled_size, self.spatial_scale,
                                         self.max_pool if max_pool is None else bool(max_pool))
