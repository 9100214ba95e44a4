"""Microbenchmark of the RoI pooling kernels on the DAF step's shape (2 images, base feature
512 x 37 x 75, 256 source + 300 target RoIs of realistic sizes): RoIAlignAvg 7x7 forward and
backward (the sorted-tap gather by default, no atomics; TLOD_ROI_BWD_GATHER=0 the
global-atomic NHWC kernel), and the fused RoI crop + max-pool (POOLING_MODE 'crop', P = 7)
forward and backward, beside the unfused crop composition (affine_grid_gen + _RoICrop +
max_pool2d) for the same RoIs."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "transfer-learning-library-for-object-detection_amd"))
from tlod import _lib  # noqa: E402


def main():
    dev = "cuda"
    B, C, H, W = 2, 512, 37, 75
    rng = np.random.default_rng(0)
    rois = []
    for b, n in ((0, 256), (1, 300)):
        x1 = rng.uniform(0, W * 16 - 64, n)
        y1 = rng.uniform(0, H * 16 - 64, n)
        w = rng.uniform(32, 600, n)
        h = rng.uniform(32, 400, n)
        rois.append(np.stack([np.full(n, b), x1, y1, np.minimum(x1 + w, W * 16 - 1),
                              np.minimum(y1 + h, H * 16 - 1)], 1))
    r = torch.from_numpy(np.concatenate(rois).astype(np.float32)).to(dev)
    R = r.shape[0]
    top = torch.randn(R, C, 7, 7, device=dev)
    grad = torch.zeros(B, C, H, W, device=dev)
    L = _lib.lib()
    wsb = max(L.tlod_roi_align_avg_bwd_gather_workspace_bytes(B, C, H, W, R, 7, 7),
              L.tlod_roi_align_avg_bwd_workspace_bytes(B, C, H, W))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

    def timed(fn, n=20):
        for _ in range(3):
            fn()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(n):
            fn()
        e.record()
        torch.cuda.synchronize()
        return round(s.elapsed_time(e) / n * 1e3, 1)

    feat = torch.randn(B, C, H, W, device=dev)
    out = torch.empty(R, C, 7, 7, device=dev)
    st = _lib.stream_of(top)

    def align_fwd():
        _lib.check(L.tlod_roi_align_avg_fwd_f32(_lib.ptr(feat), B, C, H, W, _lib.ptr(r), R, 7, 7,
                                                1.0 / 16, _lib.ptr(out), st), "roi_align_avg_fwd")

    def align_bwd():
        _lib.check(L.tlod_roi_align_avg_bwd_f32(_lib.ptr(top), B, C, H, W, _lib.ptr(r), R, 7, 7,
                                                1.0 / 16, _lib.ptr(grad), _lib.ptr(ws), ws.numel(),
                                                st), "roi_align_avg_bwd")

    argmax = torch.empty(R, C, 7, 7, dtype=torch.uint8, device=dev)

    def crop_fwd():
        _lib.check(L.tlod_roi_crop_pool_fwd_f32(_lib.ptr(feat), B, C, H, W, _lib.ptr(r), R, 7,
                                                1.0 / 16, 1, _lib.ptr(out), _lib.ptr(argmax), st),
                   "roi_crop_pool_fwd")

    def crop_bwd():
        _lib.check(L.tlod_roi_crop_pool_bwd_f32(_lib.ptr(top), _lib.ptr(argmax), B, C, H, W,
                                                _lib.ptr(r), R, 7, 1.0 / 16, 1, _lib.ptr(grad), st),
                   "roi_crop_pool_bwd")

    kind = "atomic" if os.environ.get("TLOD_ROI_BWD_GATHER") == "0" else "gather"
    res = {"kernel": kind, "roi_align_avg_fwd_us": timed(align_fwd),
           "roi_align_avg_bwd_us": timed(align_bwd), "roi_crop_pool_fwd_us": timed(crop_fwd),
           "roi_crop_pool_bwd_us": timed(crop_bwd)}

    # the unfused composition (the general sampler needs equal RoI counts per image, in order:
    # the first 256 RoIs of each image)
    import torch.nn.functional as F
    from tlod.roi_crop import _RoICrop, affine_grid_gen
    re = torch.cat([r[:256], r[256:512]], 0)
    fx = feat.clone().requires_grad_()
    sampler = _RoICrop()
    state = {}

    def comp_fwd():
        gxy = affine_grid_gen(re, (H, W), 14)
        gyx = torch.stack([gxy[..., 1], gxy[..., 0]], 3).contiguous()
        state["y"] = F.max_pool2d(sampler(fx, gyx), 2, 2)

    def comp_bwd():
        fx.grad = None
        state["y"].backward(top[:512], retain_graph=True)

    res["unfused_crop_fwd_us_512rois"] = timed(comp_fwd, 5)
    res["unfused_crop_bwd_us_512rois"] = timed(comp_bwd, 5)
    # HBM bytes: what the fused forward moves at least (map + rois in, out + argmax out), and
    # what the unfused composition writes and reads back on top of that for the same R (the
    # grid and its (y, x)-swapped copy, the (R, C, 14, 14) sample map)
    grid_bytes, map_bytes = R * 14 * 14 * 2 * 4, R * C * 14 * 14 * 4
    res["fused_fwd_min_bytes"] = 4 * B * C * H * W + 20 * R + 5 * R * C * 49
    res["unfused_fwd_extra_bytes"] = 2 * (2 * grid_bytes + map_bytes)
    res.update({"R": R, "C": C, "map": [H, W]})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
