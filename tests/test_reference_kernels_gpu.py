"""Three-way parity on the MI355X: the reference's own compiled kernels (oracle/_ref/, built by
oracle/ref_build.py from a reference checkout; wrapped by oracle/ref_kernels.py), this
project's restatements (oracle/nms.py, oracle/roi.py, tests/ref_roi_crop.py) and the HIP
kernels of libtlod.  The restatements and the HIP kernels came from one reading of the
reference's CUDA; the compiled kernels are that CUDA itself.

Bars (none looser than the existing suite's): NMS keep lists, RoIPool argmax, RoIAlign /
RoIAlignAvg / RoIPool forward values and the crop sampler's restatement bit-exact; the crop
sampler's HIP kernel within 16 * 2^-24 * max|x|; backwards (float atomics in no fixed order on
the reference side) rtol 1e-5 / atol 1e-5, crop backward 1e-5 * max|grad_in|.

A named case beyond the shared edge RoIs (test_roi_pool_backward_inverted_after_rounding):
RoIs whose rounded extent is inverted pass no gradient through the reference's RoIPool gather;
a plain scatter through argmax (tlod_roi_pool_bwd_f32) would, the module's backward
(tlod_roi_pool_bwd_gather_f32) does not.

Every case takes byte copies of its inputs and compares them after each side's call.
This module reads only oracle/_ref/*.so, never the reference checkout.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

import ref_roi_crop as rcrop
from helpers import box_iou, clustered_boxes, random_boxes, sorted_dets
from oracle import nms as onms
from oracle import ref_kernels as rk
from oracle import roi as oroi
from test_ops_gpu import _rois

pytestmark = pytest.mark.gpu
if not rk.available():
    pytest.skip("reference kernels not built (no reference checkout at build time)",
                allow_module_level=True)

dev = "cuda"
SCALE = 1.0 / 16


def t(a):
    return torch.from_numpy(np.array(a)).to(dev)


def n(x):
    return x.detach().cpu().numpy()


@contextlib.contextmanager
def frozen(*tensors):
    """Read-only inputs: the tensors' bytes before and after the block are the same."""
    before = [n(x).tobytes() for x in tensors]
    yield
    for i, (x, b) in enumerate(zip(tensors, before)):
        assert n(x).tobytes() == b, f"input {i} was written to"


# ================================================================== NMS
def _dup_dets(seed=7, count=300):
    rng = np.random.default_rng(seed)
    b = clustered_boxes(rng, count, clusters=30)
    b[100:200] = b[100]  # 100 exact duplicates: IoU == 1
    return sorted_dets(b, rng)


def _degenerate_dets():
    """Zero-area (x2 = x1 - 1: the '+1' area is 0, a pair of them has IoU 0/0) and inverted
    (x2 < x1, y2 < y1: negative extents) boxes among ordinary ones."""
    rng = np.random.default_rng(9)
    b = clustered_boxes(rng, 200, clusters=12)
    b[10:20, 2] = b[10:20, 0] - 1          # zero width
    b[20:30, 3] = b[20:30, 1] - 1          # zero height
    b[30:34] = [50.0, 60.0, 49.0, 59.0]    # zero area, identical: 0 / 0
    b[40:60, 2] = b[40:60, 0] - 20         # inverted in x
    b[60:70, [0, 1, 2, 3]] = b[60:70, [2, 3, 0, 1]]  # fully inverted
    return sorted_dets(b.astype(np.float32), rng)


def _nms_dets(name):
    if name == "dup":
        return _dup_dets()
    if name == "degenerate":
        return _degenerate_dets()
    kind, count = name.split("-")
    count = int(count)
    rng = np.random.default_rng(1000 + count)
    boxes = clustered_boxes(rng, count) if kind == "clustered" else random_boxes(rng, count)
    return sorted_dets(boxes, rng)


NMS_CASES = [("random-1", 0.7), ("clustered-63", 0.7), ("clustered-64", 0.7),
             ("clustered-65", 0.7), ("clustered-129", 0.7), ("clustered-2000", 0.7),
             ("random-2000", 0.0), ("clustered-2000", 1.0), ("clustered-300", 0.3),
             ("dup", 0.7), ("dup", 1.0), ("degenerate", 0.5)]


def _tlod_nms(dd, thr, max_keep=0):
    from tlod.nms import nms
    k = nms(dd, thr, max_keep=max_keep)
    return np.zeros(0, np.int32) if isinstance(k, list) else n(k)


@pytest.mark.parametrize("name,thr", NMS_CASES)
def test_nms_three_way(name, thr):
    """reference kernel == oracle.nms == tlod.nms as exact int32 arrays, and the reference's
    count output equals their length.  ("dup", 1.0): IoU == thresh exactly, the strict '>'.)"""
    d = _nms_dets(name)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = onms.nms(d, thr)
    dd = t(d)
    with frozen(dd):
        buf, count = rk.nms_with_count(dd, thr)
    ref = n(buf)[:count]
    with frozen(dd):
        got = _tlod_nms(dd, thr)
    print(name, thr, "kept", count, "of", len(d))
    assert ref.dtype == np.int32 and got.dtype == np.int32 and want.dtype == np.int32
    assert count == len(want)
    np.testing.assert_array_equal(ref, want)
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(n(rk.nms(dd, thr)), ref)


@pytest.mark.parametrize("mk", [1, 64, 65])
def test_nms_max_keep_is_reference_prefix(mk):
    d = _nms_dets("clustered-2000")
    dd = t(d)
    with frozen(dd):
        full = n(rk.nms(dd, 0.7))
    assert len(full) > 65
    with frozen(dd):
        got = _tlod_nms(dd, 0.7, mk)
    np.testing.assert_array_equal(got, full[:mk])


# ================================================================== RoIAlign
ALIGN_CASES = [(2, 5, 9, 11, 24, 8, 8), (1, 3, 2, 2, 8, 2, 3), (2, 33, 12, 16, 40, 8, 8),
               (1, 4, 6, 5, 12, 4, 6)]


@functools.lru_cache(maxsize=None)
def _align_inputs(B, C, H, W, R, ah, aw):
    """(feat, rois, grad_out) and the reference kernel's own forward / backward, computed once
    and shared (read-only) by the tests of this case."""
    rng = np.random.default_rng(B * 1000 + C * 10 + R)
    f = rng.standard_normal((B, C, H, W)).astype(np.float32)
    r = _rois(rng, R, B, W * 16, H * 16, edge=True)
    g = rng.standard_normal((R, C, ah, aw)).astype(np.float32)
    fd, rd, gd = t(f), t(r), t(g)
    with frozen(fd, rd, gd):
        ref_fwd = n(rk.roi_align_fwd(fd, rd, ah, aw, SCALE))
        ref_bwd = n(rk.roi_align_bwd(gd, rd, B, C, H, W, SCALE))
    for a in (f, r, g, ref_fwd, ref_bwd):
        a.setflags(write=False)
    return f, r, g, ref_fwd, ref_bwd


@pytest.mark.parametrize("B,C,H,W,R,ah,aw", ALIGN_CASES)
def test_roi_align_forward_three_way(B, C, H, W, R, ah, aw):
    from tlod.roi_align import RoIAlignFunction
    f, r, _, ref_fwd, _ = _align_inputs(B, C, H, W, R, ah, aw)
    assert not np.isnan(ref_fwd).any(), "the reference left an output unwritten"
    np.testing.assert_array_equal(ref_fwd, oroi.roi_align_fwd(f, r, ah, aw, SCALE))
    fd, rd = t(f), t(r)
    with frozen(fd, rd):
        got = n(RoIAlignFunction.apply(fd, rd, ah, aw, SCALE))
    np.testing.assert_array_equal(got, ref_fwd)


@pytest.mark.parametrize("B,C,H,W,R,ah,aw", ALIGN_CASES)
def test_roi_align_avg_fused_vs_reference(B, C, H, W, R, ah, aw):
    """RoIAlignAvg(ah - 1, aw - 1) (7 x 7 from the 8 x 8 cases): the reference forward at
    ah x aw, then oracle.roi.avg_pool_2x2_s1 on the host == the fused kernel, bit-exact."""
    from tlod.roi_align import RoIAlignAvg
    f, r, _, ref_fwd, _ = _align_inputs(B, C, H, W, R, ah, aw)
    want = oroi.avg_pool_2x2_s1(ref_fwd)
    fd, rd = t(f), t(r)
    with frozen(fd, rd):
        got = n(RoIAlignAvg(ah - 1, aw - 1, SCALE)(fd, rd))
    assert got.shape == (R, C, ah - 1, aw - 1)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("B,C,H,W,R,ah,aw", ALIGN_CASES)
def test_roi_align_backward_three_way(B, C, H, W, R, ah, aw):
    """The reference adds with float atomicAdd in no fixed order: no bit bar.  rtol / atol
    1e-5 (the family's bar) against the oracle and the HIP kernel; same set of non-zero cells.
    The plain RoIAlign backward has one path only (atomics): TLOD_ROI_BWD_GATHER switches the
    fused RoIAlignAvg backward alone, whose two paths the next test covers."""
    from tlod.roi_align import RoIAlignFunction
    f, r, g, _, ref_bwd = _align_inputs(B, C, H, W, R, ah, aw)
    want = oroi.roi_align_bwd(g, r, B, C, H, W, SCALE)
    np.testing.assert_allclose(ref_bwd, want, rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(ref_bwd != 0, want != 0)
    fd, rd, gd = t(f).requires_grad_(True), t(r), t(g)
    with frozen(rd, gd):
        RoIAlignFunction.apply(fd, rd, ah, aw, SCALE).backward(gd)
    got = n(fd.grad)
    print("max |hip - reference| =", float(np.abs(got - ref_bwd).max()))
    np.testing.assert_allclose(got, ref_bwd, rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(got != 0, ref_bwd != 0)


@pytest.mark.parametrize("path", ["gather", "atomic"])
@pytest.mark.parametrize("B,C,H,W,R,ah,aw", ALIGN_CASES)
def test_roi_align_avg_backward_vs_reference(B, C, H, W, R, ah, aw, path, monkeypatch):
    """The fused RoIAlignAvg backward, on the sorted-tap gather and on the atomic kernels,
    against the reference's RoIAlign backward fed with the avg-pool's backward
    (oracle.roi.avg_pool_2x2_s1_bwd, on the host)."""
    from tlod.roi_align import RoIAlignAvg
    monkeypatch.setenv("TLOD_ROI_BWD_GATHER", "1" if path == "gather" else "0")
    f, r, _, _, _ = _align_inputs(B, C, H, W, R, ah, aw)
    g = np.random.default_rng(R + ah).standard_normal((R, C, ah - 1, aw - 1)).astype(np.float32)
    fd, rd, gd = t(f).requires_grad_(True), t(r), t(g)
    ga = t(oroi.avg_pool_2x2_s1_bwd(g))
    with frozen(rd, ga):
        ref_bwd = n(rk.roi_align_bwd(ga, rd, B, C, H, W, SCALE))
    with frozen(rd, gd):
        RoIAlignAvg(ah - 1, aw - 1, SCALE)(fd, rd).backward(gd)
    got = n(fd.grad)
    print(path, "max |hip - reference| =", float(np.abs(got - ref_bwd).max()))
    np.testing.assert_allclose(got, ref_bwd, rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(got != 0, ref_bwd != 0)


# ================================================================== RoIPool
POOL_CASES = [(2, 5, 9, 11, 24, 7), (1, 3, 4, 5, 10, 3), (2, 16, 20, 25, 40, 7)]


def _tied_features(rng, B, C, H, W):
    """Exact ties inside the windows: every third column equals its left neighbour, so the
    strict '>' scan's first-maximum rule decides the argmax."""
    f = rng.standard_normal((B, C, H, W)).astype(np.float32)
    for w in range(1, W, 3):
        f[..., w] = f[..., w - 1]
    return f


@functools.lru_cache(maxsize=None)
def _pool_inputs(B, C, H, W, R, P):
    rng = np.random.default_rng(B * 1000 + C * 10 + R + P)
    f = _tied_features(rng, B, C, H, W)
    r = _rois(rng, R, B, W * 16, H * 16, edge=True)
    g = rng.standard_normal((R, C, P, P)).astype(np.float32)
    for a in (f, r, g):
        a.setflags(write=False)
    return f, r, g


@pytest.mark.parametrize("B,C,H,W,R,P", POOL_CASES)
def test_roi_pool_three_way(B, C, H, W, R, P):
    from tlod import _lib
    from tlod.roi_pool import roi_pool_with_argmax
    f, r, g = _pool_inputs(B, C, H, W, R, P)
    assert np.array_equal(f[..., 1], f[..., 0]) and np.array_equal(f[..., 4], f[..., 3])
    fd, rd, gd = t(f), t(r), t(g)
    with frozen(fd, rd):
        ref_out, ref_arg = rk.roi_pool_fwd(fd, rd, P, P, SCALE)
    want_out, want_arg = oroi.roi_pool_fwd(f, r, P, P, SCALE)
    ro, ra = n(ref_out), n(ref_arg)
    assert ra.dtype == np.int32 and want_arg.dtype == np.int32
    assert not np.isnan(ro).any() and ra.min() >= -1, "the reference left an output unwritten"
    assert (ra == -1).any(), "no empty bin: the RoIs past the map should give some"
    np.testing.assert_array_equal(ra, want_arg)
    np.testing.assert_array_equal(ro, want_out)
    np.testing.assert_array_equal(ro[ra == -1], 0)
    with frozen(fd, rd):
        out, arg = roi_pool_with_argmax(fd, rd, P, P, SCALE)
    assert arg.dtype == torch.int32
    np.testing.assert_array_equal(n(arg), ra)
    np.testing.assert_array_equal(n(out), ro)

    # backward, through the reference's own argmax: its deterministic per-element gather,
    # the oracle, and the HIP scatter
    with frozen(gd, ref_arg, rd):
        ref_bwd = n(rk.roi_pool_bwd(gd, ref_arg, rd, B, C, H, W, SCALE))
    assert not np.isnan(ref_bwd).any()
    np.testing.assert_allclose(ref_bwd, oroi.roi_pool_bwd(g, ra, r, B, C, H, W, SCALE),
                               rtol=1e-5, atol=1e-5)
    grad = torch.zeros((B, C, H, W), dtype=torch.float32, device=dev)
    with frozen(gd, ref_arg, rd):
        _lib.check(_lib.lib().tlod_roi_pool_bwd_gather_f32(
            _lib.ptr(gd), _lib.ptr(ref_arg), B, C, H, W, _lib.ptr(rd), R, P, P, SCALE,
            _lib.ptr(grad), _lib.stream_of(gd)), "bwd")
        torch.cuda.synchronize()
    print("max |hip - reference| =", float(np.abs(n(grad) - ref_bwd).max()))
    np.testing.assert_allclose(n(grad), ref_bwd, rtol=1e-5, atol=1e-5)


def test_roi_pool_backward_inverted_after_rounding():
    """RoIs whose *rounded* extent is inverted (round(x2 / 16) < round(x1 / 16); the edge set's
    [100, 100, 90, 95] rounds to a proper 1 x 1 box and does not reach this).  The forward
    forces them to 1 x 1 and pools the cell at (start_h, start_w); the reference's backward
    gather then skips that cell, because it lies outside the inclusive [start, end] extent
    (roi_pooling_kernel.cu:162-166), so such a RoI passes no gradient.  A scatter through
    argmax alone adds it.  Through the module's autograd, against the reference kernel."""
    from tlod.roi_pool import roi_pool_with_argmax
    B, C, H, W, P = 2, 4, 12, 15, 7
    rng = np.random.default_rng(21)
    f = rng.standard_normal((B, C, H, W)).astype(np.float32)
    r = np.array([[0, 200, 150, 100, 60],      # inverted both ways
                  [1, 100, 50, 20, 120],       # inverted in x only
                  [0, 30, 160, 150, 40],       # inverted in y only
                  [1, 16, 16, 120, 100],       # proper
                  [0, 100, 100, 90, 95]], np.float32)
    g = rng.standard_normal((len(r), C, P, P)).astype(np.float32)
    fd, rd, gd = t(f), t(r), t(g)
    with frozen(fd, rd, gd):
        ref_out, ref_arg = rk.roi_pool_fwd(fd, rd, P, P, SCALE)
        with frozen(ref_arg):
            ref_bwd = n(rk.roi_pool_bwd(gd, ref_arg, rd, B, C, H, W, SCALE))
    assert (n(ref_arg)[:3] >= 0).all()  # the inverted RoIs do pool a cell each
    np.testing.assert_allclose(ref_bwd, oroi.roi_pool_bwd(g, n(ref_arg), r, B, C, H, W, SCALE),
                               rtol=1e-5, atol=1e-5)
    only_proper = g.copy()
    only_proper[:3] = 0
    opd = t(only_proper)
    with frozen(opd, ref_arg, rd):
        proper_bwd = n(rk.roi_pool_bwd(opd, ref_arg, rd, B, C, H, W, SCALE))
    # the reference: no gradient through the three inverted RoIs
    np.testing.assert_allclose(ref_bwd, proper_bwd, rtol=1e-5, atol=1e-5)
    fg = t(f).requires_grad_(True)
    with frozen(fg, rd, gd):
        out, arg = roi_pool_with_argmax(fg, rd, P, P, SCALE)
        out.backward(gd)
    np.testing.assert_array_equal(n(arg), n(ref_arg))
    np.testing.assert_array_equal(n(out), n(ref_out))
    np.testing.assert_allclose(n(fg.grad), ref_bwd, rtol=1e-5, atol=1e-5)


# ================================================================== RoICrop sampler
CB, CH, CW = 2, 7, 9
CROP_CASES = [(C, G) for C in (5, 67) for G in (14, 7, 3)]


@functools.lru_cache(maxsize=None)
def _crop_inputs(C, G):
    x = rcrop.ramp_map(np.random.default_rng(11 + C), CB, C, CH, CW)
    rois = rcrop.edge_rois(CH, CW, CB)
    grid = rcrop.affine_grid_yx(rois, CH, CW, G)
    go = np.random.default_rng(5).standard_normal((len(rois), C, G, G)).astype(np.float32)
    for a in (x, grid, go):
        a.setflags(write=False)
    return x, grid, go


@pytest.mark.parametrize("C,G", CROP_CASES)
def test_roi_crop_forward_three_way(C, G):
    from tlod import _lib
    x, grid, _ = _crop_inputs(C, G)
    R = grid.shape[0]
    xd, gd = t(x), t(grid)
    with frozen(xd, gd):
        ref = n(rk.roi_crop_fwd(xd, gd))
    want = rcrop.sample(x, grid)
    # the restatement claims the kernel's operation order: bit-exact
    np.testing.assert_array_equal(ref, want)
    assert not ref[3].any() and not ref[9].any()  # the RoIs entirely outside the map
    out = torch.full((R, C, G, G), float("nan"), device=dev)
    with frozen(xd, gd):
        _lib.check(_lib.lib().tlod_roi_crop_fwd_f32(_lib.ptr(xd), CB, C, CH, CW, _lib.ptr(gd), R,
                                                    G, G, _lib.ptr(out), _lib.stream_of(xd)), "fwd")
        got = n(out)
    assert not np.isnan(got).any()
    err = float(np.abs(got - ref).max())
    print("hip vs reference max |err| =", err, "bit-equal:", bool(np.array_equal(got, ref)))
    assert err <= 16 * 2.0 ** -24 * float(np.abs(x).max())


@pytest.mark.parametrize("C,G", CROP_CASES)
def test_roi_crop_backward_three_way(C, G):
    from tlod.roi_crop import _RoICrop
    x, grid, go = _crop_inputs(C, G)
    xd, gd, god = t(x), t(grid), t(go)
    with frozen(xd, gd, god):
        ref_gin, ref_ggrid = rk.roi_crop_bwd(xd, gd, god)
    ref_gin = n(ref_gin)
    assert not n(ref_ggrid).any()  # the kernel never writes the grid gradient
    bar = 1e-5 * float(np.abs(ref_gin).max())
    x64 = torch.from_numpy(np.array(x)).double().requires_grad_()
    rcrop.sample_t(x64, torch.from_numpy(np.array(grid))).backward(torch.from_numpy(np.array(go)).double())
    err_o = float(np.abs(ref_gin - x64.grad.numpy()).max())
    xg, gg = t(x).requires_grad_(), t(grid).requires_grad_()
    with frozen(gg, god):
        _RoICrop()(xg, gg).backward(god)
    assert gg.grad is None or not gg.grad.any()  # no grid gradient from the project either
    err_h = float(np.abs(n(xg.grad) - ref_gin).max())
    print("reference vs fp64 autograd", err_o, "hip vs reference", err_h, "bar", bar)
    assert err_o <= bar
    assert err_h <= bar


# ================================================================== contraction
CONTRACTION_NMS = [("clustered-300", 0.3), ("clustered-129", 0.7), ("random-2000", 0.5)]


def _spaced_features(rng, B, C, H, W):
    """Each (b, c) plane a permutation of H*W equally spaced values in [-2, 2]: any two cells
    of a plane (so the top two of any window) differ by at least 4 / (H*W - 1)."""
    planes = np.stack([rng.permutation(H * W) for _ in range(B * C)]).astype(np.float64)
    return (planes / (H * W - 1) * 4 - 2).reshape(B, C, H, W).astype(np.float32)


def test_reference_contraction_gap():
    """nvcc contracts a*b+c into fma by default; the HIP kernels and the restatements follow
    the uncontracted arithmetic.  This compares the reference's own two builds
    (-ffp-contract=off against hipcc's default contraction) on the cases above; neither side
    is the code under test.  Values within 1e-5 * max|x| (the family's bar); RoIPool argmax
    and NMS keep lists equal, on inputs shown here in float64 to have no pair's IoU within
    1e-5 of the threshold and no two cells of a plane within 1e-4 * max|x|.

    Measured on the MI355X (largest deviation, relative to max|x| of its case): RoIAlign
    forward 2.074e-06, RoIAlign backward 7.2e-07 to 8.1e-07 (float atomics in no fixed
    order on both sides), RoICrop backward 6.217e-07, RoICrop forward, RoIPool
    forward and backward 0 (bit-equal); argmax and keep lists equal.
    """
    worst = {}

    def gap(key, a, b, scale):
        a, b = n(a), n(b)
        rel = float(np.abs(a - b).max()) / scale
        worst[key] = max(worst.get(key, 0.0), rel)
        assert rel <= 1e-5, (key, rel)

    for case in ALIGN_CASES:
        B, C, H, W, R, ah, aw = case
        f, r, g, ref_fwd, ref_bwd = _align_inputs(*case)
        fd, rd, gd = t(f), t(r), t(g)
        with frozen(fd, rd, gd):
            fma_fwd = rk.roi_align_fwd(fd, rd, ah, aw, SCALE, variant="fma")
            fma_bwd = rk.roi_align_bwd(gd, rd, B, C, H, W, SCALE, variant="fma")
        gap("roi_align_fwd", fma_fwd, torch.from_numpy(np.array(ref_fwd)),
            float(np.abs(f).max()))
        gap("roi_align_bwd", fma_bwd, torch.from_numpy(np.array(ref_bwd)),
            float(np.abs(ref_bwd).max()))

    for B, C, H, W, R, P in POOL_CASES:
        rng = np.random.default_rng(77 + C)
        f = _spaced_features(rng, B, C, H, W)
        scale = float(np.abs(f).max())
        planes = np.sort(f.astype(np.float64).reshape(B * C, -1), axis=1)
        assert np.diff(planes, axis=1).min() > 1e-4 * scale  # float64: no near-tied window
        r = _rois(rng, R, B, W * 16, H * 16, edge=True)
        g = rng.standard_normal((R, C, P, P)).astype(np.float32)
        fd, rd, gd = t(f), t(r), t(g)
        with frozen(fd, rd, gd):
            o0, a0 = rk.roi_pool_fwd(fd, rd, P, P, SCALE)
            o1, a1 = rk.roi_pool_fwd(fd, rd, P, P, SCALE, variant="fma")
            with frozen(a0):
                b0 = rk.roi_pool_bwd(gd, a0, rd, B, C, H, W, SCALE)
                b1 = rk.roi_pool_bwd(gd, a0, rd, B, C, H, W, SCALE, variant="fma")
        np.testing.assert_array_equal(n(a0), n(a1))
        gap("roi_pool_fwd", o0, o1, scale)
        gap("roi_pool_bwd", b0, b1, float(np.abs(n(b0)).max()))

    for C, G in CROP_CASES:
        x, grid, go = _crop_inputs(C, G)
        xd, gd, god = t(x), t(grid), t(go)
        with frozen(xd, gd, god):
            v0, v1 = rk.roi_crop_fwd(xd, gd), rk.roi_crop_fwd(xd, gd, variant="fma")
            g0 = rk.roi_crop_bwd(xd, gd, god)[0]
            g1 = rk.roi_crop_bwd(xd, gd, god, variant="fma")[0]
        gap("roi_crop_fwd", v0, v1, float(np.abs(x).max()))
        gap("roi_crop_bwd", g0, g1, float(np.abs(n(g0)).max()))

    for name, thr in CONTRACTION_NMS:
        d = _nms_dets(name)
        iou = box_iou(d[:, :4], d[:, :4])[np.triu_indices(len(d), 1)]
        margin = float(np.abs(iou - thr).min())
        print(name, thr, "closest IoU to the threshold:", margin)
        assert margin > 1e-5  # float64: no pair decided by the last bits
        dd = t(d)
        with frozen(dd):
            k0, k1 = n(rk.nms(dd, thr)), n(rk.nms(dd, thr, variant="fma"))
        np.testing.assert_array_equal(k0, k1)
    print("contraction gap (relative):", {k: f"{v:.3e}" for k, v in sorted(worst.items())})
