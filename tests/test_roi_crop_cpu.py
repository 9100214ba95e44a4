"""RoI crop (POOLING_MODE 'crop') without a GPU: the CPU restatement the GPU tests compare
against is itself checked against torch's grid_sample; the four C entry points reject bad
arguments on the host; a detector configured for 'crop' builds its pooling module."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_roi_crop as ref

B, H, W = 2, 7, 9


@pytest.mark.parametrize("C", [5, 67])
@pytest.mark.parametrize("G", [14, 7, 6, 3])  # P = 7 / 3, with and without the max-pool
def test_restatement_matches_grid_sample(C, G):
    """An independent second oracle: the float32 restatement (CUDA kernel order) against
    F.grid_sample(bilinear, zeros, align_corners=True) over F.affine_grid(align_corners=True),
    within 1e-5 * max|x|."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)
    rois = ref.edge_rois(H, W, B)
    got = ref.sample(x, ref.affine_grid_yx(rois, H, W, G))
    theta = torch.from_numpy(ref.theta(rois, H, W))
    grid_xy = F.affine_grid(theta, torch.Size((len(rois), 1, G, G)), align_corners=True)
    img = torch.from_numpy(rois[:, 0]).long()
    want = F.grid_sample(torch.from_numpy(x)[img], grid_xy, mode="bilinear",
                         padding_mode="zeros", align_corners=True).numpy()
    err = float(np.abs(got - want).max())
    print("max |restatement - grid_sample| =", err, "max|x| =", float(np.abs(x).max()))
    assert err <= 1e-5 * float(np.abs(x).max())
    # the torch version of the restatement is the same function
    got64 = ref.sample_t(torch.from_numpy(x).double(),
                         torch.from_numpy(ref.affine_grid_yx(rois, H, W, G))).numpy()
    assert float(np.abs(got64 - got).max()) <= 1e-5 * float(np.abs(x).max())


def test_restatement_edge_cases():
    """The RoI set really contains what the GPU tests rely on: a fully-outside RoI (all
    zeros), taps both inside and outside on each border, a degenerate RoI and the exact
    last-column coordinate."""
    rois = ref.edge_rois(H, W, B)
    grid = ref.affine_grid_yx(rois, H, W, 14)
    y0, _ = ref.get_top_left(grid[..., 0], H)
    x0, wx = ref.get_top_left(grid[..., 1], W)
    x = np.ones((B, 1, H, W), np.float32)
    out = ref.sample(x, grid)
    assert np.all(out[3] == 0) and np.all(out[9] == 0)            # entirely outside
    assert (x0[1] < -1).any() and (x0[1] == -1).any() and (x0[1] >= 0).any()
    assert (y0[1] < -1).any() and (y0[1] == -1).any() and (y0[1] >= 0).any()
    assert (x0[2] == W - 1).any() and (x0[2] > W - 1).any() and (x0[2] < W - 1).any()
    assert (y0[2] == H - 1).any() and (y0[2] > H - 1).any() and (y0[2] < H - 1).any()
    assert np.all(x0[4] == x0[4][0, 0])                           # x1 == x2: one column
    assert x0[5][0, -1] == W - 1 and wx[5][0, -1] == 1.0          # xcoord == W - 1 exactly
    assert x0[5][0, 0] == 2 and wx[5][0, 0] == 1.0                # integer corner


def test_max_pool_first_tie():
    v = np.zeros((1, 1, 2, 4), np.float32)
    v[0, 0, :, :2] = [[1, 3], [3, 2]]
    v[0, 0, :, 2:] = 5
    val, idx = ref.max_pool_2x2(v)
    assert val.tolist() == [[[[3.0, 5.0]]]] and idx.tolist() == [[[[1, 0]]]]


def test_entry_points_reject_bad_arguments_host_only():
    """W = 1, R % B != 0 and a null output are refused before any device work, each with a
    telling tlod_last_error (no GPU here)."""
    from tlod import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value

    def fwd(B_=2, W_=9, R=12, out=p):
        return L.tlod_roi_crop_fwd_f32(p, B_, 5, 7, W_, p, R, 14, 14, out, None)

    def bwd(B_=2, W_=9, R=12, out=p):
        return L.tlod_roi_crop_bwd_f32(p, p, R, 5, 14, 14, B_, 7, W_, out, None)

    def pfwd(W_=9, out=p, P=7, R=12):
        return L.tlod_roi_crop_pool_fwd_f32(p, 2, 5, 7, W_, p, R, P, 1 / 16, 1, out, p, None)

    def pbwd(W_=9, out=p, P=7, R=12):
        return L.tlod_roi_crop_pool_bwd_f32(p, p, 2, 5, 7, W_, p, R, P, 1 / 16, 1, out, None)

    for f in (fwd, bwd, pfwd, pbwd):
        assert f(W_=1) != 0
        assert b"W >= 2" in L.tlod_last_error(), L.tlod_last_error()
        assert f(out=None) != 0
        assert b"null" in L.tlod_last_error(), L.tlod_last_error()
    for f in (fwd, bwd):
        assert f(R=13) != 0
        assert b"R % B" in L.tlod_last_error(), L.tlod_last_error()
        assert f(R=0) != 0 and f(B_=0) != 0
        assert b"positive" in L.tlod_last_error(), L.tlod_last_error()
    for f in (pfwd, pbwd):
        assert f(P=17) != 0  # 2P = 34 samples per axis
        assert b"32 samples" in L.tlod_last_error(), L.tlod_last_error()
        assert f(P=0) != 0 and f(R=-1) != 0
    assert L.tlod_abi_version() == 1


def test_crop_model_constructs():
    """A detector under the reference's own defaults (POOLING_MODE 'crop', max-pool on) builds
    the crop module (no parameters: state_dict keys unchanged) and its _pool reaches it — on
    this CPU it stops at the product path's device check, not at a missing mode."""
    from tlod import config
    from tlod.config import cfg
    from tlod.da import daf
    from tlod.detector import faster_rcnn
    from tlod.roi_crop import RoICropPool
    saved = copy.deepcopy(cfg)
    config.reset_cfg()
    try:
        assert cfg.POOLING_MODE == "crop" and cfg.CROP_RESIZE_WITH_MAX_POOL
        for mod in (faster_rcnn, daf):
            m = mod.vgg16(("__background__", "a", "b"), pretrained=False, class_agnostic=False)
            m.create_architecture()
            assert isinstance(m.RCNN_roi_crop_pool, RoICropPool)
            assert m.RCNN_roi_crop_pool.max_pool and m.RCNN_roi_crop_pool.pooled_size == 7
            assert not any("roi_crop" in k for k in m.state_dict())
            with pytest.raises(RuntimeError, match="MI355X only"):
                m._pool(torch.zeros(1, 512, 7, 9), torch.zeros(2, 5))
    finally:
        cfg.clear()
        cfg.update(saved)
