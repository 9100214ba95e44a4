"""CPU restatement of the reference's RoI crop path, for the roi_crop tests (the oracle
package has no crop):

  * numpy float32, in the CUDA kernel's operation order
    (lib/model/roi_crop/src/roi_crop_cuda_kernel.cu:11-109: getTopLeft, the four in-bounds
    tests, the weighted sum left to right), the affine theta and grid of
    net_utils._affine_grid_gen (F.affine_grid with a base grid spanning [-1, 1] inclusive), the
    (y, x) swap of faster_rcnn.py:73-81, and F.max_pool2d(2, 2) with first-in-row-major ties;
  * the same in torch (fp64 by default), differentiable in the input, whose autograd is the
    reference gradient: the four weights times grad_out scattered to the taps, the grid
    detached (the CUDA backward never writes the grid gradient).
"""
import numpy as np
import torch
import torch.nn.functional as F

f32 = np.float32


def get_top_left(x, size):
    """getTopLeft: (point, weight) of float32 coordinates x in [-1, 1] on an axis of `size`."""
    x = np.asarray(x, f32)
    xcoord = (x + f32(1)) * f32(size - 1) / f32(2)
    point = np.floor(xcoord)
    weight = f32(1) - (xcoord - point)
    return point.astype(np.int64), weight.astype(f32)


def sample(x, grid_yx):
    """bilinearSamplingFromGrid: x (B,C,H,W) f32, grid (R,gh,gw,2) in (y, x) order -> (R,C,gh,gw).
    Grid r samples image r // (R // B).  A sample with no tap inside stays 0."""
    x = np.asarray(x, f32)
    B, C, H, W = x.shape
    R, gh, gw, _ = grid_yx.shape
    per = R // B
    y0, wy = get_top_left(grid_yx[..., 0], H)
    x0, wx = get_top_left(grid_yx[..., 1], W)
    out = np.zeros((R, C, gh, gw), f32)
    for r in range(R):
        img = x[r // per]

        def tap(yy, xx):
            ok = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
            v = img[:, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
            return np.where(ok[None], v, f32(0)).astype(f32)

        yw, xw = wy[r][None], wx[r][None]
        tl, tr = tap(y0[r], x0[r]), tap(y0[r], x0[r] + 1)
        bl, br = tap(y0[r] + 1, x0[r]), tap(y0[r] + 1, x0[r] + 1)
        out[r] = (xw * yw * tl + (f32(1) - xw) * yw * tr + xw * (f32(1) - yw) * bl
                  + (f32(1) - xw) * (f32(1) - yw) * br)
    return out


def theta(rois, H, W):
    """net_utils.py:145-160 in float32: (R, 2, 3)."""
    rois = np.asarray(rois, f32)
    x1, y1, x2, y2 = (rois[:, i] / f32(16.0) for i in (1, 2, 3, 4))
    zero = np.zeros_like(x1)
    th = np.stack([(x2 - x1) / f32(W - 1), zero, (x1 + x2 - f32(W) + f32(1)) / f32(W - 1),
                   zero, (y2 - y1) / f32(H - 1), (y1 + y2 - f32(H) + f32(1)) / f32(H - 1)], 1)
    return th.reshape(-1, 2, 3).astype(f32)


def affine_grid_yx(rois, H, W, G):
    """theta -> F.affine_grid over a G x G base grid spanning [-1, 1] inclusive -> swapped to
    (y, x): (R, G, G, 2) float32."""
    th = theta(rois, H, W)
    base = np.linspace(-1, 1, G).astype(f32) if G > 1 else np.array([-1], f32)
    gx = th[:, 0, 0, None] * base[None] + th[:, 0, 2, None]  # (R, G): x depends on the column
    gy = th[:, 1, 1, None] * base[None] + th[:, 1, 2, None]  # y on the row
    R = th.shape[0]
    grid = np.empty((R, G, G, 2), f32)
    grid[..., 0] = gy[:, :, None]
    grid[..., 1] = gx[:, None, :]
    return grid


def max_pool_2x2(v):
    """F.max_pool2d(v, 2, 2) and the winner's position in its window (row-major, first on
    ties)."""
    R, C, Hh, Ww = v.shape
    w = v.reshape(R, C, Hh // 2, 2, Ww // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(
        R, C, Hh // 2, Ww // 2, 4)
    idx = np.argmax(w, -1)  # the first maximum
    return np.take_along_axis(w, idx[..., None], -1)[..., 0], idx.astype(np.uint8)


def crop_pool(x, rois, P, max_pool):
    """The composition the detectors run (equal RoI counts per image, in image order)."""
    B, C, H, W = x.shape
    G = 2 * P if max_pool else P
    v = sample(x, affine_grid_yx(rois, H, W, G))
    return max_pool_2x2(v)[0] if max_pool else v


def window_gap(v):
    """Per 2x2 window of v (R,C,2P,2P): the maximum minus the largest candidate that is not
    exactly equal to it (inf when all four are equal), and whether all four are zero.
    Candidates exactly equal to the maximum are one candidate: an exact tie goes to the first
    in row-major order in every implementation (a degenerate RoI samples one column twice,
    taps outside the map are exact zeros), so it leaves the routing unambiguous."""
    R, C, Hh, Ww = v.shape
    w = v.reshape(R, C, Hh // 2, 2, Ww // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(
        R, C, Hh // 2, Ww // 2, 4)
    top = w.max(-1, keepdims=True)
    rest = np.where(w == top, -np.inf, w).max(-1)
    return top[..., 0] - rest, np.all(w == 0, -1)


def ramp_map(rng, B, C, H, W, noise=0.03):
    """A positive (B,C,H,W) float32 map whose 2x2 sample windows have a clear winner: per
    channel a plane a*x + b*y (|a|, |b| in [0.25, 0.5], random signs: bilinear samples of a
    plane differ by the sample spacing times the slope) around a level of 4.5 +- 0.5 (so a
    window on the border, where samples fade to the zero padding, is led by its innermost
    sample and not by a near-zero one), plus uniform noise of +-`noise`."""
    a = rng.uniform(0.25, 0.5, (B, C, 1, 1)) * rng.choice([-1.0, 1.0], (B, C, 1, 1))
    b = rng.uniform(0.25, 0.5, (B, C, 1, 1)) * rng.choice([-1.0, 1.0], (B, C, 1, 1))
    yy, xx = np.meshgrid(np.arange(H) - (H - 1) / 2, np.arange(W) - (W - 1) / 2, indexing="ij")
    x = (4.5 + rng.uniform(-0.5, 0.5, (B, C, 1, 1)) + a * xx + b * yy
         + rng.uniform(-noise, noise, (B, C, H, W)))
    return x.astype(f32)


# ---------------------------------------------------------------- torch (autograd) version
def sample_t(x, grid_yx):
    """sample() in torch at x's dtype, differentiable in x; the grid is a constant."""
    B, C, H, W = x.shape
    grid_yx = grid_yx.detach().to(x.dtype)
    R, gh, gw, _ = grid_yx.shape
    per = R // B
    img = torch.arange(R, device=x.device) // per

    def top_left(g, size):
        c = (g + 1) * (size - 1) / 2
        p = torch.floor(c)
        return p.long(), 1 - (c - p)

    y0, wy = top_left(grid_yx[..., 0], H)
    x0, wx = top_left(grid_yx[..., 1], W)

    def tap(yy, xx):
        ok = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
        flat = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).view(R, 1, gh * gw).expand(R, C, -1)
        v = x[img].reshape(R, C, H * W).gather(2, flat).view(R, C, gh, gw)
        return v * ok[:, None].to(x.dtype)

    yw, xw = wy[:, None], wx[:, None]
    return (xw * yw * tap(y0, x0) + (1 - xw) * yw * tap(y0, x0 + 1)
            + xw * (1 - yw) * tap(y0 + 1, x0) + (1 - xw) * (1 - yw) * tap(y0 + 1, x0 + 1))


def crop_pool_t(x, rois, P, max_pool):
    """crop_pool() in torch at x's dtype (the grid from the float32 restatement, so both
    versions sample the same points), differentiable in x."""
    B, C, H, W = x.shape
    G = 2 * P if max_pool else P
    grid = torch.from_numpy(affine_grid_yx(np.asarray(rois, f32), H, W, G)).to(x.device)
    v = sample_t(x, grid)
    return F.max_pool2d(v, 2, 2) if max_pool else v


# ---------------------------------------------------------------- shared test inputs
def edge_rois(H, W, B):
    """Six RoIs per image (image coords, stride 16), image-major: well inside; straddling the
    left / top borders; straddling the right / bottom borders; entirely outside; degenerate
    (x1 == x2); corners on integer cells with x2 on the last column (xcoord == W - 1)."""
    per = np.array([
        [16 * 1.3, 16 * 1.7, 16 * (W - 2.4), 16 * (H - 2.2)],
        [-16 * 3.3, -16 * 2.6, 16 * 3.7, 16 * 2.9],
        [16 * (W - 3.6), 16 * (H - 2.7), 16 * (W + 2.2), 16 * (H + 1.9)],
        [16 * (W + 3.0), 16 * (H + 2.0), 16 * (W + 6.5), 16 * (H + 5.5)],
        [16 * 4.25, 16 * 1.1, 16 * 4.25, 16 * 5.3],
        [16 * 2.0, 16 * 1.0, 16 * (W - 1.0), 16 * (H - 2.0)],
    ], f32)
    rows = []
    for b in range(B):
        p = per.copy()
        p[:3] += f32(b * 3.0)  # the second image's boxes differ a little
        rows.append(np.concatenate([np.full((len(p), 1), b, f32), p], 1))
    return np.concatenate(rows, 0).astype(f32)
