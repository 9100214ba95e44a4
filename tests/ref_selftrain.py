"""The IDF self-training ops (csrc/selftrain.hip, include/tlod_selftrain.h) restated: the pseudo
ground-truth packer in numpy and EFocalLoss in fp64 torch.  Written from reading the reference's
offline label route, not copied from it:

  faster_rcnn_test.py:316-369   the kept rows class-major, str(int(x)) into the XML;
  foggy_cityscape.py:239-242    max(x - 1, 0) into an integer roidb;
  minibatch.py:39-49            integer box * Python-float im_scale, stored to float32;
  roibatchLoader.py             rows with x1 == x2 or y1 == y2 dropped, shuffle, [:max_gt];
  net_utils.py:73-102           EFocalLoss: mean -exp(-gamma p) log p, no clamp.

Where the loader shuffles and cuts, the packer keeps the max_gt survivors with the smallest
(rng_u64(seed, PSEUDO_STREAM, rank), rank) in ascending rank: device_rng.pick_order.

Every step a defect could plausibly touch goes through a module-level name (truncate,
zero_based, to_blob, rows_of, cap), so tests/test_selftrain_cpu.py can swap one for a defective
version and show that some case of ``packer_cases`` — the cases the GPU test runs — notices.
"""
import numpy as np
import torch

from device_rng import pick_order, rng_u64

PSEUDO_STREAM = 0x70736575


def truncate(x):
    """str(int(x)): toward zero.  x float32 -> float64 whole numbers."""
    return np.trunc(x.astype(np.float64))


def zero_based(t):
    """The IDF loaders' reader: max(t - 1, 0)."""
    return np.maximum(t - 1.0, 0.0)


def to_blob(v, im_scale):
    """The roidb's integer box times the loader's Python float, stored to float32 once."""
    return (v * float(im_scale)).astype(np.float32)


def rows_of(counts, j):
    """How many rows of class j are read."""
    return int(counts[j])


def cap(n, max_gt, seed):
    """Ranks kept when n > max_gt, ascending."""
    return pick_order(rng_u64(seed, PSEUDO_STREAM, np.arange(n)), max_gt)


def survivors(dets, counts, im_scale):
    """(n, 5) float32 rows (x1, y1, x2, y2, class) in blob coordinates, in rank order."""
    out = [np.zeros((0, 5), np.float32)]
    for j in range(1, dets.shape[0]):
        g = to_blob(zero_based(truncate(dets[j, :rows_of(counts, j), :4])), im_scale)
        keep = ~((g[:, 0] == g[:, 2]) | (g[:, 1] == g[:, 3]))
        out.append(np.concatenate([g[keep], np.full((int(keep.sum()), 1), j, np.float32)], 1))
    return np.concatenate(out).astype(np.float32)


def pseudo_gt(dets, counts, im_scale, max_gt, seed):
    """(gt_boxes (max_gt, 5) float32 zero padded, num_boxes int)."""
    rows = survivors(dets, counts, im_scale)
    if len(rows) > max_gt:
        rows = rows[cap(len(rows), max_gt, seed)]
    gt = np.zeros((max_gt, 5), np.float32)
    gt[:len(rows)] = rows
    return gt, len(rows)


# ------------------------------------------------------------------------------ the cases
NAN_FILL, HUGE_FILL = float("nan"), 3.0e38
SCALES = (600.0 / 1024.0, 1.0 / 3.0)
SEEDS = (0, (1 << 32) + 12345, (1 << 63) + 99)


def _boxes(rng, n, W=2048, H=1024):
    """n boxes no truncation makes degenerate (sides >= 8), fractional coordinates, some on the
    image's left / top edge (x or y below 1: the clamp acts)."""
    x1 = rng.uniform(0, W - 64, n)
    y1 = rng.uniform(0, H - 64, n)
    edge = rng.random(n)
    x1[edge < 0.15] = rng.uniform(0, 1, int((edge < 0.15).sum()))
    y1[edge > 0.85] = rng.uniform(0, 1, int((edge > 0.85).sum()))
    w, h = rng.uniform(8, 400, n), rng.uniform(8, 300, n)
    b = np.stack([x1, y1, np.minimum(x1 + w, W - 1), np.minimum(y1 + h, H - 1),
                  rng.uniform(0.5, 1, n)], 1)
    return b.astype(np.float32)


def make_case(name, C, R, counts, max_gt, im_scale, seed, fill, degenerate=(), frac=0.0, rs=0):
    """dets (C, R, 5) / counts (C,) int32 as tlod_detect_f32 leaves them, every row at or past
    counts[j] (class 0 included) holding ``fill``.  degenerate: slot ranks (class-major over the
    valid rows) whose box truncation collapses; frac: that share of the others, at random."""
    rng = np.random.default_rng(rs + 7 * C + R)
    counts = np.asarray(counts, np.int32)
    assert counts.shape == (C,) and counts[0] == 0 and counts.max() <= R
    dets = np.full((C, R, 5), fill, np.float32)
    k, n_valid = 0, int(counts.sum())
    degenerate = {d % n_valid for d in degenerate} if n_valid else set()
    for j in range(1, C):
        b = _boxes(rng, int(counts[j]))
        for i in range(int(counts[j])):
            if k in degenerate or rng.random() < frac:
                if (k + i) % 2:
                    b[i, 2] = b[i, 0] + (0.3 if b[i, 0] % 1 < 0.6 else 0.0)  # same whole part
                else:
                    b[i, 3] = np.float32(np.trunc(b[i, 1])) + 0.9
            k += 1
        dets[j, :counts[j]] = b
    return dict(name=name, C=C, R=R, dets=dets, counts=counts, max_gt=max_gt,
                im_scale=im_scale, seed=seed)


def _spread(C, R, n):
    """n rows over classes 1 .. C-1, at most R each, uneven."""
    counts = np.zeros(C, np.int64)
    j = 1
    while n > 0:
        take = min(R, n, 1 + (j * 7) % 5)
        if counts[j] + take <= R:
            counts[j] += take
            n -= take
        j = j % (C - 1) + 1
    return counts


def packer_cases():
    """The cases tests/test_selftrain_gpu.py holds the kernel to, bit for bit."""
    s0, s1 = SCALES
    z = lambda C: np.zeros(C, np.int64)
    cases = [make_case("all zero", 9, 300, z(9), 20, s0, SEEDS[0], NAN_FILL)]
    c = z(21); c[20] = 1
    cases.append(make_case("last class only", 21, 65, c, 50, s1, SEEDS[1], HUGE_FILL))
    c = z(9); c[1:4] = (64, 65, 129)
    cases.append(make_case("wave edges", 9, 300, c, 50, s1, SEEDS[2], NAN_FILL, frac=0.3))
    cases.append(make_case("wave edges, all kept rows", 9, 300, c, 50, s0, SEEDS[1], HUGE_FILL))
    for max_gt in (1, 20, 50):
        for extra in (0, 1):
            C, R = (9, 300) if max_gt != 1 else (2, 65)
            cases.append(make_case(f"n = max_gt + {extra} ({max_gt})", C, R,
                                   _spread(C, R, max_gt + extra), max_gt, s1 if extra else s0,
                                   SEEDS[(max_gt + extra) % 3], NAN_FILL if extra else HUGE_FILL))
    c = z(9); c[2], c[5], c[8] = 7, 3, 6
    cases.append(make_case("degenerate first and last", 9, 300, c, 20, s1, SEEDS[0], NAN_FILL,
                           degenerate=(0, -1)))
    cases.append(make_case("degenerate first and last, capped", 9, 65, _spread(9, 65, 70), 20,
                           s1, SEEDS[2], HUGE_FILL, degenerate=(0, -1), frac=0.2))
    cases.append(make_case("R = 1", 9, 1, np.array([0] + [1] * 8), 20, s1, SEEDS[1], NAN_FILL))
    cases.append(make_case("R = 1, C = 2, max_gt = 1", 2, 1, np.array([0, 1]), 1, s0, SEEDS[2],
                           HUGE_FILL))
    cases.append(make_case("one class, every row", 2, 2048, np.array([0, 2048]), 20, s1,
                           SEEDS[1], NAN_FILL, frac=0.1))
    c = np.full(21, 2048); c[0] = 0
    cases.append(make_case("n = (C - 1) R", 21, 2048, c, 50, s1, SEEDS[2], NAN_FILL))
    c = np.full(21, 300); c[0] = 0; c[7] = 0; c[20] = 299
    cases.append(make_case("n over many chunks", 21, 300, c, 50, s0, SEEDS[0], HUGE_FILL,
                           frac=0.5))
    return cases


# ------------------------------------------------------------------------------ EFocalLoss
def efocal_loss(z, label, gamma):
    """EFocalLoss(class_num=2, gamma) for one label, in z's dtype (fp64 in the tests):
    mean_r -exp(-gamma p_r) log p_r, p_r = softmax(z[r])[label]; alpha 1, no clamp."""
    p = torch.softmax(z, 1)[:, int(label)]
    return (-torch.exp(-gamma * p) * torch.log(p)).mean()

