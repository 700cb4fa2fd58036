"""Plain-NumPy restatement of the depth-edge metric (TEST INFRASTRUCTURE ONLY: the yardstick of
tests/test_edges.py and tests/test_edges_gpu.py; the product path is pldepth_amd/csrc/edges.hip).

  depth_edge_metric  pldepth/active_learning/metrics.py:123-144
  auto_canny         pldepth/active_learning/preprocess_utils.py:4-13

The reference calls OpenCV for three operators. OpenCV is not installed here, so they are
restated from its documented algorithms and are unpinned:
  minmax_u8        cv2.normalize(x, None, 0, 255, NORM_MINMAX).astype(np.uint8)
  canny            cv2.Canny(img, lo, hi): aperture 3, L1 gradient, replicated border,
                   non-maximum suppression in 2^15 fixed point, hysteresis with a stack
  chamfer_two_pass cv2.distanceTransform(mask, DIST_L2, 3): the two-pass 3x3 chamfer transform
                   in 16.16 fixed point
The reference's own arithmetic around them (thresholds, the > 10 cut, the sums and the division)
is pinned by tests/golden/edge_golden.npz (tests/golden/make_edge_golden.py).
"""
import numpy as np

HV_DIST = 62587    # round(0.955 * 2^16)
DIAG_DIST = 89738  # round(1.3693 * 2^16)
TG22 = 13573       # tan(22.5 deg) * 2^15
FAR = 1 << 40      # "infinitely far": outside the image


def minmax_f32(x, hi=255.0):
    """NORM_MINMAX to [0, hi] as float32: scale = hi / (max - min) in double (0 when
    max - min <= DBL_EPSILON), shift = -min * scale."""
    x = np.asarray(x, np.float32)
    smin, smax = float(x.min()), float(x.max())
    scale = hi / (smax - smin) if (smax - smin) > np.finfo(np.float64).eps else 0.0
    shift = -smin * scale
    return (x.astype(np.float64) * scale + shift).astype(np.float32)


def minmax_u8(x):
    """Truncation toward zero, clamped to [0, 255]."""
    return np.clip(np.trunc(minmax_f32(x)), 0, 255).astype(np.uint8)


def auto_thresholds(img, sigma=1.8):
    """preprocess_utils.py:6-9."""
    v = np.median(img)
    return int(max(0, (1.0 - sigma) * v)), int(min(255, (1.0 + sigma) * v))


def sobel_mag(img):
    """3x3 Sobel dx, dy (border replicated) and |dx| + |dy| as int64 arrays."""
    p = np.pad(np.asarray(img, np.uint8).astype(np.int64), 1, mode="edge")
    dx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    dy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    return dx, dy, np.abs(dx) + np.abs(dy)


def canny_labels(img, lo, hi):
    """0 = no edge candidate, 1 = weak candidate, 2 = strong, before hysteresis."""
    lo, hi = (hi, lo) if lo > hi else (lo, hi)
    dx, dy, mag = sobel_mag(img)
    h, w = mag.shape
    m = np.pad(mag, 1)  # 0 outside the image
    c = m[1:-1, 1:-1]

    def at(oy, ox):
        return m[1 + oy:1 + oy + h, 1 + ox:1 + ox + w]

    x = np.abs(dx)
    y = np.abs(dy) << 15
    t22 = x * TG22
    horiz = y < t22
    vert = ~horiz & (y > t22 + (x << 16))
    diag = ~horiz & ~vert
    same = (dx ^ dy) >= 0  # s = 1: compare up-left and down-right; s = -1: up-right, down-left
    keep = (horiz & (c > at(0, -1)) & (c >= at(0, 1))) | \
           (vert & (c > at(-1, 0)) & (c >= at(1, 0))) | \
           (diag & same & (c > at(-1, -1)) & (c > at(1, 1))) | \
           (diag & ~same & (c > at(-1, 1)) & (c > at(1, -1)))
    cand = keep & (c > lo)
    return np.where(cand, np.where(c > hi, 2, 1), 0).astype(np.uint8)


def hysteresis(labels):
    """255 on strong pixels and on weak ones 8-connected to a strong one through weak pixels."""
    lab = np.pad(labels, 1)
    stack = [(int(y), int(x)) for y, x in zip(*np.nonzero(lab == 2))]
    while stack:
        y, x = stack.pop()
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                if lab[y + oy, x + ox] == 1:
                    lab[y + oy, x + ox] = 2
                    stack.append((y + oy, x + ox))
    return np.where(lab[1:-1, 1:-1] == 2, 255, 0).astype(np.uint8)


def canny(img, lo, hi):
    return hysteresis(canny_labels(img, lo, hi))


def auto_canny(img, sigma=1.8):
    return canny(img, *auto_thresholds(img, sigma))


def chamfer_two_pass_fixed(mask):
    """The two-pass transform in 16.16 fixed point (int64; >= FAR where no zero pixel exists).
    Zero pixels stay 0, so only the non-zero ones are visited, in raster order and back."""
    mask = np.asarray(mask)
    h, w = mask.shape
    d = np.full((h + 2, w + 2), FAR, np.int64)
    d[1:-1, 1:-1] = np.where(mask != 0, FAR, 0)
    ys, xs = np.nonzero(mask)  # raster order
    for y, x in zip(ys.tolist(), xs.tolist()):
        y, x = y + 1, x + 1
        d[y, x] = min(d[y - 1, x - 1] + DIAG_DIST, d[y - 1, x] + HV_DIST,
                      d[y - 1, x + 1] + DIAG_DIST, d[y, x - 1] + HV_DIST)
    for y, x in zip(ys.tolist()[::-1], xs.tolist()[::-1]):
        y, x = y + 1, x + 1
        d[y, x] = min(d[y, x], d[y + 1, x + 1] + DIAG_DIST, d[y + 1, x] + HV_DIST,
                      d[y + 1, x - 1] + DIAG_DIST, d[y, x + 1] + HV_DIST)
    return d[1:-1, 1:-1]


def chamfer_dt3(mask, max_dist=10.0):
    """distanceTransform(mask, DIST_L2, 3) as float32 with values above max_dist (and pixels
    without any zero pixel in the image) set to 0."""
    f = chamfer_two_pass_fixed(mask)
    e = (np.minimum(f, 1 << 30).astype(np.float32) * np.float32(1.0 / 65536.0))
    e[(e > np.float32(max_dist)) | (f >= FAR)] = 0
    return e


def chamfer_window_fixed(mask, radius=10):
    """The per-pixel form the kernels evaluate: min over zero pixels within `radius` rows and
    columns of min(|dx|, |dy|) * 89738 + (max - min) * 62587 (FAR when there is none)."""
    mask = np.asarray(mask)
    h, w = mask.shape
    zero = np.pad(mask == 0, radius)  # outside the image: not a zero pixel
    best = np.full((h, w), FAR, np.int64)
    for oy in range(-radius, radius + 1):
        for ox in range(-radius, radius + 1):
            a, b = sorted((abs(oy), abs(ox)))
            cost = a * DIAG_DIST + (b - a) * HV_DIST
            z = zero[radius + oy:radius + oy + h, radius + ox:radius + ox + w]
            best = np.where(z & (cost < best), cost, best)
    return np.where(mask != 0, best, 0)


def edge_maps(op, gt):
    """Steps 1-3 for a prediction and a ground truth, each (H, W) or (H, W, 1)."""
    op = np.asarray(op, np.float32).reshape(np.shape(op)[:2])
    gt = np.asarray(gt, np.float32).reshape(np.shape(gt)[:2])
    return auto_canny(minmax_u8(op)), auto_canny(minmax_u8(gt))


def metric_exact_from_edges(E_op, E_gt):
    """(boundary, completeness) with integer sums: what the kernels must equal."""
    out = []
    for E_a, E_b in ((E_op, E_gt), (E_gt, E_op)):
        f = chamfer_two_pass_fixed(E_b)
        f = np.where(f > 10 * 65536, 0, f)  # fixed / 65536 > 10 (exact in float32)
        s = int(f[E_a != 0].sum())
        cnt = int(np.count_nonzero(E_a))
        with np.errstate(invalid="ignore"):
            out.append(float(np.float64(s / 65536.0) / np.float64(cnt)))
    return tuple(out)


def metric_as_reference_from_edges(Y_bin, Y_star_bin):
    """metrics.py:129-144 in the reference's own arithmetic: float32 products, np.sum."""
    e = chamfer_dt3(Y_bin, np.inf)
    e[e > 10] = 0
    e_star = chamfer_dt3(Y_star_bin, np.inf)
    e_star[e_star > 10] = 0
    with np.errstate(invalid="ignore"):
        b = np.divide(np.sum(e_star * Y_bin), np.sum(Y_bin))
        c = np.divide(np.sum(e * Y_star_bin), np.sum(Y_star_bin))
    return float(b), float(c)


def exact(op, gt):
    return metric_exact_from_edges(*edge_maps(op, gt))


def as_reference(op, gt):
    return metric_as_reference_from_edges(*edge_maps(op, gt))


def scene(h, w, seed):
    """A smooth synthetic depth map with two occluders: a ramp plus a rectangle plus a disc plus
    1 % noise, float32 (H, W, 1)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    d = 0.6 * yy + 0.2 * xx
    y0, x0 = rng.uniform(0.1, 0.4, 2)
    d = np.where((yy > y0) & (yy < y0 + 0.3) & (xx > x0) & (xx < x0 + 0.35), d + 0.5, d)
    cy, cx, r = rng.uniform(0.5, 0.8), rng.uniform(0.5, 0.8), rng.uniform(0.1, 0.18)
    d = np.where((yy - cy) ** 2 + (xx - cx) ** 2 < r * r, d - 0.4, d)
    d = d + 0.01 * rng.standard_normal((h, w))
    return d.astype(np.float32)[..., None]
