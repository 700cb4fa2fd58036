"""NumPy restatement of the four test-set evaluation kernels (pldepth_amd/csrc/evalset.hip).

tests/test_evalset.py shows that these functions reproduce tests/golden/evalset_golden.npz, which
the reference's generic_ranking_provider and scipy.ndimage wrote; the GPU tests then compare the
kernels with them on inputs the fixture does not hold.
"""
import numpy as np


def depth_relation(z0, z1, tau):
    """depth_utils.get_depth_relation on float32 arrays (NumPy 2 promotion): int array."""
    z0, z1 = np.asarray(z0, np.float32), np.asarray(z1, np.float32)
    if tau is None:
        return (z0 > z1).astype(np.int64) - (z0 < z1)
    eps = np.float32(1e-10)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (z0 + eps) / (z1 + eps)
    hi, lo = np.float32(1.0 + tau), np.float32(1.0 / (1.0 + tau))
    return np.where(ratio >= hi, 1, np.where(ratio <= lo, -1, 0))


def ordinal_pairs(gts, coords, tau=0.03, invert=False):
    """gts [n, h, w] float32, coords [n, P, 4] (x0, y0, x1, y1) -> [n, P, 5] float32."""
    gts = np.asarray(gts, np.float32)
    n, h, w = gts.shape
    c = np.asarray(coords, np.int64)
    im = np.arange(n)[:, None]
    z0, z1 = gts[im, c[..., 0], c[..., 1]], gts[im, c[..., 2], c[..., 3]]
    rel = depth_relation(z0, z1, tau) * (-1 if invert else 1)
    return np.stack([c[..., 0] * w + c[..., 1], c[..., 2] * w + c[..., 3], rel, z0, z1],
                    -1).astype(np.float32)


def depth_rankings(gts, idx, invert=False):
    """gts [n, ...] float32, idx [n, R, L] -> [n, R, L, 2] float32 under the stated tie rule:
    ascending is a stable sort by list position, descending is that order reversed."""
    gts = np.asarray(gts, np.float32)
    flat = gts.reshape(gts.shape[0], -1)
    idx = np.asarray(idx, np.int64)
    z = flat[np.arange(len(flat))[:, None, None], idx]
    order = np.argsort(z, axis=-1, kind="stable")
    if not invert:
        order = order[..., ::-1]
    zs = np.take_along_axis(z, order, -1)
    dep = (1.0 / (zs.astype(np.float64) + 1.0)).astype(np.float32) if invert else zs
    return np.stack([np.take_along_axis(idx, order, -1).astype(np.float32), dep], -1)


def ordinal_pair_error(pred, pairs, tau=None, invert=False):
    """pred [n, ...], pairs [n, P, 5] -> (wrong [n], counted [n]); tau=None reads the table's
    relations, else they are recomputed from its depths."""
    pred = np.asarray(pred, np.float32)
    flat = pred.reshape(pred.shape[0], -1)
    pairs = np.asarray(pairs, np.float32)
    if tau is None:
        rel = np.sign(pairs[..., 2]).astype(np.int64)
    else:
        rel = depth_relation(pairs[..., 3], pairs[..., 4], tau) * (-1 if invert else 1)
    im = np.arange(len(flat))[:, None]
    a, b = flat[im, pairs[..., 0].astype(np.int64)], flat[im, pairs[..., 1].astype(np.int64)]
    sign = (a > b).astype(np.int64) - (a < b)  # 0 for equal and for NaN
    counted = rel != 0
    return ((sign != rel) & counted).sum(1), counted.sum(1)


def _mirror(i, n):
    """scipy.ndimage 'mirror' on integer indices: d c b | a b c d | c b a."""
    if n == 1:
        return np.zeros_like(i)
    i = np.mod(i, 2 * n - 2)
    return np.where(i >= n, 2 * n - 2 - i, i)


def _blur_axis(x, axis, n_out):
    n_in = x.shape[axis]
    sigma = max(0.0, (n_in / n_out - 1) / 2)
    radius = int(4.0 * sigma + 0.5)
    if sigma <= 0 or radius == 0:
        return x
    d = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * d ** 2)
    phi /= phi.sum()
    out = np.zeros_like(x)
    for k, wgt in zip(d, phi):
        out += wgt * np.take(x, _mirror(np.arange(n_in) + k, n_in), axis=axis)
    return out


def _interp_axis(x, axis, n_out):
    n_in = x.shape[axis]
    s = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5
    if n_in == 1:
        s = np.zeros(n_out)
    else:
        top = n_in - 1
        s = np.mod(s, 2 * top)
        s = np.where(s > top, 2 * top - s, s)
    i0 = np.floor(s).astype(np.int64)
    f = s - i0
    shape = [1] * x.ndim
    shape[axis] = n_out
    f = f.reshape(shape)
    lo = np.take(x, i0, axis=axis)
    hi = np.take(x, _mirror(i0 + 1, n_in), axis=axis)
    return (1.0 - f) * lo + f * hi


def resize_antialias(x, oh, ow):
    """x [..., h, w, c] float32 -> [..., oh, ow, c] float64: the Gaussian correlation (mirror
    border) of every axis that shrinks, then linear interpolation at (dst + 0.5) in / out - 0.5."""
    y = np.asarray(x, np.float32).astype(np.float64)
    ay, ax = y.ndim - 3, y.ndim - 2
    y = _blur_axis(_blur_axis(y, ay, oh), ax, ow)
    return _interp_axis(_interp_axis(y, ay, oh), ax, ow)
