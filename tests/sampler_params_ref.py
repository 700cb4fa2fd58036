"""NumPy restatement of the ranking samplers with every argument of the reference's classes as a
parameter — TEST INFRASTRUCTURE, the parametrised sibling of oracle/sampler.py.

Beyond oracle/sampler.py (which fixes tau = 0.03, penalty = -1000, the default factors and a mask
at the image's resolution):

  * ``tau``      ``threshold`` of get_depth_relation (pldepth/data/depth_utils.py:14-21): the
                 float32 ratio is compared with float32(1 + tau) and float32(1 / (1 + tau)), the
                 Python floats NumPy (NEP 50) casts to the ratio's type;
  * ``penalty``  ``equality_penalty``: Thresholded adds it to a float32 accumulator
                 (sampling.py:199-205: ``0 + penalty`` is a Python number until the first float32
                 gap is added, which casts it: the same value as float32(0) + float32(penalty)),
                 Info adds it to the float64 ``score_Id[i]`` (sampling.py:233-237);
  * ``factor``   ``batch_size_factor``: n_cand = int(R * factor) (sampling.py:55); every strategy
                 returns ``[:R]`` of what it has, so min(n_cand, R) lists;
  * mask grid    a mask of another resolution: a drawn mask position (mr, mc) is the pixel
                 (int(mr * (H / mask_h)), int(mc * (W / mask_w))) (sampling.py:115-116,125-129);
                 the Info strategy's expected list stays that of the whole gt;
  * ``random``   RandomSamplingStrategy.sample_points_batch (sampling.py:89-103): a draw is a
                 pixel (row, col), lists keep their draw order, the score is the float64
                 sequential sum of adjacent gaps of the depths sorted descending (:34-42).

Same float types and the same tie rule as oracle/sampler.py: stable ascending argsort, reversed.
An empty mask gives the HIP sampler's defined all-invalid lists (index 0, depth -1).
"""
import numpy as np

from oracle.sampler import (canonical_lists, info_expected_list, pairwise_sum32,  # noqa: F401
                            _sorted_desc_order)

DEFAULT_FACTORS = {"pure": 0.8, "masked": 1.5, "thresh": 1.5, "info": 5, "random": 1.5}
_EPS32 = np.float32(1e-10)


# ---- golden/sampler_params_golden.npz (golden/make_sampler_params_golden.py) ----
GOLDEN_STRATEGIES = ("thresh", "info", "pure", "random")  # the generator's run order
GOLDEN_CASES = 4


def load_case(g, ci):
    """(gt [H,W] float32, mask [mask_h,mask_w] float32, L, R, tau, penalty, factor) of case ci."""
    h, w, mh, mw, L, R = [int(v) for v in g["cases"][ci][:6]]
    tau, pen, factor = [float(v) for v in g["cases"][ci][6:]]
    gt = g[f"c{ci}_codes"].astype(np.float32) / np.float32(255)
    assert gt.shape == (h, w)
    mask = np.unpackbits(g[f"c{ci}_mask"])[: mh * mw].reshape(mh, mw).astype(np.float32)
    return gt, mask, L, R, tau, pen, factor


def case_draws(g, ci, strategy, w):
    """The recorded randint sequence as the restatement and the rank kernels take it: positions
    in np.where(mask > 0), or flat pixels from the unmasked sampler's (row, col) pairs."""
    d = g[f"c{ci}_{strategy}_draws"].astype(np.int64)
    return d[0::2] * w + d[1::2] if strategy == "random" else d


class Params:
    """A model_params stand-in: get_parameter over keyword arguments."""

    def __init__(self, **kw):
        self.p = kw

    def get_parameter(self, name, default=None):
        return self.p.get(name, default)


def n_candidates(R, factor):
    """``int(batch_size * batch_size_factor)`` — sampling.py:55."""
    return int(R * factor)


def depth_relation32(d1, d2, tau):
    d1 = np.asarray(d1, np.float32)
    d2 = np.asarray(d2, np.float32)
    hi = np.float32(1 + tau)
    lo = np.float32(1 / (1 + tau))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (d1 + _EPS32) / (d2 + _EPS32)
    return np.where(r >= hi, 1, np.where(r <= lo, -1, 0)).astype(np.int8)


def sample_candidates(mask, gt, n_cand, L, draws):
    """n_cand lists of L masked pixels, sorted by gt descending; draws index np.where(mask > 0)
    of the MASK grid. float32 [n_cand, L, 2] (flat image index row*W+col, gt)."""
    H, W = gt.shape
    xs, ys = H / mask.shape[0], W / mask.shape[1]  # determine_x_y_scales
    rows, cols = np.where(mask > 0)
    nvalid = rows.shape[0]
    out = np.empty((n_cand, L, 2), np.float32)
    if nvalid == 0:
        out[:, :, 0], out[:, :, 1] = 0, -1
        return out
    draws = np.asarray(draws, np.int64).reshape(n_cand, L)
    if draws.size and (draws.min() < 0 or draws.max() >= nvalid):
        raise ValueError("draw out of range")
    r = (rows[draws] * xs).astype(np.int64)  # int(np.int64 * float): truncation
    c = (cols[draws] * ys).astype(np.int64)
    idx = (r * W + c).astype(np.float64)
    g = gt[r, c].astype(np.float64)
    order = _sorted_desc_order(g)
    out[:, :, 0] = np.take_along_axis(idx, order, axis=1)
    out[:, :, 1] = np.take_along_axis(g, order, axis=1)
    return out


def score_candidates(cands, strategy, gt, tau, penalty):
    n_cand, L, _ = cands.shape
    g = cands[:, :, 1]
    scores = np.zeros(n_cand, np.float64)
    if strategy == "pure":
        return scores
    if strategy == "random":
        d = np.sort(g.astype(np.float64), axis=1)[:, ::-1]
        for j in range(L - 1):
            scores = scores + np.abs(d[:, j] - d[:, j + 1])
        return scores
    eq = depth_relation32(g[:, :-1], g[:, 1:], tau) == 0
    if strategy in ("masked", "thresh"):
        diff = np.abs(g[:, :-1] - g[:, 1:])  # float32
        acc = np.zeros(n_cand, np.float32)
        for j in range(L - 1):  # penalty first, then the difference
            if strategy == "thresh":
                acc = np.where(eq[:, j], (acc + np.float32(penalty)).astype(np.float32), acc)
            acc = (acc + diff[:, j]).astype(np.float32)
        scores[:] = acc
        return scores
    if strategy == "info":
        e = info_expected_list(gt, L)
        terms = (np.square(g - e) / e).astype(np.float32)
        for i in range(n_cand):
            scores[i] = -pairwise_sum32(terms[i])
        for j in range(L - 1):  # float64 accumulation
            scores = np.where(eq[:, j], scores + float(penalty), scores)
        return scores
    raise ValueError(strategy)


def sample_point_batch(strategy, mask, gt, R, L, draws, tau=0.03, penalty=-1000, factor=None):
    """``<Strategy>(params, tau, penalty).sample_masked_point_batch(image, mask, gt, R, factor)``
    or, for ``strategy == "random"`` (mask ignored; draws are flat pixels row*W+col),
    ``RandomSamplingStrategy.sample_points_batch(image, gt, R, factor)`` -> float32 [R', L, 2]."""
    factor = DEFAULT_FACTORS[strategy] if factor is None else factor
    n_cand = n_candidates(R, factor)
    if strategy == "random":
        H, W = gt.shape
        d = np.asarray(draws, np.int64).reshape(n_cand, L)
        if d.size and (d.min() < 0 or d.max() >= H * W):
            raise ValueError("draw out of range")
        cands = np.empty((n_cand, L, 2), np.float32)
        cands[:, :, 0] = d
        cands[:, :, 1] = gt[d // W, d % W]
    else:
        cands = sample_candidates(mask, gt, n_cand, L, draws)
    if strategy == "pure":
        return cands[:R]
    scores = score_candidates(cands, strategy, gt, tau, penalty)
    order = np.argsort(scores, kind="stable")[::-1][:R]
    return cands[order]
