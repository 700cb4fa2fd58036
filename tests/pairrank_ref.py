"""float64 NumPy restatement of the pairwise ranking loss — TEST INFRASTRUCTURE.

What pld_pairrank_fwd_bwd computes. y_true [B, R, L, 2] (float32 flat index, depth), pred
[B, HW]; t_i = pred[b, idx_i]. Pairs in list order: "all" = every i < j, "adjacent" = (i, i+1). A
pair is valid when both depths are >= 0 (pld_listmle_fwd_bwd's rule for an element).

  r = relation(z_i, z_j): tau >= 0: get_depth_relation (pldepth/data/depth_utils.py:5-21) as it
      evaluates on np.float32 scalars: the ratio (z_i + 1e-10) / (z_j + 1e-10) in float32,
      compared with float32(1 + tau) and float32(1 / (1 + tau)), so a ratio on a threshold falls
      the way the kernel's does; tau None (or < 0): the plain comparison; invert: r = -r
  d = t_i - t_j (float64 from here on)
  r != 0: l = max(-r d, 0) + log1p(exp(-|d|)),  dl/dt_i = -r sigmoid(-r d) = -dl/dt_j
  r == 0: l = equal_weight d^2,                 dl/dt_i = 2 equal_weight d  = -dl/dt_j
  loss_n = sum l / n_n over the n_n valid pairs (0 pairs: 0, and 0 gradient)
  per_list[n] = s_n loss_n;  "mean": sum_n s_n loss_n / N (N lists);  "sum": the plain sum;
  "none": the [N] vector, with the gradient of its sum
  the gather's gradient scatter-adds into the dense [B, HW] map.
"""
import numpy as np


def list_weights(sample_weight, n_lists, batch):
    """[N] float64 per-list weights of a sample_weight (None, scalar, per list or per image)."""
    if sample_weight is None:
        return np.ones(n_lists)
    sw = np.asarray(sample_weight, np.float64)
    if sw.ndim == 0:
        return np.full(n_lists, float(sw))
    sw = sw.reshape(-1)
    if sw.size == n_lists:
        return sw
    assert sw.size == batch, (sw.size, n_lists, batch)
    return np.repeat(sw, n_lists // batch)


def relation32(zi, zj, tau=0.03, invert=False):
    """int64 relations of float32 depth arrays, element by element."""
    zi, zj = np.asarray(zi, np.float32), np.asarray(zj, np.float32)
    if tau is None or tau < 0:
        r = (zi > zj).astype(np.int64) - (zi < zj).astype(np.int64)
    else:
        eps = np.float32(1e-10)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = (zi + eps) / (zj + eps)
        assert ratio.dtype == np.float32
        hi, lo = np.float32(1.0 + tau), np.float32(1.0 / (1.0 + tau))
        r = np.where(ratio >= hi, 1, np.where(ratio <= lo, -1, 0)).astype(np.int64)
    return -r if invert else r


def pair_indices(L, pair_mode):
    if pair_mode == "all":
        return np.triu_indices(L, 1)
    if pair_mode == "adjacent":
        return np.arange(L - 1), np.arange(1, L)
    raise ValueError(pair_mode)


def pairrank_lists(t, z, pair_mode="all", tau=0.03, invert=False, equal_weight=1.0):
    """Per-list loss. t [N, L] logits, z [N, L] float32 depths.
    Returns (loss_n [N], d loss_n / d t [N, L], counts (n_minus, n_equal, n_plus)) in float64."""
    t = np.asarray(t, np.float64)
    z = np.asarray(z, np.float32)
    N, L = t.shape
    i, j = pair_indices(L, pair_mode)
    valid = (z[:, i] >= 0) & (z[:, j] >= 0)
    r = relation32(z[:, i], z[:, j], tau, invert)
    d = t[:, i] - t[:, j]
    e = np.exp(-np.abs(d))
    x = -r * d
    sig = np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    l = np.where(r != 0, np.maximum(x, 0.0) + np.log1p(e), equal_weight * d * d)
    gi = np.where(r != 0, -r * sig, 2.0 * equal_weight * d)
    l = np.where(valid, l, 0.0)
    gi = np.where(valid, gi, 0.0)
    n = valid.sum(axis=1)
    inv = np.where(n > 0, 1.0 / np.maximum(n, 1), 0.0)
    loss = l.sum(axis=1) * inv
    g = np.zeros((N, L))
    for k in range(N):
        g[k] = (np.bincount(i, weights=gi[k], minlength=L)
                - np.bincount(j, weights=gi[k], minlength=L)) * inv[k]
    counts = tuple(int(((r == s) & valid).sum()) for s in (-1, 0, 1))
    return loss, g, counts


def hourglass_pairrank(y_true, y_pred, batch_size, ranking_size, pair_mode="all", tau=0.03,
                       invert=False, equal_weight=1.0, sample_weight=None, reduction="mean"):
    """(loss, d loss / d y_pred, s_n loss_n [N], counts) in float64. reduction "mean" | "sum" |
    "none" (loss is then the vector and the gradient that of its sum). Indices must lie in
    [0, HW)."""
    B, L = batch_size, ranking_size
    rk = np.asarray(y_true, np.float32).reshape(B, -1, L, 2)
    pred = np.asarray(y_pred, np.float64).reshape(B, -1)
    idx = rk[..., 0].reshape(B, -1).astype(np.int32)  # tf.cast(float32 -> int32) truncates
    t = np.take_along_axis(pred, idx, axis=1).reshape(-1, L)
    z = rk[..., 1].reshape(-1, L)
    loss_n, g, counts = pairrank_lists(t, z, pair_mode, tau, invert, equal_weight)
    N = loss_n.shape[0]
    sw = list_weights(sample_weight, N, B)
    per_list = sw * loss_n
    scale = sw / N if reduction == "mean" else sw
    loss = {"mean": per_list.sum() / N, "sum": per_list.sum(), "none": per_list}[reduction]
    dpred = np.zeros_like(pred)
    gb = (g * scale[:, None]).reshape(B, -1)
    for b in range(B):
        np.add.at(dpred[b], idx[b], gb[b])
    return loss, dpred.reshape(np.shape(y_pred)), per_list, counts
