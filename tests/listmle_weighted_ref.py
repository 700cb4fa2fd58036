"""float64 NumPy restatement of the position-weighted ListMLE loss — TEST INFRASTRUCTURE.

What pld_listmle_weighted_fwd_bwd computes, restated from tfr 0.3.1's ListMLELoss with a
ListMLELambdaWeight and Keras' compute_weighted_loss (parity with TF unpinned, as for
oracle/listmle.py, whose gather, validity rule, sort and tie order this follows step by step):

  valid = label >= 0; label' = valid ? label : 0; s' = valid ? s : log(1e-10)
  score = valid ? label' : min_j(label') - 1e-6; sort by score, descending (oracle.sort_order)
  t = sorted s'; m = max t; C_r = sum_{j>=r} exp(t_j - m)
  w_r = rank weight of rank r = 1..L (ListMLELambdaWeight.individual_weights)
  nll_n = sum_r w_r (log C_r - (t_r - m))
  d nll_n / d t_k = exp(t_k - m) sum_{r<=k} w_r / C_r - w_k; invalid elements: 0
  per list: s_n nll_n;  "mean": sum_n s_n nll_n / N (N lists);  "sum": sum_n s_n nll_n;
  "none": the [N] vector, with the gradient of its sum
  the gather's gradient scatter-adds into the dense [B, HW] map.
"""
import numpy as np

from oracle.listmle import LOG_EPS, sort_order


def listmle_weighted_fwd_bwd(s, labels, w=None):
    """Per-list weighted ListMLE. s, labels [N, L]; w [L] or None (ones).
    Returns (nll [N], d nll / d s [N, L]) in float64."""
    s = np.asarray(s, np.float64)
    lab = np.asarray(labels, np.float64)
    L = s.shape[1]
    w = np.ones(L) if w is None else np.asarray(w, np.float64).reshape(L)
    valid = lab >= 0
    lab0 = np.where(valid, lab, 0.0)
    sv = np.where(valid, s, LOG_EPS)
    score = np.where(valid, lab0, lab0.min(axis=1, keepdims=True) - 1e-6)
    order = sort_order(score)
    t = np.take_along_axis(sv, order, axis=1)
    m = t.max(axis=1, keepdims=True)
    e = np.exp(t - m)
    C = np.cumsum(e[:, ::-1], axis=1)[:, ::-1]
    nll = (w * (np.log(C) - (t - m))).sum(axis=1)
    g_sorted = e * np.cumsum(w / C, axis=1) - w
    g = np.empty_like(g_sorted)
    np.put_along_axis(g, order, g_sorted, axis=1)
    return nll, np.where(valid, g, 0.0)


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


def hourglass_weighted(y_true, y_pred, batch_size, ranking_size, w=None, sample_weight=None,
                       reduction="mean"):
    """(loss, d loss / d y_pred, s_n nll_n [N]) in float64. y_true [B, R, L, 2] (float32 flat
    index, label); y_pred [B, ...]. reduction "mean" | "sum" | "none" (loss is then the vector
    and the gradient that of its sum). Indices must lie in [0, HW)."""
    B, L = batch_size, ranking_size
    rk = np.asarray(y_true, np.float32).reshape(B, -1, L, 2)
    pred = np.asarray(y_pred, np.float64).reshape(B, -1)
    idx = rk[..., 0].reshape(B, -1).astype(np.int32)  # tf.cast(float32 -> int32) truncates
    s = np.take_along_axis(pred, idx, axis=1).reshape(-1, L)
    lab = rk[..., 1].reshape(-1, L)
    nll, g = listmle_weighted_fwd_bwd(s, lab, w)
    N = nll.shape[0]
    sw = list_weights(sample_weight, N, B)
    nll = sw * nll
    scale = sw / N if reduction == "mean" else sw
    loss = {"mean": nll.sum() / N, "sum": nll.sum(), "none": nll}[reduction]
    dpred = np.zeros_like(pred)
    gb = (g * scale[:, None]).reshape(B, -1)
    for b in range(B):
        np.add.at(dpred[b], idx[b], gb[b])
    return loss, dpred.reshape(np.shape(y_pred)), nll
