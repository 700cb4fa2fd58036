"""Pairwise ranking losses on the GPU, over the lists the samplers emit.

The loss the reference's method is defined against (Chen et al. 2016; Xian et al. 2018/2020),
which the reference itself only keeps the pieces of: ``--equality_threshold``, the vectorised
relation ``depth_utils.get_depth_relation_tf`` and the ``z0, z1`` columns of its pair tables
(generic_ranking_provider.py:108). Here it runs on exactly what the ListMLE losses take, so the
listwise-versus-pairwise ablation shares samples, batches, model and optimizer:

``HourglassPairwiseRankingLoss(ranking_size, batch_size)`` has ``HourglassNegativeLogLikelihood``'s
call signature (``loss(y_true[B,R,L,2], y_pred[B,H,W,1]) -> scalar``) and ``loss_and_grad``;
``PairwiseRankingLoss(ranking_size)`` is the per-list variant (labels and logits both [..., L]).
Per valid pair (i before j in list order; ``pair_mode`` ``"all"``: every i < j, ``"adjacent"``:
j = i + 1), with r = get_depth_relation(z_i, z_j, threshold) (negated by
``invert_relation_sign``) and d = t_i - t_j:

    r != 0:  softplus(-r d)          r == 0:  equal_weight d^2

averaged over the list's valid pairs; ``sample_weight`` and ``reduction`` mean what they mean for
the ListMLE losses (nll_loss.py). ``threshold=None`` is the plain comparison. One HIP call
(``pld_pairrank_fwd_bwd``) gives the value and d loss / d y_pred.

``pairs_to_lists`` turns a pair table of the evaluation providers into lists of two, so the loss
can be evaluated on it; the relation is recomputed from z0, z1 at the loss's threshold.
"""
import math

import numpy as np
import torch

from .. import kernels as K
from .nll_loss import _dev, _numel, _reduction, check_sample_weight

PAIR_MODES = ("all", "adjacent")


def pairs_to_lists(pairs):
    """A pair table [..., P, 5] of (point0, point1, relation, z0, z1) rows
    (generic_ranking_provider.py:91-109) as y_true [..., P, 2, 2]: one list of two per pair,
    (flat index, depth) per element. The stored relation column is dropped: the loss recomputes
    it from z0, z1 at its own threshold. NumPy in, NumPy out; a tensor stays a tensor."""
    if isinstance(pairs, torch.Tensor):
        if pairs.shape[-1] != 5:
            raise ValueError(f"pair table of shape {tuple(pairs.shape)}: the last axis must be 5")
        return torch.stack([pairs[..., [0, 3]], pairs[..., [1, 4]]], -2).to(torch.float32)
    p = np.asarray(pairs, np.float32)
    if p.ndim < 2 or p.shape[-1] != 5:
        raise ValueError(f"pair table of shape {p.shape}: the last axis must be 5")
    return np.ascontiguousarray(np.stack([p[..., [0, 3]], p[..., [1, 4]]], -2))


class _PairwiseRanking(object):
    """Argument handling shared by the two losses. ``kind`` tells compile() which training step
    to build; ``pair_args`` are that step's (and every call's) kernel arguments."""
    kind = "pairrank"

    def _init_pairs(self, ranking_size, threshold, pair_mode, equal_weight, invert_relation_sign,
                    reduction, extra):
        if "lambda_weight" in extra:
            raise ValueError("lambda_weight: rank discounts belong to the ListMLE losses "
                             "(nll_loss.py), not to a pairwise loss")
        if extra:
            raise TypeError(f"unexpected arguments {sorted(extra)}")
        self.ranking_size = int(ranking_size)
        if self.ranking_size < 2:
            raise ValueError(f"ranking_size {ranking_size}: a pair needs two elements")
        if pair_mode not in PAIR_MODES:
            raise ValueError(f"unknown pair_mode {pair_mode!r} (expected one of {PAIR_MODES})")
        if threshold is not None and not (math.isfinite(threshold) and threshold >= 0):
            raise ValueError(f"threshold {threshold!r}: expected a finite value >= 0, or None "
                             "for the plain comparison")
        if not (math.isfinite(equal_weight) and equal_weight >= 0):
            raise ValueError(f"equal_weight {equal_weight!r}: expected a finite value >= 0")
        self.threshold = None if threshold is None else float(threshold)
        self.pair_mode = pair_mode
        self.equal_weight = float(equal_weight)
        self.invert_relation_sign = bool(invert_relation_sign)
        self.reduction = _reduction(reduction)

    @property
    def pair_args(self):
        return dict(pair_mode=self.pair_mode, tau=self.threshold,
                    invert=self.invert_relation_sign, equal_weight=self.equal_weight)

    def _run(self, pred, y_true, B, R, L, sample_weight, dpred, per_list, loss):
        """(reduced loss or the [N] vector, dpred)."""
        list_w, per_image = None, False
        if sample_weight is not None:
            list_w, per_image = sample_weight
            list_w = _dev(list_w, pred.device)
        loss, dpred, per_list = K.pairrank_fwd_bwd(
            pred, y_true, B, R, L, list_w=list_w, list_w_per_image=per_image,
            reduction="mean" if self.reduction == "mean" else "sum", dpred=dpred,
            per_list=per_list, loss=loss, **self.pair_args)
        return (per_list if self.reduction == "none" else loss), dpred


class HourglassPairwiseRankingLoss(_PairwiseRanking):
    def __init__(self, ranking_size, batch_size, threshold=0.03, pair_mode="all",
                 equal_weight=1.0, invert_relation_sign=False, reduction="auto", name=None,
                 **extra):
        self._init_pairs(ranking_size, threshold, pair_mode, equal_weight, invert_relation_sign,
                         reduction, extra)
        self.batch_size = int(batch_size)
        self.name = name
        self._buf = {}

    def _buffers(self, pred, n_lists):
        key = (pred.shape, n_lists, pred.device)
        if key not in self._buf:
            self._buf[key] = (torch.empty_like(pred),
                              torch.empty(n_lists, device=pred.device),
                              torch.empty(1, device=pred.device))
        return self._buf[key]

    def loss_and_grad(self, y_true, y_pred, dpred=None, sample_weight=None):
        """(loss [1] device tensor, d loss / d y_pred with y_pred's shape). With
        ``reduction="none"`` the first value is the [N] vector s_n loss_n and the gradient is
        that of the vector's sum."""
        B, L = self.batch_size, self.ranking_size
        n_lists = _numel(y_true) // (2 * L)
        if n_lists % B:
            raise ValueError(f"y_true holds {n_lists} rankings, not a multiple of batch {B}")
        if sample_weight is not None:
            sample_weight = check_sample_weight(sample_weight, n_lists, B)
        y_pred = _dev(y_pred)
        y_true = _dev(y_true, y_pred.device)
        g, per_list, loss = self._buffers(y_pred, n_lists)
        if dpred is not None:
            g = dpred
        return self._run(y_pred, y_true, B, n_lists // B, L, sample_weight, g, per_list, loss)

    def __call__(self, y_true, y_pred, sample_weight=None):
        loss, _ = self.loss_and_grad(y_true, y_pred, sample_weight=sample_weight)
        return loss


class PairwiseRankingLoss(_PairwiseRanking):
    """Per-list pairwise ranking loss: y_true (depth labels) and y_pred (logits) both [..., L]."""

    def __init__(self, ranking_size, threshold=0.03, pair_mode="all", equal_weight=1.0,
                 invert_relation_sign=False, reduction="auto", name=None, **extra):
        self._init_pairs(ranking_size, threshold, pair_mode, equal_weight, invert_relation_sign,
                         reduction, extra)
        self.name = name

    def loss_and_grad(self, y_true, y_pred, sample_weight=None):
        """(loss, d loss / d y_pred); ``reduction="none"``: the [N] vector and the gradient of
        its sum. ``sample_weight``: a scalar or one weight per list."""
        L = self.ranking_size
        N = _numel(y_pred) // L
        if sample_weight is not None:
            sample_weight = check_sample_weight(sample_weight, N, N)
        y_pred = _dev(y_pred)
        labels = _dev(y_true, y_pred.device).reshape(-1, L)
        # each list is its own "image" of L pixels (index column = position)
        idx = torch.arange(L, device=y_pred.device, dtype=torch.float32).expand(N, L)
        yt = torch.stack([idx, labels], -1).contiguous()
        pred = y_pred.reshape(N, L).contiguous()
        loss, g = self._run(pred, yt, N, 1, L, sample_weight, None, None, None)
        return loss, g.reshape(y_pred.shape)

    def __call__(self, y_true, y_pred, sample_weight=None):
        return self.loss_and_grad(y_true, y_pred, sample_weight=sample_weight)[0]
