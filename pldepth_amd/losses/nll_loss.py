"""Plackett-Luce (ListMLE) losses on the GPU (mirrors pldepth/losses/nll_loss.py).

``HourglassNegativeLogLikelihood(ranking_size, batch_size)`` keeps the reference's constructor and
call signature (``loss(y_true[B,R,L,2], y_pred[B,H,W,1]) -> scalar``, nll_loss.py:32-40); the
gather of predicted depths at the sampled pixels (depth_utils.py:39-61), tfr ListMLE and the
SUM_OVER_BATCH_SIZE reduction run as one HIP kernel that also produces d loss / d y_pred
(``loss_and_grad``), which the model's backward pass consumes. ``NegativeLogLikelihoodLoss`` is the
per-list variant (nll_loss.py:10-29: logits already [*, L]).

Both honour every argument the reference declares:
  * ``lambda_weight``: a ``lambda_weights.ListMLELambdaWeight`` (or any object with tfr's
    ``individual_weights(labels, ranks)``): position r of the sorted list weighs
    ``rank_discount_fn(r)`` (p-ListMLE);
  * ``sample_weight`` (Keras ``compute_weighted_loss``): a scalar, one weight per list ([N] or
    [N,1], N = B*R lists) or, as an extension Keras' broadcasting does not have, one per image
    ([B] or [B,1], applied to all R lists of the image); any other size is a ValueError;
  * ``reduction``: ``"auto"`` / ``"sum_over_batch_size"`` (sum_n s_n nll_n / N: the list count,
    not the weight sum), ``"sum"``, ``"none"`` (the [N] vector s_n nll_n).
With all three at their defaults the call is ``pld_listmle_fwd_bwd``, as before; otherwise
``pld_listmle_weighted_fwd_bwd``. The rank-weight vector is uploaded once per loss object.
"""
import numpy as np
import torch

from .. import kernels as K
from .lambda_weights import resolve_rank_weights

REDUCTIONS = {"auto": "mean", "sum_over_batch_size": "mean", "sum": "sum", "none": "none"}


def _dev(t, device="cuda"):
    if isinstance(t, torch.Tensor):
        return t.to(device=device, dtype=torch.float32).contiguous()
    return torch.as_tensor(np.ascontiguousarray(t, dtype=np.float32), device=device)


def _numel(t):
    return t.numel() if isinstance(t, torch.Tensor) else int(np.size(t))


def _reduction(reduction):
    key = getattr(reduction, "value", reduction)  # a Keras-style enum member or its string
    if not isinstance(key, str) or key.lower() not in REDUCTIONS:
        raise ValueError(f"unknown reduction {reduction!r} (expected one of "
                         f"{sorted(REDUCTIONS)})")
    return REDUCTIONS[key.lower()]


def check_sample_weight(sample_weight, n_lists, batch):
    """(float32 host array or device tensor, flat; per_image) of a sample_weight for n_lists
    lists in `batch` images: a scalar becomes one weight per list; a size matching neither the
    lists nor the images raises ValueError (before anything reaches the GPU)."""
    n = _numel(sample_weight)
    shape = tuple(sample_weight.shape) if hasattr(sample_weight, "shape") else np.shape(
        sample_weight)
    if len(shape) == 0:
        return np.full(n_lists, float(sample_weight), np.float32), False
    if len(shape) > 2 or (len(shape) == 2 and shape[1] != 1) or n not in (n_lists, batch):
        raise ValueError(f"sample_weight of shape {shape}: expected a scalar, one weight per "
                         f"list ([{n_lists}] or [{n_lists},1]) or one per image ([{batch}] or "
                         f"[{batch},1])")
    flat = sample_weight.reshape(-1) if isinstance(sample_weight, torch.Tensor) else \
        np.asarray(sample_weight, np.float32).reshape(-1)
    return flat, n != n_lists


class _WeightedListMLE(object):
    """lambda_weight / reduction handling shared by the two losses."""

    def _init_weights(self, reduction, lambda_weight):
        self.reduction = _reduction(reduction)
        self.lambda_weight = lambda_weight
        # float32 [L] host vector (None: plain ListMLE); compile() hands it to the trainer
        self.rank_weights = resolve_rank_weights(lambda_weight, self.ranking_size)
        self._rank_w_dev = {}

    def _rank_w(self, device):
        if self.rank_weights is None:
            return None
        if device not in self._rank_w_dev:
            self._rank_w_dev[device] = torch.from_numpy(self.rank_weights).to(device)
        return self._rank_w_dev[device]

    def _run(self, pred, y_true, B, R, L, sample_weight, dpred, nll, loss):
        """(reduced loss or the [N] vector, dpred) through the unweighted entry point when
        nothing is weighted, else the weighted one."""
        if self.rank_weights is None and sample_weight is None and self.reduction == "mean":
            loss, dpred, _ = K.listmle_fwd_bwd(pred, y_true, B, R, L, dpred=dpred, nll=nll,
                                               loss=loss)
            return loss, dpred
        list_w, per_image = None, False
        if sample_weight is not None:
            list_w, per_image = sample_weight
            list_w = _dev(list_w, pred.device)
        loss, dpred, nll = K.listmle_weighted_fwd_bwd(
            pred, y_true, B, R, L, rank_w=self._rank_w(pred.device), list_w=list_w,
            list_w_per_image=per_image, reduction="mean" if self.reduction == "mean" else "sum",
            dpred=dpred, nll=nll, loss=loss)
        return (nll if self.reduction == "none" else loss), dpred


class HourglassNegativeLogLikelihood(_WeightedListMLE):
    def __init__(self, ranking_size, batch_size, reduction="auto", name=None,
                 lambda_weight=None, debug=False):
        self.ranking_size = int(ranking_size)
        self.batch_size = int(batch_size)
        self.name = name
        self._buf = {}
        self._init_weights(reduction, lambda_weight)

    def _buffers(self, pred, n_lists):
        key = (pred.shape, n_lists, pred.device)
        if key not in self._buf:
            self._buf[key] = (torch.empty_like(pred),
                              torch.empty(n_lists, device=pred.device),
                              torch.empty(1, device=pred.device))
        return self._buf[key]

    def loss_and_grad(self, y_true, y_pred, dpred=None, sample_weight=None):
        """(loss [1] device tensor, d loss / d y_pred with y_pred's shape). With
        ``reduction="none"`` the first value is the [N] vector s_n nll_n and the gradient is
        that of the vector's sum."""
        B, L = self.batch_size, self.ranking_size
        n_lists = _numel(y_true) // (2 * L)
        if n_lists % B:
            raise ValueError(f"y_true holds {n_lists} rankings, not a multiple of batch {B}")
        if sample_weight is not None:
            sample_weight = check_sample_weight(sample_weight, n_lists, B)
        y_pred = _dev(y_pred)
        y_true = _dev(y_true, y_pred.device)
        R = n_lists // B
        g, nll, loss = self._buffers(y_pred, n_lists)
        if dpred is not None:
            g = dpred
        return self._run(y_pred, y_true, B, R, L, sample_weight, g, nll, loss)

    def __call__(self, y_true, y_pred, sample_weight=None):
        loss, _ = self.loss_and_grad(y_true, y_pred, sample_weight=sample_weight)
        return loss


class NegativeLogLikelihoodLoss(_WeightedListMLE):
    """Per-list ListMLE: y_true (labels) and y_pred (logits) both [..., L]."""

    def __init__(self, ranking_size, reduction="auto", name=None, lambda_weight=None):
        self.ranking_size = int(ranking_size)
        self.name = name
        self._init_weights(reduction, lambda_weight)

    def loss_and_grad(self, y_true, y_pred, sample_weight=None):
        """(loss, d loss / d y_pred); ``reduction="none"``: the [N] vector and the gradient of
        its sum. ``sample_weight``: a scalar or one weight per list."""
        L = self.ranking_size
        N = _numel(y_pred) // L
        if sample_weight is not None:
            sample_weight = check_sample_weight(sample_weight, N, N)
        y_pred = _dev(y_pred)
        labels = _dev(y_true, y_pred.device).reshape(-1, L)
        # each list is its own "image" of L pixels, ranked in place (index column = position)
        idx = torch.arange(L, device=y_pred.device, dtype=torch.float32).expand(N, L)
        yt = torch.stack([idx, labels], -1).contiguous()
        pred = y_pred.reshape(N, L).contiguous()
        loss, g = self._run(pred, yt, N, 1, L, sample_weight, None, None, None)
        return loss, g.reshape(y_pred.shape)

    def __call__(self, y_true, y_pred, sample_weight=None):
        return self.loss_and_grad(y_true, y_pred, sample_weight=sample_weight)[0]


MetaBatchListMLELoss = NegativeLogLikelihoodLoss
