"""ListMLE lambda weights: what the reference's losses accept as ``lambda_weight`` and forward into
tensorflow_ranking's ``ListMLELoss`` (pldepth/losses/nll_loss.py:11-16, 33-40).

``ListMLELambdaWeight(rank_discount_fn)`` restates tfr 0.3.1's class of that name (third party,
not vendored; restated from its published source like oracle/listmle.py): position r = 1..L of the
sorted list gets the weight ``rank_discount_fn(float32(r))``, which turns ListMLE into
position-aware ListMLE (p-ListMLE, Lan et al. 2014). ``individual_weights(labels, ranks)`` keeps
tfr's contract in NumPy: ``ones_like(labels) * rank_discount_fn(ranks)``.

The loss classes take this class, or any object with a callable ``individual_weights(labels,
ranks)`` (a real tfr object where TensorFlow exists): ``resolve_rank_weights`` calls it once with
ones [1, L] and ranks [[1..L]] and keeps the float32 [L] vector the HIP kernel reads.
"""
import numpy as np


class ListMLELambdaWeight(object):
    """tfr ListMLELambdaWeight: per-position weights from a rank discount function."""

    def __init__(self, rank_discount_fn):
        if not callable(rank_discount_fn):
            raise TypeError("rank_discount_fn must be callable")
        self._rank_discount_fn = rank_discount_fn

    def pair_weights(self, labels, ranks):
        """tfr's ListMLELambdaWeight.pair_weights returns its labels unchanged."""
        return labels

    def individual_weights(self, labels, ranks):
        """``ones_like(labels) * rank_discount_fn(ranks)``; ranks are 1-based positions."""
        labels = np.asarray(labels, np.float32)
        ranks = np.asarray(ranks, np.float32)
        return np.ones_like(labels) * np.asarray(self._rank_discount_fn(ranks), np.float32)

    def rank_weights(self, L):
        """float32 [L]: the weights of ranks 1..L."""
        return resolve_rank_weights(self, L)


def log_discount(ranks):
    """1 / log2(1 + r): the nDCG discount."""
    return 1.0 / np.log2(1.0 + np.asarray(ranks, np.float64))


def pow2_discount(ranks):
    """2^(1 - r): p-ListMLE's 2^(L - r) - 1 normalised by its first term (for L large; the
    unnormalised form overflows float32 from L = 129). Evaluated in float64, then cast: the tail
    underflows to 0 past r = 150."""
    return np.exp2(1.0 - np.asarray(ranks, np.float64))


RANK_DISCOUNTS = {"log": log_discount, "pow2": pow2_discount}


def rank_discount_by_name(name, ranking_size=None):
    """The named discount function (``"log"``, ``"pow2"``). ``ranking_size`` is accepted for
    discounts that depend on the list length; neither of the two built in does."""
    try:
        return RANK_DISCOUNTS[name]
    except KeyError:
        raise ValueError(f"unknown rank discount {name!r} (expected one of "
                         f"{sorted(RANK_DISCOUNTS)})") from None


def lambda_weight_by_name(name, ranking_size=None):
    """``ListMLELambdaWeight`` of a named discount; ``None`` / ``"none"`` gives None (plain
    ListMLE). What the training CLI's ``--listmle_discount`` resolves through."""
    if name is None or name == "none":
        return None
    return ListMLELambdaWeight(rank_discount_by_name(name, ranking_size))


def resolve_rank_weights(lambda_weight, L):
    """float32 [L] rank weights of ``lambda_weight`` (None: None), from one call of its
    ``individual_weights(ones [1, L], ranks [[1..L]])``. Negative or non-finite weights, or a
    result of another size, raise ValueError."""
    if lambda_weight is None:
        return None
    fn = getattr(lambda_weight, "individual_weights", None)
    if not callable(fn):
        raise TypeError("lambda_weight must have a callable individual_weights(labels, ranks)")
    L = int(L)
    ones = np.ones((1, L), np.float32)
    ranks = np.arange(1, L + 1, dtype=np.float32)[None, :]
    w = np.asarray(fn(ones, ranks))
    if w.size != L:
        raise ValueError(f"individual_weights returned {w.size} weights for {L} ranks")
    w = np.ascontiguousarray(w.reshape(L), dtype=np.float32)
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("lambda weights must be finite and non-negative")
    return w
