"""Position-weighted ListMLE, CPU side: the float64 yardstick (tests/listmle_weighted_ref.py)
against torch autograd, finite differences and the unweighted oracle; the lambda-weight classes;
the loss classes' argument handling; the C entry point's argument checks (nothing launches); the
training CLI's --listmle_discount helper."""
import ctypes as C

import numpy as np
import pytest
import torch

import listmle_weighted_ref as WR
from oracle import listmle as LM
from pldepth_amd import _lib
from pldepth_amd.losses import lambda_weights as LW


# ------------------------------------------------------------------ reference vs autograd / FD
def _case(rng, B, HW, R, L):
    pred = rng.standard_normal((B, HW))
    idx = rng.integers(0, HW, (B, R, L))
    lab = rng.permutation(B * R * L).reshape(B, R, L) / (B * R * L)
    if L > 2:
        lab[0, 0, 1] = -1.0  # one invalid element
    y = np.stack([idx.astype(np.float32), lab.astype(np.float32)], -1)
    return pred, y


def _torch_weighted(y, pred, B, L, w, sw, reduction):
    """The same loss written with torch ops only (float64, CPU); gradient by autograd."""
    p = torch.tensor(pred, dtype=torch.float64, requires_grad=True)
    rk = torch.tensor(y, dtype=torch.float64).reshape(B, -1, L, 2)
    idx = rk[..., 0].reshape(B, -1).long()
    s = torch.gather(p.reshape(B, -1), 1, idx).reshape(-1, L)
    lab = rk[..., 1].reshape(-1, L)
    valid = lab >= 0
    sv = torch.where(valid, s, torch.full_like(s, np.log(1e-10)))
    score = torch.where(valid, lab, lab.clamp(min=0).min(dim=1, keepdim=True).values - 1e-6)
    order = torch.argsort(score, dim=1, descending=True)  # tie-free labels
    t = torch.gather(sv, 1, order)
    m = t.max(dim=1, keepdim=True).values.detach()
    lce = torch.logcumsumexp((t - m).flip(1), dim=1).flip(1)
    nll = (torch.tensor(w) * (lce - (t - m))).sum(dim=1) * torch.tensor(sw)
    loss = nll.sum() / nll.numel() if reduction == "mean" else nll.sum()
    loss.backward()
    return loss.item(), p.grad.numpy(), nll.detach().numpy()


def _weights(rng, family, L):
    if family == "random":
        return rng.uniform(0.5, 2.0, L)
    if family == "zeros":
        w = rng.uniform(0.5, 2.0, L)
        w[::2] = 0.0
        return w
    return LW.ListMLELambdaWeight(LW.rank_discount_by_name(family, L)).rank_weights(
        L).astype(np.float64)


CASES = [(L, fam) for L in (1, 2, 7, 64) for fam in ("random", "zeros")] + [(200, "pow2")]


@pytest.mark.parametrize("L,family", CASES)
def test_reference_matches_autograd_and_finite_differences(L, family):
    rng = np.random.default_rng(100 * L + len(family))
    B, R, HW = 2, 3, 2 * L + 9
    pred, y = _case(rng, B, HW, R, L)
    w = _weights(rng, family, L)
    if family == "pow2":
        assert w[0] == 1.0 and w[149] > 0 and (w[150:] == 0).all()  # ranks past 150 underflow
    per_list = rng.uniform(0.0, 2.0, B * R)
    per_list[1] = 0.0
    per_image = np.array([0.0, 1.5])
    for sw in (None, per_list, per_image, per_list[:, None]):
        swn = WR.list_weights(sw, B * R, B)
        for reduction in ("mean", "sum"):
            loss, dpred, nll = WR.hourglass_weighted(y, pred, B, L, w, sw, reduction)
            loss_t, g_t, nll_t = _torch_weighted(y, pred, B, L, w, swn, reduction)
            np.testing.assert_allclose(loss, loss_t, rtol=1e-10, atol=1e-10)
            np.testing.assert_allclose(nll, nll_t, rtol=1e-10, atol=1e-10)
            np.testing.assert_allclose(dpred, g_t, rtol=1e-10, atol=1e-10)
            # "none": the vector, with the gradient of its sum
            vec, dvec, _ = WR.hourglass_weighted(y, pred, B, L, w, sw, "none")
            s_loss, s_d, _ = WR.hourglass_weighted(y, pred, B, L, w, sw, "sum")
            assert vec.shape == (B * R,) and np.array_equal(vec, nll)
            assert np.array_equal(dvec, s_d) and abs(vec.sum() - s_loss) <= 1e-12 * abs(s_loss)
    # central finite differences, step and bar of tests/test_oracle.py's gradient check
    eps = 1e-6
    idx = y[..., 0].astype(int)
    loss, dpred, _ = WR.hourglass_weighted(y, pred, B, L, w, per_list, "mean")
    for b, p in [(0, idx[0, 0, 0]), (1, idx[1, 2, L - 1]), (1, idx[1, 0, L // 2])]:
        pp = pred.copy()
        pp[b, p] += eps
        lp = WR.hourglass_weighted(y, pp, B, L, w, per_list, "mean")[0]
        pp[b, p] -= 2 * eps
        lm = WR.hourglass_weighted(y, pp, B, L, w, per_list, "mean")[0]
        assert abs((lp - lm) / (2 * eps) - dpred[b, p]) < 1e-7


@pytest.mark.parametrize("L", [1, 2, 7, 64])
def test_all_ones_reference_equals_the_oracle(L):
    rng = np.random.default_rng(L)
    B, R, HW = 2, 3, 2 * L + 9
    pred, y = _case(rng, B, HW, R, L)
    loss0, dpred0, nll0 = LM.hourglass_nll(y, pred, B, L, return_nll=True)
    for w, sw in ((None, None), (np.ones(L), np.ones(B * R)), (np.ones(L), 1.0)):
        loss, dpred, nll = WR.hourglass_weighted(y, pred, B, L, w, sw, "mean")
        np.testing.assert_allclose(loss, loss0, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(nll, nll0, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(dpred, dpred0, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------ lambda weights
def test_named_rank_weights_against_literals():
    log_w = LW.ListMLELambdaWeight(LW.rank_discount_by_name("log", 5)).rank_weights(5)
    pow_w = LW.ListMLELambdaWeight(LW.rank_discount_by_name("pow2", 5)).rank_weights(5)
    assert log_w.dtype == np.float32 and log_w.shape == (5,)
    # 1 / log2(1 + r), r = 1..5: 1, 1/log2(3), 1/2, 1/log2(5), 1/log2(6)
    np.testing.assert_allclose(log_w, [1.0, 0.6309297535714575, 0.5, 0.43067655807339306,
                                       0.38685280723454163], rtol=1e-7)
    assert np.array_equal(pow_w, np.array([1.0, 0.5, 0.25, 0.125, 0.0625], np.float32))
    # float64 then cast: finite at the L the hyper-parameter ranges reach, zero past r = 150
    big = LW.ListMLELambdaWeight(LW.rank_discount_by_name("pow2", 500)).rank_weights(500)
    assert np.isfinite(big).all() and big[0] == 1.0 and big[149] == 2.0 ** -149
    assert (big[150:] == 0).all()
    with pytest.raises(ValueError):
        LW.rank_discount_by_name("linear", 5)


def test_ranks_are_one_based_and_weights_broadcast_over_lists():
    seen = {}

    def fn(ranks):
        seen["ranks"] = np.array(ranks)
        return 10.0 * ranks

    lw = LW.ListMLELambdaWeight(fn)
    assert np.array_equal(lw.rank_weights(4), np.array([10, 20, 30, 40], np.float32))
    assert seen["ranks"].dtype == np.float32
    assert np.array_equal(seen["ranks"], [[1, 2, 3, 4]])
    # tfr's contract: ones_like(labels) * rank_discount_fn(ranks)
    labels = np.array([[3.0, 0.0, 7.0], [1.0, 1.0, 1.0]], np.float32)
    ranks = np.array([[1, 2, 3], [1, 2, 3]], np.float32)
    assert np.array_equal(lw.individual_weights(labels, ranks), 10.0 * ranks)


@pytest.mark.parametrize("bad", [-1.0, np.nan, np.inf])
def test_negative_and_non_finite_weights_are_rejected(bad):
    lw = LW.ListMLELambdaWeight(lambda r: np.where(r == 2, bad, 1.0))
    with pytest.raises(ValueError):
        lw.rank_weights(3)
    from pldepth_amd.losses.nll_loss import (HourglassNegativeLogLikelihood,
                                             NegativeLogLikelihoodLoss)
    with pytest.raises(ValueError):
        HourglassNegativeLogLikelihood(3, 2, lambda_weight=lw)
    with pytest.raises(ValueError):
        NegativeLogLikelihoodLoss(3, lambda_weight=lw)


def test_duck_typed_lambda_weight():
    """Any object with individual_weights(labels, ranks) serves (a real tfr object returns a
    tensor: whatever np.asarray converts)."""
    from pldepth_amd.losses.nll_loss import (HourglassNegativeLogLikelihood, MetaBatchListMLELoss,
                                             NegativeLogLikelihoodLoss)
    calls = []

    class Duck:
        def individual_weights(self, labels, ranks):
            calls.append((np.array(labels), np.array(ranks)))
            return (labels / ranks).tolist()  # [1, L] nested list

    loss = HourglassNegativeLogLikelihood(4, 2, lambda_weight=Duck())
    assert np.array_equal(loss.rank_weights, np.array([1, 1 / 2, 1 / 3, 1 / 4], np.float32))
    assert loss.rank_weights.dtype == np.float32 and loss.reduction == "mean"
    assert len(calls) == 1  # called once per loss object
    assert np.array_equal(calls[0][0], np.ones((1, 4))) and np.array_equal(calls[0][1],
                                                                            [[1, 2, 3, 4]])
    per_list = NegativeLogLikelihoodLoss(4, lambda_weight=Duck())
    assert np.array_equal(per_list.rank_weights, loss.rank_weights)
    assert MetaBatchListMLELoss is NegativeLogLikelihoodLoss
    assert HourglassNegativeLogLikelihood(4, 2).rank_weights is None
    with pytest.raises(TypeError):
        HourglassNegativeLogLikelihood(4, 2, lambda_weight=object())

    class Short:
        def individual_weights(self, labels, ranks):
            return np.ones(3)

    with pytest.raises(ValueError):
        HourglassNegativeLogLikelihood(4, 2, lambda_weight=Short())


# ----------------------------------------------------------------- loss classes, no GPU needed
def test_loss_classes_reject_an_unknown_reduction():
    from pldepth_amd.losses.nll_loss import (HourglassNegativeLogLikelihood,
                                             NegativeLogLikelihoodLoss)
    for red, want in (("auto", "mean"), ("sum_over_batch_size", "mean"), ("sum", "sum"),
                      ("none", "none")):
        assert HourglassNegativeLogLikelihood(3, 2, reduction=red).reduction == want
        assert NegativeLogLikelihoodLoss(3, reduction=red).reduction == want
    for red in ("average", "", None, 3):
        with pytest.raises(ValueError):
            HourglassNegativeLogLikelihood(3, 2, reduction=red)
        with pytest.raises(ValueError):
            NegativeLogLikelihoodLoss(3, reduction=red)


def test_loss_classes_reject_a_mis_sized_sample_weight():
    """The size check comes before anything is sent to the GPU."""
    from pldepth_amd.losses.nll_loss import (HourglassNegativeLogLikelihood,
                                             NegativeLogLikelihoodLoss, check_sample_weight)
    B, R, L = 2, 3, 4
    y = np.zeros((B, R, L, 2), np.float32)
    pred = np.zeros((B, 5, 5, 1), np.float32)
    loss = HourglassNegativeLogLikelihood(L, B)
    for bad in (np.ones(5), np.ones((B * R, 2)), np.ones((B, R)), np.ones((1, B * R)),
                np.ones(R)):
        with pytest.raises(ValueError):
            loss(y, pred, sample_weight=bad)
    with pytest.raises(ValueError):
        NegativeLogLikelihoodLoss(L)(np.zeros((7, L)), np.zeros((7, L)), sample_weight=np.ones(6))
    # accepted shapes: scalar, [N], [N,1], [B], [B,1]
    for sw, per_image in ((2.0, False), (np.ones(B * R), False), (np.ones((B * R, 1)), False),
                          (np.ones(B), True), (np.ones((B, 1)), True),
                          (torch.ones(B), True)):
        flat, pi = check_sample_weight(sw, B * R, B)
        assert pi == per_image and flat.shape == ((B,) if per_image else (B * R,))
    assert np.array_equal(check_sample_weight(2.0, B * R, B)[0], np.full(B * R, 2.0, np.float32))


def test_compile_refuses_none_and_a_data_parallel_sum():
    """Both refusals come before compile() touches the engine or a process group."""
    from types import SimpleNamespace

    from pldepth_amd.losses.nll_loss import HourglassNegativeLogLikelihood
    from pldepth_amd.models.pl_hourglass import FullyFledgedModel
    model = FullyFledgedModel(SimpleNamespace(B=2))
    with pytest.raises(ValueError, match="none"):
        model.compile(loss=HourglassNegativeLogLikelihood(3, 2, reduction="none"))
    with pytest.raises(ValueError, match="sum"):
        model.compile(loss=HourglassNegativeLogLikelihood(3, 2, reduction="sum"),
                      distribute=(0, 2, None))
    assert model.trainer is None


# -------------------------------------------------------------------- the C entry point's checks
def _weighted_call(**kw):
    """pld_listmle_weighted_fwd_bwd on fake (never dereferenced) addresses: every case here is
    refused before any launch."""
    p = C.c_void_p(1 << 20)  # 16-byte aligned
    a = dict(pred=p, y_true=p, B=1, HW=4, R=1, L=3, rank_w=None, list_w=None, per_image=0,
             reduction=_lib.CONST["PLD_REDUCE_MEAN"], nll=p, loss=p, dpred=p, zero_dpred=1)
    a.update(kw)
    with pytest.raises(_lib.PLDError) as e:
        _lib.lib().pld_listmle_weighted_fwd_bwd(
            a["pred"], a["y_true"], a["B"], a["HW"], a["R"], a["L"], a["rank_w"], a["list_w"],
            a["per_image"], a["reduction"], a["nll"], a["loss"], a["dpred"], a["zero_dpred"],
            None)
    return str(e.value)


def test_weighted_entry_point_rejects_bad_arguments_before_any_launch():
    assert _lib.CONST["PLD_REDUCE_MEAN"] == 0 and _lib.CONST["PLD_REDUCE_SUM"] == 1
    I32, P = C.c_int, C.c_void_p
    assert _lib._SIGS["pld_listmle_weighted_fwd_bwd"] == (
        I32, [P, P, I32, I32, I32, I32, P, P, I32, I32, P, P, P, I32, P])
    assert "pld_listmle_weighted_fwd_bwd" not in _lib._NON_STATUS
    for name in ("pred", "y_true", "nll", "loss", "dpred"):
        assert "null pointer" in _weighted_call(**{name: None}), name
    for L in (0, 513, -1):
        assert "L must be 1..512" in _weighted_call(L=L)
    for red in (2, -1, 7):
        assert "unknown reduction" in _weighted_call(reduction=red)
    assert "16-byte aligned" in _weighted_call(dpred=C.c_void_p((1 << 20) + 4))
    from pldepth_amd import kernels as K
    assert K.REDUCE == {"mean": 0, "sum": 1}


def test_header_cites_the_reference_for_the_weighted_loss():
    txt = open(_lib.HEADER).read()
    at = txt.index("Position-weighted ListMLE")
    block = txt[at:txt.index("pld_listmle_weighted_fwd_bwd(", at)]
    assert "nll_loss.py" in block and "ListMLELambdaWeight" in block


# ----------------------------------------------------------------------------------------- CLI
def test_cli_discount_resolves_to_the_weight_vector():
    from pldepth_amd import PLDepth
    opt = next(p for p in PLDepth.perform_pldepth_experiment.params
               if p.name == "listmle_discount")
    assert opt.default == "none" and list(opt.type.choices) == ["none", "log", "pow2"]
    plain = PLDepth.build_loss(5, 4, "none")
    assert plain.rank_weights is None and plain.lambda_weight is None
    assert plain.reduction == "mean" and (plain.ranking_size, plain.batch_size) == (5, 4)
    assert PLDepth.build_loss(5, 4).rank_weights is None
    r = np.arange(1, 6, dtype=np.float64)
    log = PLDepth.build_loss(5, 4, "log")
    assert np.array_equal(log.rank_weights, (1.0 / np.log2(1.0 + r)).astype(np.float32))
    pow2 = PLDepth.build_loss(5, 4, "pow2")
    assert np.array_equal(pow2.rank_weights, (2.0 ** (1.0 - r)).astype(np.float32))
    with pytest.raises(ValueError):
        PLDepth.build_loss(5, 4, "linear")
