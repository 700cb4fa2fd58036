"""pld_listmle_weighted_fwd_bwd (position-weighted ListMLE, sample weights, reductions) on the
GPU against the float64 restatement tests/listmle_weighted_ref.py, from the kernel up to
train_on_batch / evaluate.

TOLERANCE. tests/test_step_kernels_gpu.py's measure err(got, ref) = max|got - ref| / max|ref| and
its bound 1e-5, on loss, per-list nll and dpred. Exact-zero claims (pixels no valid element
names, invalid elements, lists of sample weight 0) are asserted as exact zeros. Every call gets
dpred, nll and loss pre-filled with NaN. Each comparison prints its figures before it asserts.
"""
import numpy as np
import pytest
import torch

import listmle_weighted_ref as WR
from oracle import listmle as LM
from pldepth_amd import kernels as K
from pldepth_amd.losses.lambda_weights import ListMLELambdaWeight, lambda_weight_by_name
from pldepth_amd.losses.nll_loss import HourglassNegativeLogLikelihood, NegativeLogLikelihoodLoss

pytestmark = pytest.mark.gpu

BAR = 1e-5
HW0 = 11 * 13
FAMILIES = ("ones", "log", "pow2", "random", "zeros3")


def err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _lists(rng, B, HW, R, L, spread=1.0, unique=False):
    """Random pixels (unique per image on request), tie-free labels in no particular order, as
    tests/test_step_kernels_gpu.py::_lists."""
    pred = (rng.standard_normal((B, HW)) * spread).astype(np.float32)
    if unique:
        idx = np.stack([rng.permutation(HW)[:R * L] for _ in range(B)]).reshape(B, R, L)
    else:
        idx = rng.integers(0, HW, (B, R, L))
    lab = (rng.permutation(B * R * L).reshape(B, R, L) / (B * R * L)).astype(np.float32)
    y = np.ascontiguousarray(np.stack([idx.astype(np.float32), lab], -1).astype(np.float32))
    return pred, y


def rank_weights(rng, family, L):
    """float32 [L], or None for the entry point's NULL (all ones)."""
    if family == "ones":
        return None
    if family in ("log", "pow2"):
        return lambda_weight_by_name(family, L).rank_weights(L)
    w = rng.uniform(0.5, 2.0, L).astype(np.float32)
    if family == "zeros3":
        w[:3] = 0.0
    return w


def _weighted(cuda, pred, y, w=None, sw=None, per_image=False, reduction="mean",
              zero_dpred=True, prior=None):
    B, R, L = y.shape[:3]
    tp = dev(pred, cuda)
    dpred = torch.full_like(tp, float("nan")) if prior is None else dev(prior, cuda)
    nll = torch.full((B * R,), float("nan"), device=cuda)
    loss = torch.full((1,), float("nan"), device=cuda)
    out = K.listmle_weighted_fwd_bwd(
        tp, dev(y, cuda), B, R, L, rank_w=None if w is None else dev(w, cuda),
        list_w=None if sw is None else dev(np.asarray(sw, np.float32), cuda),
        list_w_per_image=per_image, reduction=reduction, dpred=dpred, nll=nll, loss=loss,
        zero_dpred=zero_dpred)
    torch.cuda.synchronize()
    assert out[0] is loss and out[1] is dpred and out[2] is nll
    return loss.item(), dpred.cpu().numpy(), nll.cpu().numpy()


def _named(y, HW):
    """[B, HW] mask of the pixels that some valid element names (indices here are in range)."""
    B = y.shape[0]
    named = np.zeros((B, HW), bool)
    for b in range(B):
        ok = y[b, ..., 1].reshape(-1) >= 0
        named[b, y[b, ..., 0].reshape(-1)[ok].astype(np.int64)] = True
    return named


def _check(cuda, pred, y, w=None, sw=None, reduction="mean", tag=""):
    B, R, L = y.shape[:3]
    per_image = sw is not None and np.size(sw) == B and B != B * R
    loss_ref, dpred_ref, nll_ref = WR.hourglass_weighted(y, pred, B, L, w, sw, reduction)
    loss, dpred, nll = _weighted(cuda, pred, y, w, sw, per_image, reduction)
    assert np.isfinite(dpred).all() and np.isfinite(nll).all() and np.isfinite(loss)
    e = (err(loss, loss_ref), err(nll, nll_ref), err(dpred, dpred_ref))
    print("listmle_w %s B=%d R=%d L=%d %s  err loss %.3g nll %.3g dpred %.3g" % (
        tag, B, R, L, reduction, *e))
    assert max(e) < BAR, (tag, e)
    named = _named(y, pred.shape[1])
    assert np.array_equal(dpred[~named], np.zeros(int((~named).sum()), np.float32))
    return loss, dpred, nll


def instance_cases(L):
    """(tag, pred, y, w) of test_every_instance_and_edge at list length L."""
    rng = np.random.default_rng(2000 + L)
    for B, R in ((1, 1), (3, 1), (1, 5)):
        for spread in (1.0, 5.0):
            for family in FAMILIES:
                pred, y = _lists(rng, B, HW0, R, L, spread)
                yield "%s x%g" % (family, spread), pred, y, rank_weights(rng, family, L)


@pytest.mark.parametrize("L", [1, 2, 64, 65, 128, 129, 256, 257, 512])
def test_every_instance_and_edge(cuda, L):
    """L <= 64, 128, 256, 512 select weighted_kernel<1, 2, 4, 8>; 1, 3, 5 lists leave 3, 1, 3
    inactive waves in the last block; logits at spread 1 and 5; every weight family ("pow2" is
    zero past rank 150, "zeros3" on the first three ranks)."""
    for tag, pred, y, w in instance_cases(L):
        _check(cuda, pred, y, w, tag=tag)


@pytest.mark.parametrize("L", [40, 200])
@pytest.mark.parametrize("pattern", ["front", "last_third", "whole_list"])
def test_invalid_labels_with_weights(cuda, L, pattern):
    """Label -1: the element stays in the list at logit log(1e-10), sorts last, takes the rank
    weight of its sorted position and gets exactly 0.0 gradient. Every pixel is named once."""
    rng = np.random.default_rng(10 * L + len(pattern))
    B, R = 2, 3
    HW = R * L + 7
    for spread in (1.0, 5.0):
        for family in ("log", "pow2", "random"):
            pred, y = _lists(rng, B, HW, R, L, spread, unique=True)
            if pattern == "front":
                y[:, :, 0, 1] = -1.0
            elif pattern == "last_third":
                y[:, :, L - L // 3:, 1] = -1.0
            else:
                y[0, 1, :, 1] = -1.0
                y[1, 2, :, 1] = -1.0
            w = rank_weights(rng, family, L)
            _, dpred, nll = _check(cuda, pred, y, w, tag="%s %s x%g" % (pattern, family, spread))
            for b in range(B):
                bad = y[b, ..., 0][y[b, ..., 1] < 0].astype(np.int64)
                assert bad.size and np.array_equal(dpred[b, bad], np.zeros(bad.size, np.float32))
            if pattern == "whole_list":  # every logit equal: nll = sum_r w_r log(L - r + 1)
                want = float(np.sum(w.astype(np.float64) * np.log(np.arange(L, 0, -1))))
                assert abs(nll[1] - want) < BAR * want and abs(nll[R + 2] - want) < BAR * want


@pytest.mark.parametrize("B,R", [(2, 3), (3, 1)])
@pytest.mark.parametrize("mode", ["per_list", "per_image"])
def test_sample_weights(cuda, B, R, mode):
    rng = np.random.default_rng(7 * B + R + len(mode))
    L = 70
    HW = R * L + 9
    pred, y = _lists(rng, B, HW, R, L, unique=True)
    w = rank_weights(rng, "log", L)
    n = B * R if mode == "per_list" else B
    sw = rng.uniform(0.25, 3.0, n).astype(np.float32)
    sw[n - 1] = 0.0
    for reduction in ("mean", "sum"):
        _, dpred, nll = _check(cuda, pred, y, w, sw, reduction, tag=mode)
        # the lists of weight 0: nll exactly 0.0, and exactly 0.0 on the pixels only they name
        # (pixels are unique per image, so those are all of their pixels)
        lists = [B * R - 1] if mode == "per_list" else list(range((B - 1) * R, B * R))
        for ln in lists:
            b, r = divmod(ln, R)
            assert nll[ln] == 0.0
            own = y[b, r, :, 0].astype(np.int64)
            assert np.array_equal(dpred[b, own], np.zeros(L, np.float32))
        assert (dpred != 0).any() and (nll[:1] != 0).all()


def test_scalar_weight_of_two_doubles_bit_for_bit(cuda):
    """Scaling by a power of two is exact: loss, nll and dpred of sample_weight=2 are twice the
    weight-1 run's, bit for bit (unique pixels: the order of the atomics plays no part)."""
    rng = np.random.default_rng(5)
    B, R, L, H = 2, 3, 70, 16
    pred, y = _lists(rng, B, H * H, R, L, unique=True)
    loss_fn = HourglassNegativeLogLikelihood(L, B, lambda_weight=lambda_weight_by_name("log"))
    p4 = pred.reshape(B, H, H, 1)
    one, g1 = loss_fn.loss_and_grad(y, p4, dpred=torch.full((B, H, H, 1), float("nan"),
                                                           device=cuda))
    one, g1 = one.clone(), g1.clone()
    two, g2 = loss_fn.loss_and_grad(y, p4, sample_weight=2.0,
                                    dpred=torch.full((B, H, H, 1), float("nan"), device=cuda))
    torch.cuda.synchronize()
    assert one.item() > 0 and two.item() == 2.0 * one.item()
    assert torch.equal(g2, 2.0 * g1) and (g1 != 0).any()
    ref = WR.hourglass_weighted(y, pred, B, L, loss_fn.rank_weights, 2.0, "mean")
    assert err(two.item(), ref[0]) < BAR and err(g2.cpu().numpy().reshape(B, -1), ref[1]) < BAR


def test_reductions(cuda):
    rng = np.random.default_rng(11)
    B, R, L = 2, 3, 130
    pred, y = _lists(rng, B, HW0, R, L)
    w = rank_weights(rng, "random", L)
    sw = rng.uniform(0.5, 2.0, B * R).astype(np.float32)
    mean, d_mean, nll_mean = _check(cuda, pred, y, w, sw, "mean")
    total, d_sum, nll_sum = _check(cuda, pred, y, w, sw, "sum")
    N = B * R
    print("sum vs N x mean: loss %.3g dpred %.3g" % (err(total, N * mean),
                                                    err(d_sum, N * d_mean)))
    assert err(total, N * mean) < BAR and err(d_sum, N * d_mean) < BAR
    assert np.array_equal(nll_sum, nll_mean)
    # "none" through the loss classes: the [N] vector s_n nll_n, the gradient of its sum
    lw = ListMLELambdaWeight(lambda r: w[np.asarray(r, np.int64) - 1])
    H = (11, 13)
    vec, g = HourglassNegativeLogLikelihood(L, B, reduction="none", lambda_weight=lw) \
        .loss_and_grad(y, pred.reshape(B, *H, 1), sample_weight=sw)
    torch.cuda.synchronize()
    ref_vec, ref_d, _ = WR.hourglass_weighted(y, pred, B, L, w, sw, "none")
    assert tuple(vec.shape) == (N,) and tuple(g.shape) == (B, *H, 1)
    assert err(vec.cpu().numpy(), ref_vec) < BAR
    assert err(g.cpu().numpy().reshape(B, -1), ref_d) < BAR
    s = rng.standard_normal((N, L)).astype(np.float32)
    vec2 = NegativeLogLikelihoodLoss(L, reduction="none", lambda_weight=lw)(y[..., 1], s)
    torch.cuda.synchronize()
    ref2, _ = WR.listmle_weighted_fwd_bwd(s, y[..., 1].reshape(N, L), w)
    assert tuple(vec2.shape) == (N,) and err(vec2.cpu().numpy(), ref2) < BAR


@pytest.mark.parametrize("L", [5, 64, 100, 200, 400])
def test_all_ones_against_the_unweighted_entry_point(cuda, L):
    """Same inputs, unique pixels per image (the order of the atomics cannot matter): within the
    bar of pld_listmle_fwd_bwd; whether the two were bit-identical is printed."""
    rng = np.random.default_rng(L)
    B, R = 2, 3
    HW = R * L + 5
    for spread in (1.0, 5.0):
        pred, y = _lists(rng, B, HW, R, L, spread, unique=True)
        tp, ty = dev(pred, cuda), dev(y, cuda)
        loss0, dpred0, nll0 = K.listmle_fwd_bwd(tp, ty, B, R, L)
        torch.cuda.synchronize()
        loss0, dpred0, nll0 = loss0.item(), dpred0.cpu().numpy(), nll0.cpu().numpy()
        for w, sw in ((None, None), (np.ones(L, np.float32), np.ones(B * R, np.float32))):
            loss, dpred, nll = _weighted(cuda, pred, y, w, sw)
            same = loss == loss0 and np.array_equal(dpred, dpred0) and np.array_equal(nll, nll0)
            e = (err(loss, loss0), err(nll, nll0), err(dpred, dpred0))
            print("all-ones L=%d x%g %s: bit-identical %s, err loss %.3g nll %.3g dpred %.3g" % (
                L, spread, "NULL" if w is None else "ones", same, *e))
            assert max(e) < BAR, e


@pytest.mark.parametrize("B,HW", [(1, 3), (5, 29), (2, 75)])
def test_accumulates_without_zero_dpred(cuda, B, HW):
    rng = np.random.default_rng(B * HW + 2)
    R, L = (1, 2) if HW == 3 else (2, 5)
    pred, y = _lists(rng, B, HW, R, L)
    w = rank_weights(rng, "random", L)
    sw = rng.uniform(0.5, 2.0, B * R).astype(np.float32)
    prior = (0.25 * rng.standard_normal((B, HW))).astype(np.float32)
    loss_ref, dpred_ref, _ = WR.hourglass_weighted(y, pred, B, L, w, sw, "sum")
    loss, dpred, _ = _weighted(cuda, pred, y, w, sw, reduction="sum", zero_dpred=False,
                               prior=prior)
    assert err(loss, loss_ref) < BAR
    assert err(dpred, prior.astype(np.float64) + dpred_ref) < BAR
    untouched = ~_named(y, HW)
    assert untouched.any() and np.array_equal(dpred[untouched], prior[untouched])


def test_loss_classes(cuda):
    """Both classes with a "log" lambda weight, sample weights and reduction="sum" give the
    reference's value and gradient; NegativeLogLikelihoodLoss takes logits [N, L]."""
    rng = np.random.default_rng(21)
    B, R, L, H = 2, 3, 9, 8
    pred, y = _lists(rng, B, H * H, R, L)
    y[1, 0, 4, 1] = -1.0
    calls = []

    class Log2:  # an object that only has tfr's method
        def individual_weights(self, labels, ranks):
            calls.append(1)
            return labels / np.log2(1.0 + np.asarray(ranks, np.float64))

    w = lambda_weight_by_name("log").rank_weights(L)
    for sw in (rng.uniform(0.5, 2.0, B * R).astype(np.float32),
               rng.uniform(0.5, 2.0, (B, 1)).astype(np.float32)):
        fn = HourglassNegativeLogLikelihood(L, B, reduction="sum", lambda_weight=Log2())
        assert np.array_equal(fn.rank_weights, w)
        val, g = fn.loss_and_grad(y, pred.reshape(B, H, H, 1), sample_weight=sw)
        val2 = fn(y, torch.from_numpy(pred.reshape(B, H, H, 1)).to(cuda), sample_weight=sw)
        torch.cuda.synchronize()
        ref, dref, _ = WR.hourglass_weighted(y, pred, B, L, w, sw, "sum")
        assert tuple(g.shape) == (B, H, H, 1) and val.item() == val2.item()
        assert err(val.item(), ref) < BAR and err(g.cpu().numpy().reshape(B, -1), dref) < BAR
    assert len(calls) == 2  # once per loss object, not per call
    N = 7
    s = rng.standard_normal((N, L)).astype(np.float32)
    lab = (rng.permutation(N * L).reshape(N, L) / (N * L)).astype(np.float32)
    lab[2, 4] = -1.0
    sw = rng.uniform(0.5, 2.0, N).astype(np.float32)
    sw[3] = 0.0
    fn = NegativeLogLikelihoodLoss(L, reduction="sum", lambda_weight=lambda_weight_by_name("log"))
    val, g = fn.loss_and_grad(lab, s, sample_weight=sw)
    torch.cuda.synchronize()
    nll_ref, g_ref = WR.listmle_weighted_fwd_bwd(s, lab, w)
    assert tuple(g.shape) == (N, L)
    assert err(val.item(), (sw * nll_ref).sum()) < BAR
    assert err(g.cpu().numpy(), g_ref * sw[:, None]) < BAR
    assert g[2, 4].item() == 0.0 and np.array_equal(g[3].cpu().numpy(), np.zeros(L, np.float32))
    # defaults: the value of the unweighted loss
    plain = NegativeLogLikelihoodLoss(L)(lab, s)
    torch.cuda.synchronize()
    assert err(plain.item(), LM.listmle_fwd_bwd(s, lab)[0].mean()) < BAR


# ----------------------------------------------------------------------------- through the model
def _model(B, L, R, H):
    from pldepth_amd.losses.losses_meta import DepthLossType
    from pldepth_amd.models.models_meta import ModelParameters, get_model_type_by_name
    from pldepth_amd.models.PLDepthNet import get_pl_depth_net
    mp = ModelParameters()
    mp.set_parameter("model_type", get_model_type_by_name("ff_effnet"))
    mp.set_parameter("ranking_size", L)
    mp.set_parameter("rankings_per_image", R)
    mp.set_parameter("val_rankings_per_img", R)
    mp.set_parameter("batch_size", B)
    mp.set_parameter("loss_type", DepthLossType.NLL)
    mp.set_parameter("seed", 0)
    return get_pl_depth_net(mp, [H, H, 3])[0]


def _spy(monkeypatch):
    counts = {"plain": 0, "weighted": 0}
    plain, weighted = K.listmle_fwd_bwd, K.listmle_weighted_fwd_bwd

    def spy_plain(*a, **kw):
        counts["plain"] += 1
        return plain(*a, **kw)

    def spy_weighted(*a, **kw):
        counts["weighted"] += 1
        return weighted(*a, **kw)

    monkeypatch.setattr(K, "listmle_fwd_bwd", spy_plain)
    monkeypatch.setattr(K, "listmle_weighted_fwd_bwd", spy_weighted)
    return counts


def test_through_the_model(cuda, fixed_schedules, monkeypatch):
    """compile(loss with lambda weights) -> evaluate -> train_on_batch (eager, replayed, with
    sample weights after the capture, without them again). The trainer's loss, nll and dpred are
    compared with the reference evaluated on that step's own prediction and rankings, read back
    from the device, so drop-connect and BN mode play no part."""
    from pldepth_amd.optimizers import Adam
    B, H, R, L = 2, 64, 4, 5
    rng = np.random.default_rng(3)
    x = rng.random((B, H, H, 3)).astype(np.float32)
    _, y = _lists(rng, B, H * H, R, L)
    counts = _spy(monkeypatch)
    loss_fn = HourglassNegativeLogLikelihood(L, B, lambda_weight=lambda_weight_by_name("pow2"))
    w = loss_fn.rank_weights
    assert np.array_equal(w, np.array([1, 0.5, 0.25, 0.125, 0.0625], np.float32))
    model = _model(B, L, R, H)
    model.compile(loss=loss_fn, optimizer=Adam(0.01, amsgrad=True))
    # evaluate / val_loss go through the loss object: inference-mode prediction, same weights
    # (before any training step: the BN moving statistics are still their initial values)
    val = model.evaluate([(x, y)])
    pred = model(x, training=False).cpu().numpy().reshape(B, -1)
    ref = WR.hourglass_weighted(y, pred, B, L, w, None, "mean")[0]
    print("model evaluate: %.6g vs %.6g" % (val, ref))
    assert np.isfinite(val) and err(val, ref) < BAR and counts["weighted"] == 1
    tr = model.trainer
    captures = []
    capture = tr.capture
    monkeypatch.setattr(tr, "capture", lambda: (captures.append(1), capture())[1])

    def check_step(sw, tag):
        torch.cuda.synchronize()
        pred = model.engine.act["pred"].cpu().numpy().reshape(B, -1)
        yt = tr.y_true.cpu().numpy()
        assert np.array_equal(yt, y)
        ref, dref, nref = WR.hourglass_weighted(yt, pred, B, L, w, sw, "mean")
        e = (err(tr.loss.item(), ref), err(tr.nll.cpu().numpy(), nref),
             err(tr.dpred.cpu().numpy().reshape(B, -1), dref))
        print("model %s: err loss %.3g nll %.3g dpred %.3g" % (tag, *e))
        assert max(e) < BAR, (tag, e)
        return ref

    v = model.train_on_batch(x, y)  # eager step, then the capture
    assert err(v, check_step(None, "eager")) < BAR and len(captures) == 1
    model.train_on_batch(x, y)  # replayed
    check_step(None, "replay")
    model.train_on_batch(x, y)
    check_step(None, "replay 2")
    assert len(captures) == 1 and tr.list_w is None
    sw = np.array([0.5, 3.0], np.float32)  # per image
    v = model.train_on_batch(x, y, sample_weight=sw)  # captured again, once
    assert err(v, check_step(sw, "weights, eager")) < BAR and len(captures) == 2
    model.train_on_batch(x, y, sample_weight=np.repeat(sw[::-1], R))  # per list, replayed
    check_step(sw[::-1], "weights, replay")
    model.train_on_batch(x, y)  # weights of one again: a refill, no capture
    check_step(None, "no weights, replay")
    assert len(captures) == 2
    assert counts["plain"] == 0 and counts["weighted"] > 0
    # refused at compile()
    with pytest.raises(ValueError):
        model.compile(loss=HourglassNegativeLogLikelihood(L, B, reduction="none"))
    # the same model compiled with the default loss runs the unweighted call
    counts["plain"] = counts["weighted"] = 0
    model.compile(loss=HourglassNegativeLogLikelihood(L, B), optimizer=Adam(0.01, amsgrad=True))
    model.train_on_batch(x, y)
    model.train_on_batch(x, y)
    torch.cuda.synchronize()
    assert counts["plain"] > 0 and counts["weighted"] == 0
    pred = model.engine.act["pred"].cpu().numpy().reshape(B, -1)
    ref0 = LM.hourglass_nll(y, pred, B, L)[0]
    assert err(model.trainer.loss.item(), ref0) < BAR
