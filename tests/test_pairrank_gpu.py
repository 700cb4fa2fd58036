"""pld_pairrank_fwd_bwd (the pairwise ranking loss over the sampled lists) on the GPU against the
float64 restatement tests/pairrank_ref.py, from the kernel up to train_on_batch / evaluate.

TOLERANCE. tests/test_step_kernels_gpu.py's measure err(got, ref) = max|got - ref| / max|ref| and
its bound 1e-5, on loss, per-list loss and dpred. Exact-zero claims (pixels no valid element
names, invalid elements, lists of sample weight 0 or without a valid pair) are asserted as exact
zeros. Every call gets dpred, per_list and loss pre-filled with NaN. Each comparison prints its
figures before it asserts. Every case that names a tau >= 0 must see all three relations: the
reference's three counts are asserted positive.
"""
import numpy as np
import pytest
import torch

import pairrank_ref as PR
from oracle import listmle as LM
from pldepth_amd import kernels as K
from pldepth_amd.losses.nll_loss import HourglassNegativeLogLikelihood
from pldepth_amd.losses.ranking_loss import (HourglassPairwiseRankingLoss, PairwiseRankingLoss,
                                             pairs_to_lists)

pytestmark = pytest.mark.gpu

BAR = 1e-5
HW0 = 11 * 13
MODES = ("all", "adjacent")
# (tau, invert, equal_weight): every tau, both signs, every equal weight
SETTINGS = ((0.03, False, 1.0), (0.5, True, 0.5), (None, False, 0.0), (0.03, True, 0.0),
            (0.5, False, 1.0), (None, True, 0.5))


def err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _lists(rng, B, HW, R, L, spread=1.0, unique=False):
    """Random pixels (unique per image on request) and, per list, the labels (perm + 1) / L in no
    particular order; the first two labels of every list are planted within 1 % of each other
    (an equal pair at tau 0.03 in both pair modes, however short the list), the third four times
    the second and the fourth a quarter of it, so that a list of four or more holds all three
    relations at every tau >= 0 in either pair mode."""
    pred = (rng.standard_normal((B, HW)) * spread).astype(np.float32)
    if unique:
        idx = np.stack([rng.permutation(HW)[:R * L] for _ in range(B)]).reshape(B, R, L)
    else:
        idx = rng.integers(0, HW, (B, R, L))
    lab = np.stack([(rng.permutation(L) + 1) / L for _ in range(B * R)]).reshape(B, R, L)
    lab = lab.astype(np.float32)
    lab[..., 1] = lab[..., 0] * np.float32(1.005)
    if L >= 4:
        lab[..., 2] = lab[..., 1] * 4
        lab[..., 3] = lab[..., 1] / 4
    y = np.ascontiguousarray(np.stack([idx.astype(np.float32), lab], -1).astype(np.float32))
    return pred, y


def _run(cuda, pred, y, pair_mode="all", tau=0.03, invert=False, ew=1.0, sw=None,
         per_image=False, reduction="mean", zero_dpred=True, prior=None):
    B, R, L = y.shape[:3]
    tp = dev(pred, cuda)
    dpred = torch.full_like(tp, float("nan")) if prior is None else dev(prior, cuda)
    per_list = torch.full((B * R,), float("nan"), device=cuda)
    loss = torch.full((1,), float("nan"), device=cuda)
    out = K.pairrank_fwd_bwd(
        tp, dev(y, cuda), B, R, L, pair_mode=pair_mode, tau=tau, invert=invert, equal_weight=ew,
        list_w=None if sw is None else dev(np.asarray(sw, np.float32), cuda),
        list_w_per_image=per_image, reduction=reduction, dpred=dpred, per_list=per_list,
        loss=loss, zero_dpred=zero_dpred)
    torch.cuda.synchronize()
    assert out[0] is loss and out[1] is dpred and out[2] is per_list
    return loss.item(), dpred.cpu().numpy(), per_list.cpu().numpy()


def _named(y, HW):
    """[B, HW] mask of the pixels that some valid element names (indices here are in range)."""
    B = y.shape[0]
    named = np.zeros((B, HW), bool)
    for b in range(B):
        ok = y[b, ..., 1].reshape(-1) >= 0
        named[b, y[b, ..., 0].reshape(-1)[ok].astype(np.int64)] = True
    return named


def _check(cuda, pred, y, pair_mode="all", tau=0.03, invert=False, ew=1.0, sw=None,
           reduction="mean", tag="", relations=True):
    B, R, L = y.shape[:3]
    per_image = sw is not None and np.size(sw) == B and B != B * R
    loss_ref, dpred_ref, pl_ref, counts = PR.hourglass_pairrank(
        y, pred, B, L, pair_mode, tau, invert, ew, sw, reduction)
    loss, dpred, per_list = _run(cuda, pred, y, pair_mode, tau, invert, ew, sw, per_image,
                                 reduction)
    assert np.isfinite(dpred).all() and np.isfinite(per_list).all() and np.isfinite(loss)
    e = (err(loss, loss_ref), err(per_list, pl_ref), err(dpred, dpred_ref))
    print("pairrank %s B=%d R=%d L=%d %s tau=%s inv=%d ew=%g %s  relations %s  err loss %.3g "
          "per_list %.3g dpred %.3g" % (tag, B, R, L, pair_mode, tau, invert, ew, reduction,
                                        counts, *e))
    if relations and tau is not None:
        assert min(counts) > 0, counts
    assert max(e) < BAR, (tag, e)
    named = _named(y, pred.shape[1])
    assert np.array_equal(dpred[~named], np.zeros(int((~named).sum()), np.float32))
    return loss, dpred, per_list


@pytest.mark.parametrize("pair_mode", MODES)
@pytest.mark.parametrize("L", [2, 3, 64, 65, 128, 129, 256, 257, 512])
def test_every_instance_and_edge(cuda, L, pair_mode):
    """L <= 64, 128, 256, 512 select pair_kernel<1, 2, 4, 8>; 1, 3, 5 lists leave 3, 1, 3 idle
    waves in the last block; logits at spread 1 and 5; HW = 143, so pixels repeat within and
    across lists; every tau, both signs and every equal weight. Lists of two or three cannot hold
    the planted equal pair and both signs at once: there tau 0.5 takes the place of 0.03 and the
    second label is planted per list, so that the batch's lists hold all three relations."""
    rng = np.random.default_rng(3000 + L)
    k = 0
    for B, R in ((1, 1), (3, 1), (1, 5)):
        for spread in (1.0, 5.0):
            tau, invert, ew = SETTINGS[k % len(SETTINGS)]
            k += 1
            pred, y = _lists(rng, B, HW0, R, L, spread)
            if L < 4:
                # the lists of the batch take turns: second label 1 % off the first, 4 x above,
                # 4 x below (one list of two or three cannot hold three relations; three can)
                lab = y[..., 1].reshape(B * R, L)
                for n in range(B * R):
                    lab[n, 1] = lab[n, 0] * np.float32((1.005, 4.0, 0.25)[n % 3])
                y[..., 1] = lab.reshape(B, R, L)
            _check(cuda, pred, y, pair_mode, tau, invert, ew, tag="x%g" % spread,
                   relations=L >= 4 or B * R >= 3)


@pytest.mark.parametrize("pair_mode", MODES)
def test_every_setting_at_short_and_long_lists(cuda, pair_mode):
    """tau in {None, 0.03, 0.5} x invert x equal_weight in {1, 0.5, 0}, all of them, at L = 5
    (one lane group) and L = 130 (two elements per lane, a partial last chunk)."""
    rng = np.random.default_rng(17)
    for L in (5, 130):
        for tau in (None, 0.03, 0.5):
            for invert in (False, True):
                for ew in (1.0, 0.5, 0.0):
                    pred, y = _lists(rng, 2, HW0, 3, L, 2.0)
                    _check(cuda, pred, y, pair_mode, tau, invert, ew)


def test_labels_alone_give_equal_pairs_in_long_lists(cuda):
    """Without planted labels: (perm + 1) / n labels hold equal pairs at tau 0.03 once the list is
    long (L 70 "all", L 130 "adjacent")."""
    rng = np.random.default_rng(23)
    for L, pair_mode in ((70, "all"), (130, "adjacent")):
        B, R = 2, 3
        pred = rng.standard_normal((B, HW0)).astype(np.float32)
        idx = rng.integers(0, HW0, (B, R, L))
        lab = ((rng.permutation(B * R * L).reshape(B, R, L) + 1) / (B * R * L))
        y = np.ascontiguousarray(np.stack([idx, lab], -1).astype(np.float32))
        _check(cuda, pred, y, pair_mode, 0.03, tag="unplanted")


@pytest.mark.parametrize("pair_mode", MODES)
@pytest.mark.parametrize("L", [40, 200])
@pytest.mark.parametrize("pattern", ["front", "last_third", "whole_list"])
def test_invalid_labels(cuda, L, pattern, pair_mode):
    """Label -1: the element forms no pair and gets exactly 0.0 gradient; a list without a valid
    pair gives per_list exactly 0.0. Every pixel is named once."""
    rng = np.random.default_rng(10 * L + len(pattern))
    B, R = 2, 3
    HW = R * L + 7
    for spread in (1.0, 5.0):
        pred, y = _lists(rng, B, HW, R, L, spread, unique=True)
        if pattern == "front":
            y[:, :, 0, 1] = -1.0
            y[0, 0, 5, 1] = y[0, 0, 4, 1] * np.float32(1.005)  # an equal pair past the front
        elif pattern == "last_third":
            y[:, :, L - L // 3:, 1] = -1.0
        else:
            y[0, 1, :, 1] = -1.0
            y[1, 2, :, 1] = -1.0
            y[1, 0, 1:, 1] = -1.0  # one valid element: no pair either
        _, dpred, per_list = _check(cuda, pred, y, pair_mode, 0.03,
                                    tag="%s x%g" % (pattern, spread))
        for b in range(B):
            bad = y[b, ..., 0][y[b, ..., 1] < 0].astype(np.int64)
            assert bad.size and np.array_equal(dpred[b, bad], np.zeros(bad.size, np.float32))
        if pattern == "whole_list":
            assert per_list[1] == 0.0 and per_list[R + 2] == 0.0 and per_list[R] == 0.0
            assert dpred[1, int(y[1, 0, 0, 0])] == 0.0  # the lone valid element
            assert (per_list[[0, 2]] > 0).all()


@pytest.mark.parametrize("B,R", [(2, 3), (3, 1)])
@pytest.mark.parametrize("mode", ["per_list", "per_image"])
def test_sample_weights(cuda, B, R, mode):
    rng = np.random.default_rng(7 * B + R + len(mode))
    L = 70
    HW = R * L + 9
    pred, y = _lists(rng, B, HW, R, L, unique=True)
    n = B * R if mode == "per_list" else B
    sw = rng.uniform(0.25, 3.0, n).astype(np.float32)
    sw[n - 1] = 0.0
    for pair_mode in MODES:
        for reduction in ("mean", "sum"):
            _, dpred, per_list = _check(cuda, pred, y, pair_mode, 0.03, sw=sw,
                                        reduction=reduction, tag=mode)
            # the lists of weight 0: per_list exactly 0.0, and exactly 0.0 on their own pixels
            lists = [B * R - 1] if mode == "per_list" else list(range((B - 1) * R, B * R))
            for ln in lists:
                b, r = divmod(ln, R)
                assert per_list[ln] == 0.0
                own = y[b, r, :, 0].astype(np.int64)
                assert np.array_equal(dpred[b, own], np.zeros(L, np.float32))
            assert (dpred != 0).any() and (per_list[:1] != 0).all()


@pytest.mark.parametrize("pair_mode", MODES)
def test_scalar_weight_of_two_doubles_bit_for_bit(cuda, pair_mode):
    """Scaling by a power of two is exact: loss, per-list loss and dpred of sample_weight=2 are
    twice the weight-1 run's, bit for bit (unique pixels: the order of the atomics plays no
    part)."""
    rng = np.random.default_rng(5)
    B, R, L, H = 2, 3, 70, 16
    pred, y = _lists(rng, B, H * H, R, L, unique=True)
    p4 = pred.reshape(B, H, H, 1)
    for reduction in ("auto", "none"):
        loss_fn = HourglassPairwiseRankingLoss(L, B, pair_mode=pair_mode, reduction=reduction)
        one, g1 = loss_fn.loss_and_grad(y, p4, dpred=torch.full((B, H, H, 1), float("nan"),
                                                               device=cuda))
        one, g1 = one.clone(), g1.clone()
        two, g2 = loss_fn.loss_and_grad(y, p4, sample_weight=2.0,
                                        dpred=torch.full((B, H, H, 1), float("nan"),
                                                         device=cuda))
        torch.cuda.synchronize()
        assert (one > 0).all() and torch.equal(two, 2.0 * one)
        assert torch.equal(g2, 2.0 * g1) and (g1 != 0).any()
        ref = PR.hourglass_pairrank(y, pred, B, L, pair_mode, sample_weight=2.0,
                                    reduction="mean" if reduction == "auto" else "none")
        assert err(two.cpu().numpy(), ref[0]) < BAR
        assert err(g2.cpu().numpy().reshape(B, -1), ref[1]) < BAR


def test_reductions(cuda):
    rng = np.random.default_rng(11)
    B, R, L = 2, 3, 130
    pred, y = _lists(rng, B, HW0, R, L)
    sw = rng.uniform(0.5, 2.0, B * R).astype(np.float32)
    for pair_mode in MODES:
        mean, d_mean, pl_mean = _check(cuda, pred, y, pair_mode, sw=sw, reduction="mean")
        total, d_sum, pl_sum = _check(cuda, pred, y, pair_mode, sw=sw, reduction="sum")
        N = B * R
        print("sum vs N x mean: loss %.3g dpred %.3g" % (err(total, N * mean),
                                                        err(d_sum, N * d_mean)))
        assert err(total, N * mean) < BAR and err(d_sum, N * d_mean) < BAR
        assert np.array_equal(pl_sum, pl_mean)
        # "none" through the loss classes: the [N] vector s_n loss_n, the gradient of its sum
        H = (11, 13)
        vec, g = HourglassPairwiseRankingLoss(L, B, pair_mode=pair_mode, reduction="none") \
            .loss_and_grad(y, pred.reshape(B, *H, 1), sample_weight=sw)
        torch.cuda.synchronize()
        ref_vec, ref_d, _, _ = PR.hourglass_pairrank(y, pred, B, L, pair_mode, sample_weight=sw,
                                                     reduction="none")
        assert tuple(vec.shape) == (N,) and tuple(g.shape) == (B, *H, 1)
        assert err(vec.cpu().numpy(), ref_vec) < BAR
        assert err(g.cpu().numpy().reshape(B, -1), ref_d) < BAR
        s = rng.standard_normal((N, L)).astype(np.float32)
        vec2 = PairwiseRankingLoss(L, pair_mode=pair_mode, reduction="none")(y[..., 1], s)
        torch.cuda.synchronize()
        ref2 = PR.pairrank_lists(s, y[..., 1].reshape(N, L), pair_mode)[0]
        assert tuple(vec2.shape) == (N,) and err(vec2.cpu().numpy(), ref2) < BAR


@pytest.mark.parametrize("B,HW", [(1, 3), (5, 29), (2, 75)])
def test_accumulates_without_zero_dpred(cuda, B, HW):
    rng = np.random.default_rng(B * HW + 2)
    R, L = (1, 2) if HW == 3 else (2, 5)
    pred, y = _lists(rng, B, HW, R, L)
    sw = rng.uniform(0.5, 2.0, B * R).astype(np.float32)
    prior = (0.25 * rng.standard_normal((B, HW))).astype(np.float32)
    for pair_mode in MODES:
        loss_ref, dpred_ref, _, _ = PR.hourglass_pairrank(y, pred, B, L, pair_mode, 0.5,
                                                          sample_weight=sw, reduction="sum")
        loss, dpred, _ = _run(cuda, pred, y, pair_mode, 0.5, sw=sw, reduction="sum",
                              zero_dpred=False, prior=prior)
        e = (err(loss, loss_ref), err(dpred, prior.astype(np.float64) + dpred_ref))
        print("accumulate B=%d HW=%d %s: err loss %.3g dpred %.3g" % (B, HW, pair_mode, *e))
        assert max(e) < BAR
        untouched = ~_named(y, HW)
        assert untouched.any() and np.array_equal(dpred[untouched], prior[untouched])


def test_loss_classes_and_pair_tables(cuda):
    """Both classes with sample weights and reduction="sum" give the reference's value and
    gradient; PairwiseRankingLoss takes logits [N, L]; a pair table of the evaluation providers
    goes through pairs_to_lists, and the relation comes from z0, z1 at the loss's threshold,
    whatever the table's relation column holds."""
    rng = np.random.default_rng(21)
    B, R, L, H = 2, 3, 9, 8
    pred, y = _lists(rng, B, H * H, R, L)
    y[1, 0, 4, 1] = -1.0
    for sw in (rng.uniform(0.5, 2.0, B * R).astype(np.float32),
               rng.uniform(0.5, 2.0, (B, 1)).astype(np.float32)):
        fn = HourglassPairwiseRankingLoss(L, B, threshold=0.5, pair_mode="adjacent",
                                          equal_weight=0.5, invert_relation_sign=True,
                                          reduction="sum")
        val, g = fn.loss_and_grad(y, pred.reshape(B, H, H, 1), sample_weight=sw)
        val2 = fn(y, torch.from_numpy(pred.reshape(B, H, H, 1)).to(cuda), sample_weight=sw)
        torch.cuda.synchronize()
        ref, dref, _, _ = PR.hourglass_pairrank(y, pred, B, L, "adjacent", 0.5, True, 0.5, sw,
                                                "sum")
        assert tuple(g.shape) == (B, H, H, 1) and val.item() == val2.item()
        assert err(val.item(), ref) < BAR and err(g.cpu().numpy().reshape(B, -1), dref) < BAR
    N = 7
    s = rng.standard_normal((N, L)).astype(np.float32)
    lab = _lists(rng, N, 4, 1, L)[1][..., 1].reshape(N, L)
    lab[2, 4] = -1.0
    sw = rng.uniform(0.5, 2.0, N).astype(np.float32)
    sw[3] = 0.0
    fn = PairwiseRankingLoss(L, reduction="sum")
    val, g = fn.loss_and_grad(lab, s, sample_weight=sw)
    torch.cuda.synchronize()
    loss_n, g_ref, counts = PR.pairrank_lists(s, lab)
    assert min(counts) > 0 and tuple(g.shape) == (N, L)
    assert err(val.item(), (sw * loss_n).sum()) < BAR
    assert err(g.cpu().numpy(), g_ref * sw[:, None]) < BAR
    assert g[2, 4].item() == 0.0 and np.array_equal(g[3].cpu().numpy(), np.zeros(L, np.float32))
    # a pair table: P pairs per image, (point0, point1, relation, z0, z1)
    P = 40
    gt = rng.uniform(0.05, 1.0, (B, H * H)).astype(np.float32)
    pts = rng.integers(0, H * H, (B, P, 2))
    table = np.zeros((B, P, 5), np.float32)
    table[..., :2] = pts
    table[..., 3] = np.take_along_axis(gt, pts[..., 0], 1)
    table[..., 4] = np.take_along_axis(gt, pts[..., 1], 1)
    table[..., 4][:, :3] = table[..., 3][:, :3] * np.float32(1.01)
    table[..., 2] = 7.0  # never read
    yp = pairs_to_lists(table)
    for tau in (0.03, 0.5, None):
        fn = HourglassPairwiseRankingLoss(2, B, threshold=tau)
        val, g = fn.loss_and_grad(yp, pred.reshape(B, H, H, 1))
        torch.cuda.synchronize()
        ref, dref, _, counts = PR.hourglass_pairrank(yp, pred, B, 2, "all", tau)
        print("pair table tau=%s relations %s: err loss %.3g dpred %.3g" % (
            tau, counts, err(val.item(), ref), err(g.cpu().numpy().reshape(B, -1), dref)))
        assert tau is None or min(counts) > 0
        assert err(val.item(), ref) < BAR and err(g.cpu().numpy().reshape(B, -1), dref) < BAR
    # with two elements per list the two pair modes are the same loss
    a = HourglassPairwiseRankingLoss(2, B, pair_mode="adjacent")(yp, pred.reshape(B, H, H, 1))
    b = HourglassPairwiseRankingLoss(2, B, pair_mode="all")(yp, pred.reshape(B, H, H, 1))
    torch.cuda.synchronize()
    assert a.item() == b.item()


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
    mp.set_parameter("loss_type", DepthLossType.RANKING)
    mp.set_parameter("seed", 0)
    return get_pl_depth_net(mp, [H, H, 3])[0]


def _spy(monkeypatch):
    counts = {"plain": 0, "weighted": 0, "pairrank": 0}
    plain, weighted, pairrank = (K.listmle_fwd_bwd, K.listmle_weighted_fwd_bwd,
                                 K.pairrank_fwd_bwd)

    def spy(name, fn):
        def call(*a, **kw):
            counts[name] += 1
            return fn(*a, **kw)
        return call

    monkeypatch.setattr(K, "listmle_fwd_bwd", spy("plain", plain))
    monkeypatch.setattr(K, "listmle_weighted_fwd_bwd", spy("weighted", weighted))
    monkeypatch.setattr(K, "pairrank_fwd_bwd", spy("pairrank", pairrank))
    return counts


def test_through_the_model(cuda, fixed_schedules, monkeypatch, tmp_path):
    """compile(ranking loss) -> evaluate -> train_on_batch (eager, replayed twice, with per-image
    weights after the capture, without them again). The trainer's loss, per-list loss and dpred
    are compared with the reference evaluated on that step's own prediction and rankings, read
    back from the device, so drop-connect and BN mode play no part."""
    from pldepth_amd.optimizers import Adam
    B, H, R, L = 2, 64, 4, 5
    rng = np.random.default_rng(3)
    x = rng.random((B, H, H, 3)).astype(np.float32)
    _, y = _lists(rng, B, H * H, R, L)
    counts = _spy(monkeypatch)
    args = dict(pair_mode="all", tau=0.03, invert=False, equal_weight=0.5)
    loss_fn = HourglassPairwiseRankingLoss(L, B, threshold=0.03, equal_weight=0.5)
    assert loss_fn.pair_args == args

    def reference(yt, pred, sw):
        out = PR.hourglass_pairrank(yt, pred, B, L, "all", 0.03, False, 0.5, sw, "mean")
        assert min(out[3]) > 0, out[3]
        return out[:3]

    model = _model(B, L, R, H)
    model.compile(loss=loss_fn, optimizer=Adam(0.01, amsgrad=True))
    assert model.trainer.loss_kind == "pairrank" and model.trainer.pair_args == args
    # evaluate / val_loss go through the loss object: inference-mode prediction
    val = model.evaluate([(x, y)])
    pred = model(x, training=False).cpu().numpy().reshape(B, -1)
    ref = reference(y, pred, None)[0]
    print("model evaluate: %.6g vs %.6g" % (val, ref))
    assert np.isfinite(val) and err(val, ref) < BAR and counts["pairrank"] == 1
    tr = model.trainer
    captures = []
    capture = tr.capture
    monkeypatch.setattr(tr, "capture", lambda: (captures.append(1), capture())[1])

    def check_step(sw, tag):
        torch.cuda.synchronize()
        pred = model.engine.act["pred"].cpu().numpy().reshape(B, -1)
        yt = tr.y_true.cpu().numpy()
        assert np.array_equal(yt, y)
        ref, dref, nref = reference(yt, pred, sw)
        e = (err(tr.loss.item(), ref), err(tr.nll.cpu().numpy(), nref),
             err(tr.dpred.cpu().numpy().reshape(B, -1), dref))
        print("model %s: err loss %.3g per_list %.3g dpred %.3g" % (tag, *e))
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
    model.train_on_batch(x, y)  # weights of one again: a refill, no capture
    check_step(None, "no weights, replay")
    assert len(captures) == 2
    assert counts["plain"] == 0 and counts["weighted"] == 0 and counts["pairrank"] > 1
    # a saved model records the loss's class name (the loss itself is given again at compile())
    import json

    from pldepth_amd.util import hdf5
    path = str(tmp_path / "ranking_model.h5")
    model.save(path)
    value = np.asarray(hdf5.load(path).attrs["training_config"]).item()
    cfg = json.loads(value.decode("utf8") if isinstance(value, bytes) else value)
    assert cfg["loss"] == "HourglassPairwiseRankingLoss"
    # the same model compiled with the default NLL loss runs the ListMLE call and not this one
    for k in counts:
        counts[k] = 0
    model.compile(loss=HourglassNegativeLogLikelihood(L, B), optimizer=Adam(0.01, amsgrad=True))
    assert model.trainer.loss_kind == "nll" and model.trainer.pair_args == {}
    model.train_on_batch(x, y)
    model.train_on_batch(x, y)
    torch.cuda.synchronize()
    assert counts["plain"] > 0 and counts["weighted"] == 0 and counts["pairrank"] == 0
    pred = model.engine.act["pred"].cpu().numpy().reshape(B, -1)
    ref0 = LM.hourglass_nll(y, pred, B, L)[0]
    assert err(model.trainer.loss.item(), ref0) < BAR
