"""Pairwise ranking loss, CPU side: the float64 yardstick (tests/pairrank_ref.py) against torch
autograd and finite differences, known answers, the small mirror additions
(get_depth_relation_tf, DepthLossType.RANKING, the factories), every argument refusal of the loss
classes, the trainer and the C entry point, and the command line. No GPU is touched."""
import ctypes as C

import numpy as np
import pytest
import torch

import pairrank_ref as PR
from pldepth_amd import _lib

HW0 = 11 * 13


def _lists(rng, B, HW, R, L, spread=1.0):
    pred = (rng.standard_normal((B, HW)) * spread).astype(np.float32)
    idx = rng.integers(0, HW, (B, R, L))
    lab = ((rng.permutation(B * R * L).reshape(B, R, L) + 1) / (B * R * L)).astype(np.float32)
    return pred, np.ascontiguousarray(np.stack([idx.astype(np.float32), lab], -1))


def _torch_loss(pred, y, B, L, pair_mode, tau, invert, ew, sw, reduction):
    """The section "The loss" written with torch ops in float64, for autograd. Relations are
    constants (no gradient flows through them): taken from the yardstick's relation32."""
    rk = y.reshape(B, -1, L, 2)
    idx = torch.from_numpy(rk[..., 0].reshape(B, -1).astype(np.int64))
    t = torch.gather(pred, 1, idx).reshape(-1, L)
    z = rk[..., 1].reshape(-1, L)
    i, j = PR.pair_indices(L, pair_mode)
    valid = torch.from_numpy((z[:, i] >= 0) & (z[:, j] >= 0))
    r = torch.from_numpy(PR.relation32(z[:, i], z[:, j], tau, invert)).double()
    d = t[:, i] - t[:, j]
    # (not torch's softplus: past its threshold of 20 it returns x itself, off by e^-20 = 2e-9)
    x = -r * d
    l = torch.where(r != 0, torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs())), ew * d * d)
    l = torch.where(valid, l, torch.zeros_like(l))
    n = valid.sum(1)
    loss_n = l.sum(1) / torch.clamp(n, min=1)
    N = loss_n.shape[0]
    per_list = torch.from_numpy(PR.list_weights(sw, N, B)) * loss_n
    return per_list.sum() / N if reduction == "mean" else per_list.sum()


@pytest.mark.parametrize("L", [2, 5, 70, 130])
@pytest.mark.parametrize("pair_mode", ["all", "adjacent"])
def test_reference_gradient_against_autograd(L, pair_mode):
    rng = np.random.default_rng(100 + L)
    B, R = 2, 3
    worst = 0.0
    for spread in (1.0, 5.0):
        for tau, invert, ew, red in ((0.03, False, 1.0, "mean"), (0.5, True, 0.5, "sum"),
                                     (None, False, 0.0, "mean")):
            pred, y = _lists(rng, B, HW0, R, L, spread)
            y[0, 1, L // 2, 1] = -1.0
            sw = rng.uniform(0.5, 2.0, B * R)
            loss, dpred, per_list, _ = PR.hourglass_pairrank(y, pred, B, L, pair_mode, tau,
                                                             invert, ew, sw, red)
            p = torch.tensor(pred, dtype=torch.float64, requires_grad=True)
            tl = _torch_loss(p, y, B, L, pair_mode, tau, invert, ew, sw, red)
            tl.backward()
            e = max(abs(loss - tl.item()) / abs(tl.item()),
                    float(np.abs(dpred - p.grad.numpy()).max() / np.abs(p.grad.numpy()).max()))
            worst = max(worst, e)
    print("pairrank ref vs autograd L=%d %s: worst %.3g" % (L, pair_mode, worst))
    assert worst < 1e-10


@pytest.mark.parametrize("pair_mode", ["all", "adjacent"])
def test_reference_gradient_against_finite_differences(pair_mode):
    rng = np.random.default_rng(7)
    B, R, L, HW = 2, 2, 6, 17
    pred, y = _lists(rng, B, HW, R, L, 2.0)
    y[1, 0, 2, 1] = y[1, 0, 3, 1] * np.float32(1.005)  # an equal pair at tau 0.03
    y[0, 1, 4, 1] = -1.0
    sw = rng.uniform(0.5, 2.0, B * R)
    args = (B, L, pair_mode, 0.03, False, 0.7, sw, "mean")
    loss, dpred, _, counts = PR.hourglass_pairrank(y, pred, *args)
    assert min(counts) > 0
    p64 = pred.astype(np.float64)
    h = 1e-6
    fd = np.zeros_like(p64)
    for b in range(B):
        for k in range(HW):
            up, dn = p64.copy(), p64.copy()
            up[b, k] += h
            dn[b, k] -= h
            fd[b, k] = (PR.hourglass_pairrank(y, up, *args)[0]
                        - PR.hourglass_pairrank(y, dn, *args)[0]) / (2 * h)
    e = np.abs(fd - dpred).max() / np.abs(dpred).max()
    print("pairrank ref vs central differences (%s): %.3g" % (pair_mode, e))
    # the central difference's own error: h^2 f''' / 6 ~ 1e-13, plus rounding 1e-16 / h ~ 1e-10
    assert e < 1e-7


def test_known_answers_at_two_elements():
    y = np.zeros((1, 1, 2, 2), np.float32)
    y[0, 0, :, 0] = (0, 1)
    flat = np.array([[0.3, 0.3]])
    for z, r in (((0.9, 0.1), 1), ((0.1, 0.9), -1)):
        y[0, 0, :, 1] = z
        loss, dpred, per_list, counts = PR.hourglass_pairrank(y, flat, 1, 2)
        assert abs(loss - np.log(2.0)) < 1e-15 and abs(per_list[0] - np.log(2.0)) < 1e-15
        assert np.allclose(dpred, [[-r / 2, r / 2]], rtol=0, atol=1e-15)
        assert counts == ((1, 0, 0) if r < 0 else (0, 0, 1))
        inv = PR.hourglass_pairrank(y, flat, 1, 2, invert=True)
        assert np.allclose(inv[1], [[r / 2, -r / 2]], rtol=0, atol=1e-15)
    # an equal pair: equal_weight d^2, gradient 2 equal_weight d
    y[0, 0, :, 1] = (0.5, 0.505)
    pred = np.array([[0.75, 0.25]])
    for ew in (1.0, 0.5, 0.0):
        loss, dpred, _, counts = PR.hourglass_pairrank(y, pred, 1, 2, equal_weight=ew)
        assert counts == (0, 1, 0) and abs(loss - ew * 0.25) < 1e-15
        assert np.allclose(dpred, [[ew, -ew]], rtol=0, atol=1e-15)
    # the same depths are unequal under the plain comparison
    assert PR.hourglass_pairrank(y, pred, 1, 2, tau=None)[3] == (1, 0, 0)
    # a pair with an invalid element: no pair, loss 0, gradient 0
    y[0, 0, 1, 1] = -1.0
    loss, dpred, per_list, counts = PR.hourglass_pairrank(y, pred, 1, 2)
    assert loss == 0.0 and per_list[0] == 0.0 and counts == (0, 0, 0)
    assert np.array_equal(dpred, np.zeros((1, 2)))


def test_relation_falls_like_the_scalar_helper_on_float32():
    """relation32 is get_depth_relation on np.float32 scalars, element by element, thresholds
    included (labels k/64 put many ratios exactly on 1.5 and 1/1.5)."""
    from pldepth_amd.data.depth_utils import get_depth_relation
    z = (np.arange(1, 65) / 64).astype(np.float32)
    zi, zj = np.meshgrid(z, z, indexing="ij")
    for tau in (0.5, 0.03, None):
        got = PR.relation32(zi, zj, tau)
        want = np.array([[get_depth_relation(a, b, tau) for b in z] for a in z])
        assert np.array_equal(got, want), tau
        assert np.array_equal(PR.relation32(zi, zj, tau, invert=True), -want)
    on = np.isclose(zi / zj, 1.5, rtol=0, atol=0) | np.isclose(zj / zi, 1.5, rtol=0, atol=0)
    assert on.sum() > 20


def test_sum_is_n_times_mean():
    rng = np.random.default_rng(3)
    B, R, L = 2, 3, 9
    pred, y = _lists(rng, B, HW0, R, L)
    sw = rng.uniform(0.5, 2.0, B * R)
    mean = PR.hourglass_pairrank(y, pred, B, L, sample_weight=sw, reduction="mean")
    total = PR.hourglass_pairrank(y, pred, B, L, sample_weight=sw, reduction="sum")
    none = PR.hourglass_pairrank(y, pred, B, L, sample_weight=sw, reduction="none")
    N = B * R
    assert abs(total[0] - N * mean[0]) < 1e-12 * total[0]
    assert np.allclose(total[1], N * mean[1], rtol=1e-12, atol=0)
    assert np.array_equal(total[2], mean[2]) and np.array_equal(none[0], mean[2])
    assert np.array_equal(none[1], total[1])


def test_pairs_to_lists_round_trip():
    from pldepth_amd.losses.ranking_loss import pairs_to_lists
    rng = np.random.default_rng(5)
    n, P = 3, 7
    pairs = np.zeros((n, P, 5), np.float32)
    pairs[..., 0] = rng.integers(0, 50, (n, P))
    pairs[..., 1] = rng.integers(0, 50, (n, P))
    pairs[..., 3:] = rng.random((n, P, 2))
    pairs[..., 2] = np.sign(pairs[..., 3] - pairs[..., 4])
    y = pairs_to_lists(pairs)
    assert y.shape == (n, P, 2, 2) and y.dtype == np.float32 and y.flags["C_CONTIGUOUS"]
    assert np.array_equal(y[..., 0, 0], pairs[..., 0]) and np.array_equal(y[..., 1, 0],
                                                                          pairs[..., 1])
    assert np.array_equal(y[..., 0, 1], pairs[..., 3]) and np.array_equal(y[..., 1, 1],
                                                                          pairs[..., 4])
    back = np.concatenate([y[..., 0, :1], y[..., 1, :1], pairs[..., 2:3], y[..., 0, 1:],
                           y[..., 1, 1:]], -1)
    assert np.array_equal(back, pairs)
    yt = pairs_to_lists(torch.from_numpy(pairs))
    assert isinstance(yt, torch.Tensor) and np.array_equal(yt.numpy(), y)
    assert pairs_to_lists(pairs[0]).shape == (P, 2, 2)
    # the relation the loss recomputes from z0, z1 is the stored one under the plain comparison
    assert np.array_equal(PR.relation32(y[..., 0, 1], y[..., 1, 1], None), pairs[..., 2])
    for bad in (np.zeros((4, 4)), np.zeros(5)):
        with pytest.raises(ValueError):
            pairs_to_lists(bad)


def test_get_depth_relation_tf():
    from pldepth_amd.data.depth_utils import get_depth_relation, get_depth_relation_tf
    rng = np.random.default_rng(9)
    d = rng.uniform(0.05, 1.0, (500, 2)).astype(np.float32)
    for tau in (0.03, 0.5):
        ratio = d[:, 0].astype(np.float64) / d[:, 1]
        off = (np.abs(ratio - (1 + tau)) > 1e-4) & (np.abs(ratio - 1 / (1 + tau)) > 1e-4)
        got = get_depth_relation_tf(torch.from_numpy(d), tau)
        assert got.dtype == torch.int8 and tuple(got.shape) == (500,)
        want = np.array([get_depth_relation(a, b, tau) for a, b in d])
        assert off.sum() > 450 and np.array_equal(got.numpy()[off], want[off])
        assert set(np.unique(want)) == {-1, 0, 1}
    # on the thresholds: >= gives +1, but -1 needs the strict >. Depths 4 and 8 absorb both
    # epsilons in float32 (half an ulp of 4 is 2.4e-7), so with tau = 1 the ratios are exactly
    # the bounds 2 and 0.5
    on = torch.tensor([[8.0, 4.0], [4.0, 8.0], [4.0, 8.5]])
    assert get_depth_relation_tf(on, 1.0).tolist() == [1, 0, -1]
    # the scalar helper is symmetric there: <= gives -1
    assert [get_depth_relation(np.float32(a), np.float32(b), 1.0) for a, b in on.numpy()] == [
        1, -1, -1]
    # it runs in the dtype asked for, on the tensor's device
    assert get_depth_relation_tf(on.double(), 1.0, dtype=torch.float64).device == on.device


def test_loss_classes_refuse_bad_arguments():
    from pldepth_amd.losses.ranking_loss import (HourglassPairwiseRankingLoss,
                                                 PairwiseRankingLoss)
    from pldepth_amd.losses.lambda_weights import lambda_weight_by_name
    ok = HourglassPairwiseRankingLoss(5, 2)
    assert ok.kind == "pairrank" and ok.reduction == "mean"
    assert ok.pair_args == dict(pair_mode="all", tau=0.03, invert=False, equal_weight=1.0)
    assert (ok.ranking_size, ok.batch_size) == (5, 2)
    plain = PairwiseRankingLoss(2, threshold=None, pair_mode="adjacent", equal_weight=0,
                                invert_relation_sign=True, reduction="none")
    assert plain.pair_args == dict(pair_mode="adjacent", tau=None, invert=True, equal_weight=0.0)
    assert plain.reduction == "none" and plain.kind == "pairrank"
    for make in (lambda **kw: HourglassPairwiseRankingLoss(kw.pop("ranking_size", 5), 2, **kw),
                 lambda **kw: PairwiseRankingLoss(kw.pop("ranking_size", 5), **kw)):
        for bad in (dict(ranking_size=1), dict(ranking_size=0), dict(pair_mode="some"),
                    dict(pair_mode=None), dict(equal_weight=-0.5),
                    dict(equal_weight=float("nan")), dict(equal_weight=float("inf")),
                    dict(threshold=-0.03), dict(threshold=float("nan")),
                    dict(threshold=float("inf")), dict(reduction="average"),
                    dict(lambda_weight=lambda_weight_by_name("log", 5)),
                    dict(lambda_weight=None)):
            with pytest.raises(ValueError):
                make(**bad)
    # sample weights are checked before anything reaches the GPU
    B, R, L = 2, 3, 4
    y = np.zeros((B, R, L, 2), np.float32)
    for bad in (np.ones(5), np.ones((B * R, 2)), np.ones(R)):
        with pytest.raises(ValueError):
            HourglassPairwiseRankingLoss(L, B)(y, np.zeros((B, 5, 5, 1), np.float32),
                                               sample_weight=bad)
    with pytest.raises(ValueError):
        HourglassPairwiseRankingLoss(L, 4)(y, np.zeros((4, 5, 5, 1), np.float32))


def test_module_resolves_through_the_alias_package():
    import pldepth.losses.ranking_loss as alias
    from pldepth_amd.losses import ranking_loss
    assert alias is ranking_loss
    from pldepth.data.depth_utils import get_depth_relation_tf  # noqa: F401


def test_loss_type_and_factories(monkeypatch):
    from pldepth_amd.losses.losses_meta import DepthLossType
    from pldepth_amd.models import effnet_ff, redweb_ff
    from pldepth_amd.models.pl_hourglass import EffNetFullyFledged
    from pldepth_amd.models.redweb import ReDWebNetTFVersion
    assert DepthLossType.RANKING.value == "RANKING" and str(DepthLossType.RANKING) == "RANKING"
    assert [m.name for m in DepthLossType] == ["NLL", "RANKING"]

    class Engine:  # stands in for the device engines: nothing here may touch a GPU
        def __init__(self, shape, batch, seed=0):
            self.B, self.shape = batch, shape

    monkeypatch.setattr(effnet_ff, "EffNetFF", Engine)
    monkeypatch.setattr(redweb_ff, "RedWebFF", Engine)
    for factory in (EffNetFullyFledged, ReDWebNetTFVersion):
        for lt in (DepthLossType.NLL, DepthLossType.RANKING):
            model, pre = factory.get_model_and_normalization([64, 64, 3], 5, lt, batch_size=2)
            assert isinstance(model, factory) and model.engine.shape == (64, 64, 3)
        for lt in ("RANKING", None, "nll"):
            with pytest.raises(ValueError):
                factory.get_model_and_normalization([64, 64, 3], 5, lt, batch_size=2)


def test_compile_reads_the_kind_and_trainer_refuses_rank_weights(monkeypatch):
    """compile() hands the trainer loss_kind and pair_args of a ranking loss and nothing of the
    kind for an NLL loss; the trainer's refusals come before it touches a device."""
    from types import SimpleNamespace

    from pldepth_amd import trainer as T
    from pldepth_amd.losses.nll_loss import HourglassNegativeLogLikelihood
    from pldepth_amd.losses.ranking_loss import HourglassPairwiseRankingLoss
    from pldepth_amd.models.pl_hourglass import FullyFledgedModel
    seen = []
    monkeypatch.setattr(T, "ReplicaTrainer", lambda *a, **kw: seen.append(kw) or "trainer")
    model = FullyFledgedModel(SimpleNamespace(B=2, H=8, W=8))
    loss = HourglassPairwiseRankingLoss(3, 2, threshold=0.1, pair_mode="adjacent",
                                        equal_weight=0.25, reduction="sum")
    model.compile(loss=loss, distribute=(0, 1, None))
    assert seen[-1]["loss_kind"] == "pairrank" and seen[-1]["reduction"] == "sum"
    assert seen[-1]["pair_args"] == dict(pair_mode="adjacent", tau=0.1, invert=False,
                                         equal_weight=0.25)
    assert "rank_weights" not in seen[-1]
    model.compile(loss=HourglassNegativeLogLikelihood(3, 2), distribute=(0, 1, None))
    assert "loss_kind" not in seen[-1] and "pair_args" not in seen[-1]
    with pytest.raises(ValueError, match="none"):
        model.compile(loss=HourglassPairwiseRankingLoss(3, 2, reduction="none"))
    monkeypatch.undo()
    for kw in (dict(loss_kind="pairrank", rank_weights=np.ones(5, np.float32)),
               dict(loss_kind="hinge"), dict(pair_args=dict(pair_mode="all"))):
        with pytest.raises(ValueError):
            T.ReplicaTrainer((8, 8, 3), 2, 5, 1, engine=object(), gpu_sampler=False, **kw)
    assert not torch.cuda.is_initialized()


# -------------------------------------------------------------------- the C entry point's checks
def _call(**kw):
    """pld_pairrank_fwd_bwd on fake (never dereferenced) addresses: every case here is refused
    before any launch."""
    p = C.c_void_p(1 << 20)  # 16-byte aligned
    a = dict(pred=p, y_true=p, B=1, HW=4, R=1, L=3, pair_mode=0, tau=0.03, invert=0, ew=1.0,
             list_w=None, per_image=0, reduction=0, per_list=p, loss=p, dpred=p, zero_dpred=1)
    a.update(kw)
    with pytest.raises(_lib.PLDError) as e:
        _lib.lib().pld_pairrank_fwd_bwd(
            a["pred"], a["y_true"], a["B"], a["HW"], a["R"], a["L"], a["pair_mode"], a["tau"],
            a["invert"], a["ew"], a["list_w"], a["per_image"], a["reduction"], a["per_list"],
            a["loss"], a["dpred"], a["zero_dpred"], None)
    return str(e.value)


def test_entry_point_rejects_bad_arguments_before_any_launch():
    assert _lib.CONST["PLD_PAIRS_ALL"] == 0 and _lib.CONST["PLD_PAIRS_ADJACENT"] == 1
    I32, P, F32, F64 = C.c_int, C.c_void_p, C.c_float, C.c_double
    assert _lib._SIGS["pld_pairrank_fwd_bwd"] == (
        I32, [P, P, I32, I32, I32, I32, I32, F64, I32, F32, P, I32, I32, P, P, P, I32, P])
    assert "pld_pairrank_fwd_bwd" not in _lib._NON_STATUS
    for L in (1, 0, 513, -1):
        assert "L must be 2..512" in _call(L=L)
    for mode in (2, -1):
        assert "unknown pair_mode" in _call(pair_mode=mode)
    for red in (2, -1, 7):
        assert "unknown reduction" in _call(reduction=red)
    for tau in (float("nan"), float("inf"), -float("inf")):
        assert "tau must be finite" in _call(tau=tau)
    for ew in (-1.0, float("nan"), float("inf")):
        assert "equal_weight" in _call(ew=ew)
    assert "2^24" in _call(HW=(1 << 24) + 1)
    # the scalars come first: with every pointer null it is still the scalar that is named
    nulls = dict(pred=None, y_true=None, per_list=None, loss=None, dpred=None)
    assert "unknown pair_mode" in _call(pair_mode=5, **nulls)
    assert "L must be 2..512" in _call(L=1, **nulls)
    for name in nulls:
        assert "null pointer" in _call(**{name: None}), name
    assert "16-byte aligned" in _call(dpred=C.c_void_p((1 << 20) + 4))
    from pldepth_amd import kernels as K
    assert K.PAIRS == {"all": 0, "adjacent": 1}


def test_header_cites_the_reference_for_the_pairwise_loss():
    txt = open(_lib.HEADER).read()
    at = txt.index("Pairwise ranking loss")
    block = txt[at:txt.index("pld_pairrank_fwd_bwd(", at)]
    assert "depth_utils.py:5-36" in block and "generic_ranking_provider.py:108" in block


# ----------------------------------------------------------------------------------------- CLI
def test_cli_options_and_build_loss(monkeypatch):
    from click.testing import CliRunner
    from pldepth_amd import PLDepth
    from pldepth_amd.losses.losses_meta import DepthLossType
    from pldepth_amd.losses.nll_loss import HourglassNegativeLogLikelihood
    from pldepth_amd.losses.ranking_loss import HourglassPairwiseRankingLoss
    opts = {p.name: p for p in PLDepth.perform_pldepth_experiment.params}
    assert opts["loss_type"].default == "nll"
    assert list(opts["loss_type"].type.choices) == ["nll", "ranking"]
    assert opts["pair_mode"].default == "all"
    assert list(opts["pair_mode"].type.choices) == ["all", "adjacent"]
    assert opts["equal_weight"].default == 1.0
    assert isinstance(PLDepth.build_loss(5, 4), HourglassNegativeLogLikelihood)
    loss = PLDepth.build_loss(5, 4, loss_type="ranking", equality_threshold=0.1,
                              pair_mode="adjacent", equal_weight=0.5)
    assert isinstance(loss, HourglassPairwiseRankingLoss)
    assert loss.pair_args == dict(pair_mode="adjacent", tau=0.1, invert=False, equal_weight=0.5)
    assert (loss.ranking_size, loss.batch_size) == (5, 4)
    with pytest.raises(ValueError):
        PLDepth.build_loss(5, 4, "log", loss_type="ranking")
    with pytest.raises(ValueError):
        PLDepth.build_loss(5, 4, loss_type="hinge")
    # the command: the new options reach run_experiment; a discount with ranking is a usage error
    seen = []
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(PLDepth, "run_experiment", lambda **kw: seen.append(kw) or 0)
    res = CliRunner().invoke(PLDepth.perform_pldepth_experiment,
                             ["--loss_type", "ranking", "--pair_mode", "adjacent",
                              "--equal_weight", "0.5", "--equality_threshold", "0.1"])
    assert res.exit_code == 0, res.output
    assert (seen[0]["loss_type"], seen[0]["pair_mode"], seen[0]["equal_weight"]) == (
        "ranking", "adjacent", 0.5) and seen[0]["equality_threshold"] == pytest.approx(0.1)
    res = CliRunner().invoke(PLDepth.perform_pldepth_experiment, [])
    assert res.exit_code == 0 and seen[1]["loss_type"] == "nll"
    res = CliRunner().invoke(PLDepth.perform_pldepth_experiment,
                             ["--loss_type", "ranking", "--listmle_discount", "log"])
    assert res.exit_code == 2 and "listmle_discount" in res.output and len(seen) == 2
    monkeypatch.undo()
    import inspect
    params = inspect.signature(PLDepth.run_experiment).parameters
    assert list(params)[-3:] == ["loss_type", "pair_mode", "equal_weight"]  # last, with defaults
    assert [params[k].default for k in list(params)[-3:]] == ["nll", "all", 1.0]
    assert DepthLossType.RANKING is not DepthLossType.NLL
