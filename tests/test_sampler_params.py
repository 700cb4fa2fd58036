"""CPU tests of the samplers' run-time arguments: the parametrised restatement
(tests/sampler_params_ref.py) against the reference's recorded outputs
(golden/sampler_params_golden.npz, written by golden/make_sampler_params_golden.py) and against
oracle/sampler.py at the defaults; the strategy classes' constructors and hierarchy; the host-only
argument checks of pld_sampler_rank_ex."""
import ctypes as C
import os

import numpy as np
import pytest

import sampler_params_ref as P
from oracle import sampler as S
from pldepth_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
STRATEGIES, N_CASES = P.GOLDEN_STRATEGIES, P.GOLDEN_CASES


@pytest.fixture(scope="module")
def pgolden():
    return np.load(os.path.join(HERE, "golden", "sampler_params_golden.npz"))


def test_golden_holds_the_issue_cases(pgolden):
    assert pgolden["cases"].tolist() == [
        [24, 32, 24, 32, 5, 20, 0.1, -2.5, 2.2], [24, 32, 12, 16, 9, 10, 0.3, -1000, 1.5],
        [20, 28, 40, 14, 70, 6, 0.01, -7, 3], [16, 16, 16, 16, 3, 15, 0.5, -0.1, 1.0]]


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("ci", range(N_CASES))
def test_restatement_equals_reference_golden(pgolden, ci, strategy):
    gt, mask, L, R, tau, pen, factor = P.load_case(pgolden, ci)
    ref = pgolden[f"c{ci}_{strategy}_out"]
    mine = P.sample_point_batch(strategy, mask, gt, R, L,
                                P.case_draws(pgolden, ci, strategy, gt.shape[1]), tau, pen, factor)
    assert mine.shape == ref.shape == (min(int(R * factor), R), L, 2)
    assert np.array_equal(P.canonical_lists(mine), P.canonical_lists(ref))


@pytest.mark.parametrize("strategy", ["thresh", "info", "pure", "masked"])
@pytest.mark.parametrize("ci", range(4))
def test_restatement_at_defaults_equals_oracle(golden, ci, strategy):
    h, w, L, R = [int(v) for v in golden[f"c{ci}_shape"]]
    R = min(R, 12)  # the first draws of the recorded sequence: the restatement is per candidate
    mask = np.unpackbits(golden[f"c{ci}_mask"])[: h * w].reshape(h, w).astype(np.float32)
    gt = golden[f"c{ci}_codes"].astype(np.float32) / np.float32(255)
    nc = S.n_candidates(R, strategy)
    draws = golden[f"c{ci}_{strategy}_draws"][: nc * L]
    ref, _ = S.sample_masked_point_batch(strategy, mask, gt, R, L, draws)
    assert np.array_equal(P.sample_point_batch(strategy, mask, gt, R, L, draws), ref)
    assert np.array_equal(
        P.sample_point_batch(strategy, mask, gt, R, L, draws, 0.03, -1000, S.FACTORS[strategy]),
        ref)


def test_classes_take_and_report_non_default_arguments():
    from pldepth.data import sampling as PS
    mp = P.Params(ranking_size=7, downscaling_factor=2)
    t = PS.ThresholdedMaskedRandomSamplingStrategy(mp, 0.1, -5)
    assert (t.threshold, t.equality_penalty, t.num_points_per_sample) == (0.1, -5, 7)
    assert "threshold=0.1" in str(t) and "equality_penalty=-5" in str(t)
    i = PS.InformationScoreBasedSampling(mp, threshold=0.25, equality_penalty=-3.5)
    assert (i.threshold, i.equality_penalty) == (0.25, -3.5)
    assert str(i) == "InformationScoreBasedSampling(num_points_per_sample=7, threshold=0.25)"
    # candidate counts and what is kept: int(R * factor), min(n_cand, R); defaults recognised
    assert t.rank_arguments(20, 2.2) == (44, 20, False)
    assert t.rank_arguments(15, 1.0) == (15, 15, False)
    assert PS.ThresholdedMaskedRandomSamplingStrategy(mp).rank_arguments(100) == (150, 100, True)
    assert PS.InformationScoreBasedSampling(mp).rank_arguments(100) == (500, 100, True)
    assert PS.InformationScoreBasedSampling(mp).rank_arguments(100, 4)[2] is False
    assert PS.PurelyMaskedRandomSamplingStrategy(mp).rank_arguments(100) == (80, 80, True)
    assert PS.PurelyMaskedRandomSamplingStrategy(mp).rank_arguments(10, 3) == (30, 10, False)
    for bad in (None, -0.1, float("nan")):
        with pytest.raises(ValueError):
            PS.InformationScoreBasedSampling(mp, threshold=bad)
        with pytest.raises(ValueError):
            PS.ThresholdedMaskedRandomSamplingStrategy(mp, bad)


def test_random_strategy_and_hierarchy_match_the_reference():
    from pldepth.data.sampling import (InformationScoreBasedSampling,
                                       MaskedRandomSamplingStrategy,
                                       PurelyMaskedRandomSamplingStrategy, RandomSamplingStrategy,
                                       SamplingStrategy, ThresholdedMaskedRandomSamplingStrategy)
    assert RandomSamplingStrategy.__mro__[1] is SamplingStrategy
    assert PurelyMaskedRandomSamplingStrategy.__mro__[1] is RandomSamplingStrategy
    assert MaskedRandomSamplingStrategy.__mro__[1] is PurelyMaskedRandomSamplingStrategy
    assert ThresholdedMaskedRandomSamplingStrategy.__mro__[1] is MaskedRandomSamplingStrategy
    assert InformationScoreBasedSampling.__mro__[1] is MaskedRandomSamplingStrategy
    r = RandomSamplingStrategy(P.Params(ranking_size=4, downscaling_factor=2))
    assert (r.threshold, r.downscaling_factor, r.num_points_per_sample) == (0.03, 2, 4)
    assert str(r) == "RandomSamplingStrategy(num_points_per_sample=4)"
    assert r.rank_arguments(10)[:2] == (15, 10)
    res, gts, pts, dists = r.initialize_buffers(10, 1.5)
    assert res.shape == (15, 4, 2) and res.dtype == np.float32
    assert gts.shape == pts.shape == (4,) and dists.shape == (15,)
    d = np.array([0.5, 0.125, 1.0, 0.25], np.float32)
    assert SamplingStrategy.calculate_depth_differences(d) == 0.875  # max - min, exactly here


def test_rank_ex_host_checks_raise_before_any_launch():
    """Every scalar argument is checked on the host before a pointer is looked at or a kernel
    launched: these calls carry no device memory at all."""
    lib = _lib.lib()
    assert _lib.CONST["PLD_SAMPLER_RANDOM"] == 4
    need = C.c_size_t()
    lib.pld_sampler_rank_ex_workspace_size(2, 30, 5, C.byref(need))
    assert need.value >= 2 * 30 * 5 * 2 * 4 + 2 * 30 * 8
    with pytest.raises(_lib.PLDError, match="bad args"):
        lib.pld_sampler_rank_ex_workspace_size(2, 0, 5, C.byref(need))

    def call(n_cand=30, L=5, tau=0.1, penalty=-5.0, ws_bytes=None, strategy=2, H=8, W=8,
             mh=8, mw=8):
        ws_bytes = need.value if ws_bytes is None else ws_bytes
        lib.pld_sampler_rank_ex(None, None, None, None, None, 2, H, W, mh, mw, 20, L, n_cand,
                                strategy, tau, penalty, None, None, ws_bytes, None)

    with pytest.raises(_lib.PLDError, match="tau"):
        call(tau=-0.01)
    with pytest.raises(_lib.PLDError, match="tau"):
        call(tau=float("nan"))
    with pytest.raises(_lib.PLDError, match="tau"):
        call(tau=float("inf"))
    with pytest.raises(_lib.PLDError, match="penalty"):
        call(penalty=float("nan"))
    with pytest.raises(_lib.PLDError, match="n_cand"):
        call(n_cand=0)
    with pytest.raises(_lib.PLDError, match="n_cand"):
        call(n_cand=-3)
    with pytest.raises(_lib.PLDError, match="L=513 > 512"):
        call(L=513)
    with pytest.raises(_lib.PLDError, match="workspace"):
        call(ws_bytes=need.value - 1)
    with pytest.raises(_lib.PLDError, match="bad strategy"):
        call(strategy=5)
    with pytest.raises(_lib.PLDError, match="2\\^24"):
        call(H=4096, W=4096)
    with pytest.raises(_lib.PLDError, match="bad args"):
        call(mh=0)
    with pytest.raises(_lib.PLDError, match="null pointer"):
        call()  # every scalar in range: the pointers are looked at last
    # the LDS selection buffer holds 150 KB of scores: 19200 candidates, pure aside
    big = C.c_size_t()
    lib.pld_sampler_rank_ex_workspace_size(2, 19201, 2, C.byref(big))
    with pytest.raises(_lib.PLDError, match="LDS selection buffer"):
        call(n_cand=19201, L=2, ws_bytes=big.value)
    with pytest.raises(_lib.PLDError, match="null pointer"):
        call(n_cand=19201, L=2, ws_bytes=big.value, strategy=0)
