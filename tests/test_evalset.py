"""Test-set evaluation, host side: the reference's import paths, the DAO dispatch, the NumPy
restatement of the four kernels (tests/evalset_ref.py) against the goldens the reference wrote
(tests/golden/evalset_golden.npz), and the vectorised draws' RNG contract."""
import importlib
import os

import numpy as np
import pytest

import evalset_ref as ER

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(HERE, "golden", "evalset_golden.npz")) as z:
        return {k: z[k] for k in z.files}


def _gts8(gold):
    return gold["codes"].astype(np.float32) / np.float32(255.0)


@pytest.mark.parametrize("path", [
    "data.dao.dao_meta", "data.dao.ibims", "data.dao.diode", "data.dao.sintel", "data.dao.tum",
    "data.providers.generic_ranking_provider", "test_data_eval"])
def test_reference_import_paths_resolve(path):
    mod = importlib.import_module("pldepth." + path)
    assert mod is importlib.import_module("pldepth_amd." + path)
    assert mod.__name__ == "pldepth_amd." + path


def test_reference_names_exist():
    from pldepth.data.data_meta import TESTING_ONLY_STR, TFDatasetDataProvider
    from pldepth.data.providers.generic_ranking_provider import (
        GenericHourglassPairRelationDataProvider as PairP,
        GenericHourglassRankingDataProvider as RankP)
    from pldepth.test_data_eval import eval_model
    assert issubclass(PairP, TFDatasetDataProvider) and issubclass(RankP, TFDatasetDataProvider)
    assert TESTING_ONLY_STR.format("TUM", "training") == \
        "TUM is intended to be used for testing only and, thus, this DAO does not provide a " \
        "training set."
    for cls in (PairP, RankP):
        for name in ("provide_train_dataset", "provide_val_dataset", "provide_test_dataset"):
            assert callable(getattr(cls, name))
    assert RankP.assure_no_equal_relation([1.0, 2.0], 2.01, 2, 0.03) is False
    assert RankP.assure_no_equal_relation([1.0, 2.0], 3.0, 2, 0.03) is True
    opts = {p.name for p in eval_model.params}
    assert opts == {"model_name", "load_model_path", "dataset", "data_path", "data_npz",
                    "input_size", "batch_size", "seed", "ranking_size", "val_rankings_per_img",
                    "equality_threshold", "cache"}


class _Params:
    def __init__(self, **p):
        self.p = p

    def get_parameter(self, name, default=None):
        return self.p.get(name, default)


def test_providers_refuse_training_and_need_a_config_to_cache():
    from pldepth_amd.data.providers import generic_ranking_provider as G
    mp = _Params(dataset="SINTEL", val_rankings_per_img=5)
    with pytest.raises(NotImplementedError):
        G.GenericHourglassPairRelationDataProvider(mp, 0, True).provide_train_dataset(None)
    with pytest.raises(NotImplementedError):
        G.GenericHourglassRankingDataProvider(mp, 5, 0, True).provide_train_dataset(None)
    with pytest.raises(AssertionError):
        G.GenericHourglassPairRelationDataProvider(mp, 0, True, save_pairs_on_disk=True)
    with pytest.raises(AssertionError):
        G.GenericHourglassRankingDataProvider(mp, 5, 0, True, save_rankings_on_disk=True)


def test_dao_dispatch(tmp_path):
    from pldepth_amd.data.dao import dao_meta
    from pldepth_amd.data.io_utils import Dataset
    from pldepth_amd.util.env import get_config
    config = get_config(path=str(tmp_path / "none.ini"))
    names = {Dataset.IBIMS: "IbimsTFDataAccessObject", Dataset.DIODE: "DIODETFDataAccessObject",
             Dataset.SINTEL: "SintelTFDataAccessObject", Dataset.TUM: "TUMTFDataAccessObject",
             Dataset.HR_WSI: "HRWSITFDataAccessObject"}
    for ds, cls in names.items():
        key = ds.name + "_ROOT_PATH"
        assert key in config["DATA"]  # env.get_config lists a default for every root
        config["DATA"][key] = str(tmp_path / ds.name)
        dao = dao_meta.get_dao_for_dataset_type(ds, config, [32, 48, 3], seed=4)
        assert type(dao).__name__ == cls and dao.root_path == str(tmp_path / ds.name)
        if ds != Dataset.HR_WSI:
            for getter, what in ((dao.get_training_dataset, "training"),
                                 (dao.get_validation_dataset, "validation")):
                with pytest.raises(NotImplementedError, match="testing only.*" + what):
                    getter()
    assert dao.seed == 4
    with pytest.raises(NotImplementedError, match="does not support dataset type 'NYU'"):
        dao_meta.get_dao_for_dataset_type("NYU", config, [32, 48, 3])


# ------------------------------------------------------------------ restatement == reference
@pytest.mark.parametrize("inv", [0, 1])
def test_ref_pairs_reproduce_golden(gold, inv):
    got = ER.ordinal_pairs(_gts8(gold), gold["pairs_draws"], 0.03, bool(inv))
    want = gold[f"pairs_inv{inv}"]
    assert got.dtype == want.dtype == np.float32
    assert np.array_equal(got, want)
    assert {-1.0, 0.0, 1.0} == set(np.unique(want[..., 2]))


def tie_groups_equal(got, want):
    """Rankings [.., L, 2]: depth columns identical, and the index column equal wherever a depth
    is unique in its list and equal as a multiset within every group of equal depths."""
    if not np.array_equal(got[..., 1], want[..., 1]):
        return False
    for g, w in zip(got.reshape(-1, *got.shape[-2:]), want.reshape(-1, *want.shape[-2:])):
        for d in np.unique(w[:, 1]):
            m = w[:, 1] == d
            if not np.array_equal(np.sort(g[m, 0]), np.sort(w[m, 0])):
                return False
    return True


@pytest.mark.parametrize("inv", [0, 1])
@pytest.mark.parametrize("L", [5, 40])
def test_ref_rankings_reproduce_golden(gold, L, inv):
    draws = gold[f"rank_draws_L{L}"]
    # no two different pixels tie: exact, index column included (a pixel drawn twice gives two
    # identical rows)
    got = ER.depth_rankings(gold["gts_cont"], draws, bool(inv))
    assert np.array_equal(got, gold[f"rank_cont_L{L}_inv{inv}"])
    # 8-bit depths: the reference's order within a tie group is np.argsort's unstable one
    got = ER.depth_rankings(_gts8(gold), draws, bool(inv))
    assert tie_groups_equal(got, gold[f"rank_q8_L{L}_inv{inv}"])


def test_ref_pair_error_known_answers(gold):
    gts = _gts8(gold)
    for inv in (0, 1):
        pairs = gold[f"pairs_inv{inv}"]
        sign = -1.0 if inv else 1.0
        wrong, counted = ER.ordinal_pair_error(sign * gts, pairs)
        assert counted.sum() == (pairs[..., 2] != 0).sum() and not wrong.any()
        wrong, counted = ER.ordinal_pair_error(-sign * gts, pairs)
        assert np.array_equal(wrong, counted)
        # recomputing at the table's own threshold gives the table's relations
        w2, c2 = ER.ordinal_pair_error(-sign * gts, pairs, tau=0.03, invert=bool(inv))
        assert np.array_equal(w2, wrong) and np.array_equal(c2, counted)
        # a wider threshold counts fewer pairs
        assert ER.ordinal_pair_error(gts, pairs, tau=0.5, invert=bool(inv))[1].sum() < \
            counted.sum()


@pytest.mark.parametrize("k,shape", [(0, (16, 24)), (1, (16, 16)), (2, (16, 24)), (3, (16, 24))])
def test_ref_resize_reproduces_golden(gold, k, shape):
    want = gold[f"resize{k}_out"]
    got = ER.resize_antialias(gold[f"resize{k}_in"], *shape)
    assert got.shape == want.shape and got.dtype == np.float64
    # both are float64 sums of at most a few hundred terms in another order
    assert np.max(np.abs(got - want)) <= 1e-13


def test_antialias_taps_match_the_restatement():
    from pldepth_amd import kernels as K
    assert np.array_equal(K.antialias_taps(12, 16), [1.0])
    assert np.array_equal(K.antialias_taps(16, 16), [1.0])
    t = K.antialias_taps(53, 24)
    sigma = (53 / 24 - 1) / 2
    assert len(t) == int(4 * sigma + 0.5) + 1 and t.dtype == np.float64
    assert abs(t[0] + 2 * t[1:].sum() - 1.0) < 1e-15
    assert np.allclose(t[1:] / t[0], np.exp(-0.5 * np.arange(1, len(t)) ** 2 / sigma ** 2),
                       rtol=1e-14)


def test_synthetic_eval_set_has_a_depth_edge_in_every_map():
    """What makes the depth-edge metrics of the command line's synthetic run defined: every
    ground-truth map has Canny edges (tests/edge_ref.py is the NumPy statement of auto_canny)."""
    import edge_ref
    from pldepth_amd.test_data_eval import synthetic_eval_set
    for seed in range(8):
        imgs, gts = synthetic_eval_set(4, 64, 64, seed)
        assert imgs.shape == (4, 64, 64, 3) and gts.shape == (4, 64, 64)
        assert imgs.dtype == gts.dtype == np.float32 and gts.min() >= 0 and gts.max() == 1
        for g in gts:
            assert (edge_ref.auto_canny(edge_ref.minmax_u8(g)) != 0).sum() > 0
    again = synthetic_eval_set(4, 64, 64, 7)
    assert np.array_equal(again[0], imgs) and np.array_equal(again[1], gts)


# ------------------------------------------------------------------ RNG contract
def test_vectorised_draws_leave_the_rng_where_the_reference_does(gold):
    from pldepth_amd.data.providers import generic_ranking_provider as G
    N, H, W, P, R, seed = (int(v) for v in gold["shape"])
    np.random.seed(seed)
    coords = G.draw_pair_coords(N, H, W, P)
    assert np.array_equal(coords, gold["pairs_draws"])
    assert np.random.randint(1 << 30) == gold["pairs_inv0_next"] == gold["pairs_inv1_next"]
    for L in (5, 40):
        np.random.seed(seed)
        idx = G.draw_ranking_indices(N, H * W, R, L)
        assert np.array_equal(idx, gold[f"rank_draws_L{L}"])
        assert np.random.randint(1 << 30) == gold[f"rank_q8_L{L}_inv0_next"]
        assert gold[f"rank_q8_L{L}_inv0_next"] == gold[f"rank_cont_L{L}_inv1_next"]
