"""Test-set evaluation on the GPU: the four kernels of evalset.hip against the goldens the
reference wrote (tests/golden/evalset_golden.npz) and the NumPy restatement (tests/evalset_ref.py,
shown to reproduce those goldens by tests/test_evalset.py), then the providers, the metric, the
DAOs and the command line on top of them."""
import os

import numpy as np
import pytest

import evalset_ref as ER
from test_evalset import _Params, _gts8, gold, tie_groups_equal  # noqa: F401  (gold: fixture)

pytestmark = pytest.mark.gpu


def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


# ------------------------------------------------------------------ pairs
@pytest.mark.parametrize("inv", [0, 1])
def test_pairs_kernel_bit_exact(cuda, gold, inv):
    from pldepth_amd import kernels as K
    got = K.ordinal_pairs(_dev(_gts8(gold), cuda), gold["pairs_draws"], 0.03, bool(inv))
    assert np.array_equal(got.cpu().numpy(), gold[f"pairs_inv{inv}"])


def test_pairs_kernel_other_thresholds_and_sizes(cuda):
    """More than one block, a size that is no multiple of it, tau = None and another tau."""
    from pldepth_amd import kernels as K
    rng = np.random.default_rng(5)
    n, h, w, P = 2, 17, 23, 333
    gts = (rng.integers(0, 64, (n, h, w)) / 63).astype(np.float32)
    coords = rng.integers(0, [h, w, h, w], (n, P, 4))
    for tau in (None, 0.0, 0.2):
        for inv in (False, True):
            got = K.ordinal_pairs(_dev(gts, cuda), coords, tau, inv).cpu().numpy()
            assert np.array_equal(got, ER.ordinal_pairs(gts, coords, tau, inv)), (tau, inv)


@pytest.mark.parametrize("inv", [0, 1])
def test_pair_provider_and_cache(cuda, gold, tmp_path, inv):
    from pldepth_amd.data.providers import generic_ranking_provider as G
    N, H, W, P, R, seed = (int(v) for v in gold["shape"])
    gts = _gts8(gold)
    imgs = np.random.default_rng(1).random((N, H, W, 3), dtype=np.float32)
    config = {"DATA": {"CACHE_PATH_PREFIX": str(tmp_path)}}
    mp = _Params(dataset="SINTEL", val_rankings_per_img=P)
    prov = G.GenericHourglassPairRelationDataProvider(mp, seed, bool(inv), threshold=0.03,
                                                      save_pairs_on_disk=True, config=config)
    ds = prov.provide_test_dataset((imgs, gts))
    want = gold[f"pairs_inv{inv}"]
    assert ds.targets.is_cuda and ds.images.is_cuda and len(ds) == N
    assert np.array_equal(ds.targets.cpu().numpy(), want)
    assert np.random.randint(1 << 30) == gold[f"pairs_inv{inv}_next"]
    x, y = ds.batch(2)[0]
    assert len(ds.batch(2)) == 1 and tuple(x.shape) == (2, H, W, 3) and tuple(y.shape) == (2, P, 5)
    img0, tab0 = next(iter(ds))
    assert np.array_equal(img0.cpu().numpy(), imgs[0]) and np.array_equal(tab0.cpu().numpy(),
                                                                          want[0])
    # the reference's file name; a list of (img, gt) pairs reads it back instead of redrawing
    path = tmp_path / "ordinal_pair_cache" / f"SINTEL_{P}_{seed}.npy"
    assert np.array_equal(np.load(path), want)
    marked = want.copy()
    marked[:, :, 3] += 1.0
    np.save(path, marked)
    again = prov.provide_test_dataset(list(zip(imgs, gts)))
    assert np.array_equal(again.targets.cpu().numpy(), marked)
    val = prov.provide_val_dataset((imgs, gts))
    assert np.array_equal(val.targets.cpu().numpy(), want)
    assert (tmp_path / "ordinal_pair_cache" / f"SINTEL_val_{P}_{seed}.npy").exists()


# ------------------------------------------------------------------ rankings
@pytest.mark.parametrize("inv", [0, 1])
@pytest.mark.parametrize("L", [5, 40])
def test_rankings_kernel_against_golden(cuda, gold, L, inv):
    from pldepth_amd import kernels as K
    draws = gold[f"rank_draws_L{L}"]
    got = K.depth_rankings(_dev(gold["gts_cont"], cuda), draws, bool(inv)).cpu().numpy()
    assert np.array_equal(got, gold[f"rank_cont_L{L}_inv{inv}"])
    gts = _gts8(gold)
    got = K.depth_rankings(_dev(gts, cuda), draws, bool(inv)).cpu().numpy()
    assert tie_groups_equal(got, gold[f"rank_q8_L{L}_inv{inv}"])
    # this build's tie rule, exactly
    assert np.array_equal(got, ER.depth_rankings(gts, draws, bool(inv)))


@pytest.mark.parametrize("L,R", [(1, 3), (63, 7), (64, 5)])
def test_rankings_kernel_list_sizes(cuda, L, R):
    """The shortest and the longest list, and list counts that do not fill the last workgroup;
    few depth levels, so every long list has ties; a NaN sorts last in ascending order."""
    from pldepth_amd import kernels as K
    rng = np.random.default_rng(L)
    n, hw = 3, 500
    gts = (rng.integers(0, 16, (n, hw)) / 15).astype(np.float32)
    gts[1, 7] = np.nan
    idx = rng.integers(0, hw, (n, R, L))
    idx[1, 0, 0] = 7
    for inv in (False, True):
        got = K.depth_rankings(_dev(gts, cuda), idx, inv).cpu().numpy()
        want = ER.depth_rankings(gts, idx, inv)
        assert np.array_equal(got, want, equal_nan=True), (L, R, inv)


def test_ranking_provider(cuda, gold, tmp_path):
    from pldepth_amd.data.providers import generic_ranking_provider as G
    N, H, W, P, R, seed = (int(v) for v in gold["shape"])
    imgs = np.zeros((N, H, W, 3), np.float32)
    mp = _Params(dataset="TUM", val_rankings_per_img=P)
    prov = G.GenericHourglassRankingDataProvider(mp, 5, seed, True)
    np.random.seed(seed)
    got = prov.generate_rankings((imgs, gold["gts_cont"]), invert_relation_sign=True,
                                 val_rankings_per_img=R)
    assert got.dtype == np.float32 and np.array_equal(got, gold["rank_cont_L5_inv1"])
    assert np.random.randint(1 << 30) == gold["rank_cont_L5_inv1_next"]
    config = {"DATA": {"CACHE_PATH_PREFIX": str(tmp_path)}}
    prov = G.GenericHourglassRankingDataProvider(mp, 5, seed, False, save_rankings_on_disk=True,
                                                 config=config)
    ds = prov.provide_test_dataset((imgs, gold["gts_cont"][..., None]))
    assert tuple(ds.targets.shape) == (N, 100, 5, 2) and ds.targets.is_cuda
    assert np.array_equal(ds.targets.cpu().numpy()[:, :R][0], gold["rank_cont_L5_inv0"][0])
    assert np.array_equal(np.load(tmp_path / "ranking_cache" / f"TUM_100_{seed}_5.npy"),
                          ds.targets.cpu().numpy())


# ------------------------------------------------------------------ ordinal pair error
def test_pair_error_kernel(cuda, gold):
    from pldepth_amd import kernels as K
    from pldepth_amd.active_learning.metrics import ordinal_pair_error
    gts = _gts8(gold)
    N, H, W = gts.shape
    rng = np.random.default_rng(9)
    # 700 pairs per image: more than one pass of the workgroup over the table
    coords = rng.integers(0, [H, W, H, W], (N, 700, 4))
    for inv in (False, True):
        pairs = ER.ordinal_pairs(gts, coords, 0.03, inv)
        pred = (rng.integers(0, 8, (N, H, W)) / 7).astype(np.float32)  # many exact ties
        pred[0, 5, 5] = np.nan
        pairs[0, 0, :2] = 5 * W + 5, 0  # a NaN prediction in a counted pair
        pairs[0, 0, 2] = 1.0
        for tau in (None, 0.03, 0.25):
            w, c = K.ordinal_pair_error(_dev(pred, cuda), _dev(pairs, cuda), tau, inv)
            wr, cr = ER.ordinal_pair_error(pred, pairs, tau, inv)
            assert np.array_equal(w.cpu().numpy(), wr) and np.array_equal(c.cpu().numpy(), cr)
        assert 0 < wr.sum() < cr.sum()
        sign = -1.0 if inv else 1.0
        err, per, counted = ordinal_pair_error(sign * gts, None, gold[f"pairs_inv{int(inv)}"])
        assert err == 0.0 and not per.any()
        assert counted.sum() == (gold[f"pairs_inv{int(inv)}"][..., 2] != 0).sum()
        err, per, _ = ordinal_pair_error(-sign * gts[..., None], None,
                                         gold[f"pairs_inv{int(inv)}"])
        assert err == 1.0 and (per == 1.0).all()
        err2, _, c2 = ordinal_pair_error(sign * gts, None, gold[f"pairs_inv{int(inv)}"],
                                         threshold=0.5, invert=inv)
        assert err2 == 0.0 and 0 < c2.sum() < counted.sum()


# ------------------------------------------------------------------ anti-aliased resize
def _assert_one_ulp(got, ref64):
    """One final rounding of a double accumulation: within one float32 ulp of the float64 value."""
    assert got.dtype == np.float32 and got.shape == ref64.shape
    ulp = np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - ref64)
    print("max error / ulp", float(np.max(err / ulp)))
    assert np.all(err <= ulp)


@pytest.mark.parametrize("k,shape", [(0, (16, 24)), (1, (16, 16)), (2, (16, 24)), (3, (16, 24))])
def test_resize_antialias_against_golden(cuda, gold, k, shape):
    from pldepth_amd import kernels as K
    x = gold[f"resize{k}_in"]
    got = K.resize_antialias(_dev(x[None], cuda), *shape).cpu().numpy()
    _assert_one_ulp(got[0], gold[f"resize{k}_out"])


def test_resize_antialias_batch_and_blocks(cuda):
    """Several images, more than one workgroup, a blur radius beyond the image's side."""
    from pldepth_amd import kernels as K
    x = np.random.default_rng(2).random((3, 9, 70, 2), dtype=np.float32)
    got = K.resize_antialias(_dev(x, cuda), 1, 200).cpu().numpy()
    assert len(K.antialias_taps(9, 1)) - 1 > 9
    _assert_one_ulp(got, ER.resize_antialias(x, 1, 200))
    got = K.resize_antialias(_dev(x, cuda), 20, 5).cpu().numpy()
    _assert_one_ulp(got, ER.resize_antialias(x, 20, 5))


# ------------------------------------------------------------------ DAOs
def _png(path, a):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(a).save(path)


def _u8(rng, *shape):
    return rng.integers(0, 256, shape, dtype=np.uint8)


def test_sintel_dao(cuda, tmp_path):
    from pldepth_amd import kernels as K
    from pldepth_amd.data.dao.sintel import SintelTFDataAccessObject
    rng = np.random.default_rng(0)
    rel = ["b_scene/frame_0002.png", "a_scene/frame_0001.png", "b_scene/frame_0001.png"]
    rgb = {r: _u8(rng, 20, 30, 3) for r in rel}
    dep = {r: _u8(rng, 20, 30) for r in rel}
    for r in rel:
        _png(str(tmp_path / "images" / r), rgb[r])
        _png(str(tmp_path / "depth_viz" / r), dep[r])
    imgs, gts = SintelTFDataAccessObject(str(tmp_path), [16, 24, 3]).get_test_dataset(zip_ds=False)
    assert imgs.shape == (3, 16, 24, 3) and gts.shape == (3, 16, 24)
    assert imgs.dtype == gts.dtype == np.float32
    for i, r in enumerate(sorted(rel)):
        x = rgb[r].astype(np.float32) / np.float32(255)
        g = (dep[r].astype(np.float32) / np.float32(255))[..., None] * np.float32(255)
        assert np.array_equal(imgs[i], K.resize(_dev(x[None], cuda), 16, 24).cpu().numpy()[0])
        assert np.array_equal(gts[i], K.resize(_dev(g[None], cuda), 16, 24).cpu().numpy()[0, ..., 0])
    assert 0 <= imgs.min() and imgs.max() <= 1 and 1 < gts.max() <= 255.01
    pairs = SintelTFDataAccessObject(str(tmp_path), [16, 24]).get_test_dataset()
    assert len(pairs) == 3 and np.array_equal(pairs[2][1], gts[2])


def test_diode_dao(cuda, tmp_path):
    from pldepth_amd import kernels as K
    from pldepth_amd.data.dao.diode import DIODETFDataAccessObject
    rng = np.random.default_rng(1)
    rel = ["outdoor/scene_2/scan_1/b.png", "indoors/scene_1/scan_9/a.png"]
    rgb = {r: _u8(rng, 30, 44, 3) for r in rel}
    dep = {r: (rng.random((30, 44, 1)) * 50).astype(np.float32) for r in rel}
    for r in rel:
        _png(str(tmp_path / r), rgb[r])
        np.save(str(tmp_path / r).replace(".png", "_depth.npy"), dep[r])
    imgs, gts = DIODETFDataAccessObject(str(tmp_path), [16, 16, 3]).get_test_dataset(zip_ds=False)
    assert imgs.shape == (2, 16, 16, 3) and gts.shape == (2, 16, 16)
    for i, r in enumerate(sorted(rel)):
        x = rgb[r].astype(np.float32) / np.float32(255)
        assert np.array_equal(imgs[i], K.resize(_dev(x[None], cuda), 16, 16).cpu().numpy()[0])
        want = K.resize_antialias(_dev(dep[r][None], cuda), 16, 16).cpu().numpy()[0, ..., 0]
        assert np.array_equal(gts[i], want)
        _assert_one_ulp(gts[i], ER.resize_antialias(dep[r], 16, 16)[..., 0])
    assert 0 < gts.min() and gts.max() < 50


def test_tum_dao(cuda, tmp_path):
    from pldepth_amd import kernels as K
    from pldepth_amd.data.dao.tum import TUMTFDataAccessObject
    from pldepth_amd.util import hdf5
    rng = np.random.default_rng(2)
    data = {}
    for name in ("f2.h5", "f1.h5"):
        root = hdf5.Group()
        img, dep = rng.random((24, 36, 3), dtype=np.float32), rng.random((24, 36), dtype=np.float32)
        root.create_dataset("gt/img_1", img)
        root.create_dataset("gt/pp_depth", dep)
        root.create_dataset("gt/depth", dep + 1)  # not the field the DAO reads
        hdf5.save(str(tmp_path / name), root)
        data[name] = (img, dep)
    imgs, gts = TUMTFDataAccessObject(str(tmp_path), [16, 24, 3]).get_test_dataset(zip_ds=False)
    assert imgs.shape == (2, 16, 24, 3) and gts.shape == (2, 16, 24)
    for i, name in enumerate(sorted(data)):
        img, dep = data[name]
        assert np.array_equal(imgs[i],
                              K.resize_antialias(_dev(img[None], cuda), 16, 24).cpu().numpy()[0])
        _assert_one_ulp(gts[i], ER.resize_antialias(dep[..., None], 16, 24)[..., 0])
    assert 0 <= gts.min() and gts.max() <= 1


def test_ibims_dao(cuda, tmp_path):
    sio = pytest.importorskip("scipy.io")
    from pldepth_amd.data.dao.ibims import IbimsTFDataAccessObject
    rng = np.random.default_rng(3)
    data = {}
    for name in ("room_b.mat", "room_a.mat"):
        rgb, dep = _u8(rng, 30, 40, 3), (rng.random((30, 40)) * 10).astype(np.float32)
        sio.savemat(str(tmp_path / name), {"data": {"scene": name, "calib": np.eye(3), "rgb": rgb,
                                                    "depth": dep}})
        data[name] = (rgb, dep)
    dao = IbimsTFDataAccessObject(str(tmp_path), [16, 24, 3])
    assert [os.path.basename(f) for f in dao.file_names] == sorted(data)
    imgs, gts = dao.get_test_dataset(zip_ds=False)
    assert imgs.shape == (2, 16, 24, 3) and gts.shape == (2, 16, 24)
    for i, name in enumerate(sorted(data)):
        rgb, dep = data[name]
        x = rgb.astype(np.float32) / np.float32(255)
        _assert_one_ulp(imgs[i], ER.resize_antialias(x, 16, 24))
        _assert_one_ulp(gts[i], ER.resize_antialias(dep[..., None], 16, 24)[..., 0])
    assert 0 <= imgs.min() and imgs.max() <= 1 and 0 <= gts.min() and gts.max() <= 10


# ------------------------------------------------------------------ command line
def _run_cli(args):
    from click.testing import CliRunner
    from pldepth_amd.test_data_eval import eval_model
    res = CliRunner().invoke(eval_model, args)
    assert res.exit_code == 0, (res.output, res.exception)
    out = {}
    for line in res.output.splitlines():
        parts = line.split()
        if len(parts) == 2 and parts[0].replace("_", "").isalnum() and parts[0][0].isalpha():
            out[parts[0]] = float(parts[1])
    return out


def test_eval_model_cli(cuda, tmp_path):
    base = ["--model_name", "ff_effnet", "--input_size", "64", "--batch_size", "2", "--seed", "5",
            "--dataset", "sintel", "--val_rankings_per_img", "40"]
    first = _run_cli(base)
    print(first)
    # 64 x 64 images: the two metrics that draw from at least 10,000 / 224 x 224 pixels are left
    # out, as in the training entry point's test pass
    assert set(first) == {"ordinal_pair_error", "ranking_loss", "depth_boundary_metric",
                          "depth_completeness"}
    assert all(np.isfinite(v) for v in first.values()), first
    assert 0 <= first["ordinal_pair_error"] <= 1
    second = _run_cli(base + ["--cache", str(tmp_path)])
    assert second["ordinal_pair_error"] == first["ordinal_pair_error"]
    assert second["ranking_loss"] == first["ranking_loss"]
    assert (tmp_path / "ordinal_pair_cache" / "SINTEL_40_5.npy").exists()
    assert (tmp_path / "ranking_cache" / "SINTEL_100_5_5.npy").exists()


# ------------------------------------------------------------------ host checks
def test_arguments_are_checked_before_any_launch(cuda):
    import torch
    from pldepth_amd import kernels as K
    from pldepth_amd._lib import PLDError, lib
    gt = torch.zeros((2, 8, 12), device=cuda)
    ok = np.zeros((2, 3, 4), np.int64)
    for bad in ([8, 0, 0, 0], [0, 12, 0, 0], [0, 0, -1, 0], [0, 0, 0, 12]):
        c = ok.copy()
        c[1, 2] = bad
        with pytest.raises(ValueError, match="outside a map of 8 x 12"):
            K.ordinal_pairs(gt, c)
    K.ordinal_pairs(gt, ok + [7, 11, 7, 11])  # the last pixel is inside
    idx = np.zeros((2, 3, 5), np.int64)
    idx[0, 1, 4] = 96
    with pytest.raises(ValueError, match="index 96 outside an image of 96 pixels"):
        K.depth_rankings(gt, idx)
    idx[0, 1, 4] = -1
    with pytest.raises(ValueError, match="index -1 outside"):
        K.depth_rankings(gt, idx)
    with pytest.raises(PLDError, match=f"above the limit of {K.RANKING_MAX_L}"):
        K.depth_rankings(gt, np.zeros((2, 1, K.RANKING_MAX_L + 1), np.int64))
    K.depth_rankings(gt, np.zeros((2, 1, K.RANKING_MAX_L), np.int64))
    assert K.RANKING_MAX_L >= 64
    # 2^24 pixels are the most a float32 index column can address: the wrappers refuse more
    # from the shapes alone, and so do the entry points
    big = torch.empty((1, 1), device=cuda).expand(1, (1 << 24) + 1)
    with pytest.raises(ValueError, match="16777217 pixels"):
        K.depth_rankings(big, np.zeros((1, 1, 2), np.int64))
    with pytest.raises(ValueError, match="16777217 pixels"):
        K.ordinal_pair_error(big, torch.zeros((1, 1, 5), device=cuda))
    p = K.ptr(gt)
    with pytest.raises(PLDError, match="2\\^24"):
        lib().pld_depth_rankings(p, 1, (1 << 24) + 1, p, 1, 2, 0, p, None)
    with pytest.raises(PLDError, match="2\\^24"):
        lib().pld_ordinal_pairs(p, 1, 4097, 4096, p, 1, 0.03, 0, p, None)
    with pytest.raises(PLDError, match="2\\^24"):
        lib().pld_ordinal_pair_error(p, 1, (1 << 24) + 1, p, 1, 0.0, 0, 0, p, p, None)
    with pytest.raises(PLDError, match="null pointer"):
        lib().pld_resize_antialias(None, 1, 4, 4, 1, 2, 2, p, 0, p, 0, p, None)
    torch.cuda.synchronize()
