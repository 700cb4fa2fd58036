"""Active-learning selection on the GPU: every entry point of pldepth_amd/csrc/active.hip
against the NumPy yardstick (tests/al_ref.py) with exact equality, against the reference's
recorded results (tests/golden/active_golden.npz) under the tie waiver described in
tests/test_active.py, then the reference-shaped API and one active round end to end.

Without the feature nothing here passes: the symbols and the ``active_learning_method`` module do
not exist, and the second ``fit`` of the end-to-end test raises ``ranking count changed after
graph capture``."""
import os
import warnings

import numpy as np
import pytest

import al_ref as A
import edge_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


@pytest.fixture(scope="module")
def ag():
    return np.load(os.path.join(ROOT, "tests", "golden", "active_golden.npz"))


def _fixtures():
    """The golden fixtures with their yardstick tile tables, computed once."""
    if "fx" not in _CACHE:
        _CACHE["fx"] = [(a, b, s, A.hausdorff_table(a, b, s)) for a, b, s in A.fixtures()]
    return _CACHE["fx"]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- image operators
def test_gray(cuda):
    from pldepth_amd import kernels as K
    rng = np.random.default_rng(1)
    rgb = rng.random((3, 20, 33, 3), dtype=np.float32) * np.float32(255)
    got = K.gray(_cuda(rgb)).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, A.gray(rgb))
    # as the pipeline consumes it: the 8-bit map after the min-max scaling
    u8 = K.minmax_u8(K.gray(_cuda(rgb))).cpu().numpy()
    assert np.array_equal(u8, np.stack([R.minmax_u8(A.gray(x)) for x in rgb]))


@pytest.mark.parametrize("h,w,ksize", [(20, 33, 3), (20, 33, 15), (64, 64, 15), (5, 5, 7)])
def test_median_blur(cuda, h, w, ksize):
    """20 x 33 with ksize 15: the window is wider than the map's margin everywhere; 33 columns
    leave a second, partly filled 32-wide tile."""
    from pldepth_amd import kernels as K
    rng = np.random.default_rng(h + ksize)
    img = rng.integers(0, 256, (3, h, w)).astype(np.uint8)
    img[1] = (img[1] // 64) * 64  # few levels: many equal values around the median
    img[2, :, : w // 2] = 255
    got = K.median_blur(_cuda(img), ksize).cpu().numpy()
    assert np.array_equal(got, np.stack([A.median_blur(x, ksize) for x in img]))


def test_unsharp(cuda, ag):
    from pldepth_amd import kernels as K
    rng = np.random.default_rng(2)
    batch = np.stack([A.fixture_depths(0)[1][:40, :56], np.full((40, 56), -2.5, np.float32),
                      rng.standard_normal((40, 56)).astype(np.float32) * 30])
    cases = [batch, rng.random((1, 5, 5), dtype=np.float32), np.full((1, 9, 7), 3.0, np.float32),
             A.fixture_depths(4)[1][None], A.fixture_depths(1)[0][None]]
    for x in cases:
        got = K.unsharp(_cuda(x)).cpu().numpy()
        want = np.stack([A.unsharp_u8(a) for a in x])
        assert got.dtype == np.uint8 and np.array_equal(got, want), x.shape
    assert not K.unsharp(_cuda(cases[2])).any()  # a constant map scales to 0
    got = K.unsharp(_cuda(batch), sigma=1.8, amount=1.5).cpu().numpy()
    assert np.array_equal(got, np.stack([A.unsharp_u8(a, 1.8, 1.5) for a in batch]))
    # the reference's unsharp_mask on maps already in 0..255, through its import path
    from pldepth.active_learning.preprocess_utils import unsharp_mask
    for k in range(2):
        got = unsharp_mask(ag[f"u{k}_x"])
        assert isinstance(got, np.ndarray) and np.array_equal(got, ag[f"u{k}_sharp"]), k


# ---------------------------------------------------------------- tiles
def test_tile_hausdorff_every_fixture(cuda, ag):
    from pldepth_amd import kernels as K
    for f, (e_in, e_pred, split, want) in enumerate(_fixtures()):
        got = K.tile_hausdorff(_cuda(e_in[None]), _cuda(e_pred[None]), split).cpu().numpy()[0]
        assert got.dtype == np.int32 and np.array_equal(got, want), f
        A.check_table(got, e_in, e_pred, split, ag[f"f{f}_hd2"], ag[f"f{f}_pair"])
        assert (got[:, 7] >= 0).sum() == ag[f"f{f}_tied"][1]


def test_tile_hausdorff_batches(cuda):
    """n > 1 with different content per image: the two hand-made pairs (tiles of 32) in one call,
    and three maps of 7-pixel tiles (a tile count that is no multiple of the tiles per
    workgroup: 3 * 81 = 243)."""
    from pldepth_amd import kernels as K
    a, b = A.handmade_edges()
    got = K.tile_hausdorff(_cuda(a), _cuda(b), 2).cpu().numpy()
    assert np.array_equal(got, np.stack([A.hausdorff_table(x, y, 2) for x, y in zip(a, b)]))
    assert got[0, 3].tolist() == [23 * 23 + 18 * 18, 8, 18, 31, 0, 1, 1024, 0]
    assert got[1, 1].tolist() == [21 * 21 + 21 * 21, 31, 0, 10, 21, 1024, 1, 1]
    e_in, e_pred = A.fixture_edges(4)
    a = np.stack([e_in[:63, :63], e_pred[:63, :63], e_in[40:103, 30:93]])
    b = np.stack([e_pred[:63, :63], e_in[1:64, :63], np.zeros((63, 63), np.uint8)])
    got = K.tile_hausdorff(_cuda(a), _cuda(b), 9).cpu().numpy()
    assert np.array_equal(got, np.stack([A.hausdorff_table(x, y, 9) for x, y in zip(a, b)]))
    # any non-zero value marks an edge
    got1 = K.tile_hausdorff(_cuda(a // 255), _cuda(b // 255 * 3), 9).cpu().numpy()
    assert np.array_equal(got1, got)


def test_tile_nth_edge(cuda):
    import torch
    from pldepth_amd import kernels as K
    e_in, _, split, table = _fixtures()[2]
    maps = np.stack([e_in, np.roll(e_in, 5, axis=0)])
    n_in = np.stack([table[:, 5], A.hausdorff_table(maps[1], maps[1], split)[:, 5]])
    tiles = [A.split_image(m, split) for m in maps]
    k = np.full((2, split * split), -1, np.int32)
    have = [np.nonzero(n > 2)[0] for n in n_in]
    assert len(have[0]) >= 4 and len(have[1]) >= 4
    for im in range(2):
        t0, t1, t2, t3 = have[im][:4]
        k[im, t0] = 0
        k[im, t1] = n_in[im][t1] - 1
        k[im, t2] = n_in[im][t2] // 2
        k[im, t3] = n_in[im][t3]       # one past the last: (-1, -1), nothing read
    empty = int(np.nonzero(n_in[0] == 0)[0][0])
    k[0, empty] = 0                    # a tile without edges
    rc = torch.full((2, split * split, 2), -7, dtype=torch.int32, device="cuda")
    got = K.tile_nth_edge(_cuda(maps), split, _cuda(k), rc).cpu().numpy()
    for im in range(2):
        for t in range(split * split):
            want = (-7, -7) if k[im, t] < 0 else A.nth_edge(tiles[im][t], int(k[im, t]))
            assert tuple(got[im, t]) == want, (im, t, k[im, t])
    assert (got == -7).sum() == 2 * (k < 0).sum() and tuple(got[0, empty]) == (-1, -1)
    # every pixel of a full 32 x 32 tile
    full = np.full((1, 32, 32), 9, np.uint8)
    for kk in (0, 31, 32, 1023):
        rc = torch.full((1, 1, 2), -7, dtype=torch.int32, device="cuda")
        got = K.tile_nth_edge(_cuda(full), 1, _cuda(np.array([[kk]], np.int32)), rc)
        assert got[0, 0].tolist() == [kk // 32, kk % 32]


def test_al_oracle(cuda, ag):
    from pldepth_amd import kernels as K
    for f, (e_in, _, _, _) in enumerate(_fixtures()):
        h = e_in.shape[0]
        gt = np.random.default_rng(900 + f).random((h, h)).astype(np.float32)
        for L in (3, 4):  # P = 16, 64, 64, 36, 256, 4, 4: L divides P and does not
            np.random.seed(11 + L)
            pxy = ag[f"f{f}_pts"].astype(np.int32)
            np.random.shuffle(pxy)
            got = K.al_oracle(_cuda(gt[None]), _cuda(pxy[None]), L, h).cpu().numpy()[0]
            assert got.dtype == np.float32 and np.array_equal(got, ag[f"f{f}_oracle{L}"]), (f, L)
    # equal depths (5 levels), L up to the limit, a batch of 3 with different points
    rng = np.random.default_rng(5)
    gt = (np.floor(rng.random((3, 24, 24)) * 5) / 4).astype(np.float32)
    pxy = rng.integers(0, 24, (3, 50, 2)).astype(np.int32)
    for L in (2, 7, 16):
        got = K.al_oracle(_cuda(gt), _cuda(pxy), L, 31).cpu().numpy()
        want = np.stack([A.oracle_rows(g, p, L, 31) for g, p in zip(gt, pxy)])
        assert np.array_equal(got, want), L
    assert K.al_oracle(_cuda(gt), _cuda(pxy[:, :5]), 7, 31).shape == (3, 0, 7, 2)


def test_limits_are_errors(cuda):
    """Past a limit: PLD_ERR_UNSUPPORTED (3) and nothing is launched."""
    import torch
    from pldepth_amd import _lib
    from pldepth_amd import kernels as K
    assert (K.TILE_MAX, K.MEDIAN_MAX_KSIZE, K.ORACLE_MAX_L) == (32, 15, 16)
    lib = _lib.lib()
    for h, w, split in ((66, 66, 2), (64, 48, 2), (64, 64, 3)):  # tile 33, h != w, h % split
        e = torch.zeros((1, h, w), dtype=torch.uint8, device="cuda")
        out = torch.full((1, split * split, 8), 7, dtype=torch.int32, device="cuda")
        k = torch.zeros((1, split * split), dtype=torch.int32, device="cuda")
        rc = torch.full((1, split * split, 2), 7, dtype=torch.int32, device="cuda")
        with pytest.raises(_lib.PLDError, match=r"pld_tile_hausdorff failed \(3\)"):
            lib.pld_tile_hausdorff(K.ptr(e), K.ptr(e), 1, h, w, split, K.ptr(out), K.stream())
        with pytest.raises(_lib.PLDError, match=r"pld_tile_nth_edge failed \(3\)"):
            lib.pld_tile_nth_edge(K.ptr(e), 1, h, w, split, K.ptr(k), K.ptr(rc), K.stream())
        torch.cuda.synchronize()
        assert bool((out == 7).all()) and bool((rc == 7).all())
    img = torch.zeros((1, 40, 40), dtype=torch.uint8, device="cuda")
    out = torch.full((1, 40, 40), 7, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.PLDError, match=r"\(3\).*limit of 15"):
        lib.pld_median_blur_u8(K.ptr(img), 1, 40, 40, 17, K.ptr(out), K.stream())
    with pytest.raises(_lib.PLDError, match=r"\(1\)"):
        lib.pld_median_blur_u8(K.ptr(img), 1, 40, 40, 4, K.ptr(out), K.stream())
    gt = torch.zeros((1, 8, 8), device="cuda")
    pxy = torch.zeros((1, 40, 2), dtype=torch.int32, device="cuda")
    y = torch.full((1, 2, 17, 2), 7.0, device="cuda")
    with pytest.raises(_lib.PLDError, match=r"\(3\).*limit of 16"):
        lib.pld_al_oracle(K.ptr(gt), 1, 8, 8, K.ptr(pxy), 40, 17, 8, K.ptr(y), K.stream())
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((y == 7).all())
    # the largest supported tile runs
    e = torch.zeros((2, 64, 64), dtype=torch.uint8, device="cuda")
    e[0, 0, 0] = e[1, 0, 31] = 255
    t = K.tile_hausdorff(e[:1], e[1:], 2)[0].tolist()
    assert t[0] == [31 * 31, 0, 0, 0, 31, 1, 1, 0] and t[1] == [0, -1, -1, -1, -1, 0, 0, -1]


# ---------------------------------------------------------------- the reference's API
def test_api_matches_reference(cuda, ag):
    """active_sampling, oracle, hausdorff_pair and hausdorf_dist through the reference's import
    path. active_sampling equals the yardstick element for element (both sort stably and share
    the lowest-index rule; the yardstick with the reference's pick on the waived tiles equals the
    golden as a multiset, tests/test_active.py), its statistics and the RNG state equal the
    reference's."""
    from pldepth.active_learning.active_learning_method import (active_sampling, get_edge_pixel,
                                                                oracle)
    from pldepth.active_learning.metrics import hausdorf_dist, hausdorff_pair
    for f, (e_in, e_pred, split, _) in enumerate(_fixtures()):
        h = e_in.shape[0]
        np.random.seed(7)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            pos, pts, mean, var = active_sampling(e_in, e_pred, split, [h, h, 3])
        st = np.random.get_state()
        assert np.array_equal(st[1], ag[f"f{f}_rng"]) and st[2] == int(ag[f"f{f}_rng_pos"]), f
        assert [mean, var] == ag[f"f{f}_stat"].tolist(), f
        np.random.seed(7)
        want = A.active_sampling(e_in, e_pred, split, [h, h, 3])
        assert pos.dtype == np.uint32 and pts.dtype == np.uint32
        assert np.array_equal(pos, want[0]) and np.array_equal(pts, want[1]), f
        if not A.waived_tiles(e_in, e_pred, split, ag[f"f{f}_pair"]):
            assert np.array_equal(A.multiset(pos, pts),
                                  A.multiset(ag[f"f{f}_pos"], ag[f"f{f}_pts"])), f
        gt = np.random.default_rng(900 + f).random((h, h)).astype(np.float32)
        for L in (3, 4):
            np.random.seed(11 + L)
            pxy = ag[f"f{f}_pts"].copy()
            got = oracle(None, gt[..., None], pxy, L, [h, h, 3])
            assert got.dtype == np.float32 and np.array_equal(got, ag[f"f{f}_oracle{L}"]), (f, L)
            assert np.random.get_state()[2] == int(ag[f"f{f}_oracle{L}_rng_pos"])
            assert not np.array_equal(pxy, ag[f"f{f}_pts"])  # shuffled in place
    # per-tile helpers on the 16-pixel tiles of fixture 0 and the hand-made 32-pixel tiles
    for f in (0, 5, 6):
        e_in, e_pred, split, _ = _fixtures()[f]
        si, sp = A.split_image(e_in, split), A.split_image(e_pred, split)
        rows = []
        for i in range(len(si)):
            d = hausdorf_dist(si[i], sp[i])
            hd2 = int(ag[f"f{f}_hd2"][i])
            assert (np.isinf(d) if hd2 < 0 else d == np.sqrt(float(hd2))), (f, i, d)
            if hd2 < 0:
                with pytest.warns(UserWarning, match="empty"):
                    assert hausdorff_pair(si[i], sp[i]) == ((), ())
                rows.append([hd2, -1, -1, -1, -1])
            elif (si[i] != 0).any():
                pa, pb = hausdorff_pair(si[i], sp[i])
                rows.append([hd2, pa[0], pa[1], pb[0], pb[1]])
            else:
                assert d == 0 and isinstance(d, int)
                rows.append([0, -1, -1, -1, -1])
        A.check_table(np.array(rows), e_in, e_pred, split, ag[f"f{f}_hd2"], ag[f"f{f}_pair"])
    tile = A.split_image(_fixtures()[0][0], 4)[5]
    np.random.seed(3)
    got = get_edge_pixel(tile)
    np.random.seed(3)
    idx = np.nonzero(tile)
    i = np.random.choice(idx[0].shape[0])
    assert got == (idx[0][i], idx[1][i])
    assert get_edge_pixel(np.zeros((7, 7), np.uint8)) == (3.5, 3.5)


# ---------------------------------------------------------------- one active round
def test_active_round_end_to_end(cuda):
    """ff_effnet at 64 x 64, B = 2: two steps on the ordinary provider (captured at R = 20), the
    active provider's rankings against the yardstick fed model.predict's maps under the same
    seed (P = 16 points, L = 3: 5 rankings per image), two steps on them (the ranking count
    changes under the captured step), and one ordinary step again."""
    import torch
    from pldepth.active_learning.active_learning_method import active_learning_data_provider
    from pldepth_amd.data.providers.hourglass_provider import HourglassLargeScaleDataProvider
    from pldepth_amd.data.sampling import InformationScoreBasedSampling
    from pldepth_amd.losses.losses_meta import DepthLossType
    from pldepth_amd.losses.nll_loss import HourglassNegativeLogLikelihood
    from pldepth_amd.models.models_meta import ModelParameters, get_model_type_by_name
    from pldepth_amd.models.PLDepthNet import get_pl_depth_net
    from pldepth_amd.optimizers import Adam
    from pldepth_amd.PLDepth import synthetic_hrwsi
    from pldepth_amd.run_scripts.active_PLDepth import run_active_rounds
    B, H, L, Rk, split = 2, 64, 3, 20, 4
    mp = ModelParameters()
    mp.set_parameter("model_type", get_model_type_by_name("ff_effnet"))
    mp.set_parameter("ranking_size", L)
    mp.set_parameter("rankings_per_image", Rk)
    mp.set_parameter("val_rankings_per_img", Rk)
    mp.set_parameter("batch_size", B)
    mp.set_parameter("loss_type", DepthLossType.NLL)
    mp.set_parameter("seed", 0)
    mp.set_parameter("sampling_strategy", InformationScoreBasedSampling(mp))
    model, pre = get_pl_depth_net(mp, [H, H, 3])
    model.compile(loss=HourglassNegativeLogLikelihood(L, B), optimizer=Adam(0.01, amsgrad=True))
    imgs, gts, masks = synthetic_hrwsi(4, H, H, seed=0)
    pool_imgs, pool_gts, _ = synthetic_hrwsi(6, H, H, seed=1)
    prov = HourglassLargeScaleDataProvider(mp, masks, masks[:2], augmentation=False)
    train = prov.provide_train_dataset(pre(imgs), gts)
    model.fit(x=train, epochs=1, steps_per_epoch=2, verbose=0)
    assert model.trainer.graphs is not None and model.trainer.R_out == Rk

    np.random.seed(21)
    ds = active_learning_data_provider(pool_imgs, pool_gts[..., None], model, batch_size=B,
                                       ranking_size=L, split_num=split, img_size=[H, H, 3])
    end_state = np.random.get_state()
    preds = model.predict(pool_imgs)
    np.random.seed(21)
    want, means = [], []
    for img, gt, pred in zip(pool_imgs, pool_gts, preds):
        e_in = R.auto_canny(A.median_blur(R.minmax_u8(A.gray(img)), 15))
        e_pred = R.auto_canny(A.unsharp_u8(pred[..., 0]), 1.8)
        _, pts, m, _ = A.active_sampling(e_in, e_pred, split, [H, H, 3])
        want.append(A.oracle(gt, pts, L, [H, H, 3]))
        means.append(m)
    assert np.array_equal(np.random.get_state()[1], end_state[1])
    assert np.random.get_state()[2] == end_state[2]
    assert len(ds) == 3 and ds.hd_mean == means and len(ds.hd_var) == 6
    batches = [b for b, _ in zip(iter(ds), range(3))]
    y = torch.cat([yb for _, yb in batches]).cpu().numpy()
    assert y.shape == (6, 16 // L, L, 2) and np.array_equal(y, np.stack(want))
    assert all(xb.is_cuda and tuple(xb.shape) == (B, H, H, 3) for xb, _ in batches)
    assert np.array_equal(torch.cat([xb for xb, _ in batches]).cpu().numpy(), pool_imgs)

    w0 = model.get_weights()["dec_conv0/kernel"].copy()
    model.fit(x=ds, epochs=1, steps_per_epoch=2, verbose=0)
    assert np.isfinite(model.history["loss"]).all() and len(model.history["loss"]) == 2
    assert model.trainer.R_out == 16 // L and model.trainer.graphs is not None
    w1 = model.get_weights()["dec_conv0/kernel"].copy()
    assert not np.allclose(w0, w1)
    xb, yb = next(iter(train))  # back to the ordinary provider's 20 rankings
    assert np.isfinite(model.train_on_batch(xb, yb)) and model.trainer.R_out == Rk
    # the run script's round on arrays: the provider, one fit, and the reference's break
    np.random.seed(21)
    rounds = run_active_rounds(model, pool_imgs, pool_gts, None, batch_size=B, ranking_size=L,
                               epochs=1, split_num=split, steps_per_epoch=1, verbose=0)
    assert len(rounds) == 1 and len(rounds[0]) == 3 and model.trainer.R_out == 16 // L
    assert np.isfinite(model.history["loss"]).all()
