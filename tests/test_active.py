"""Active-learning selection, CPU side: the NumPy yardstick (tests/al_ref.py) against the
reference's own results (tests/golden/active_golden.npz), the ctypes signatures of the new entry
points, and the host-only parts of the Python surface.

Where the reference's answer depends on a library's tie order the comparison says so: the chosen
input pixel must lie in the tied set on tiles whose nearest input pixel is not unique (at most
1/6 of the tiles with edges in both maps, asserted when the golden is made), and the sorted
points are compared as a multiset."""
import os
import subprocess
import sys

import numpy as np
import pytest

import al_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pld_gray_f32", "pld_median_blur_u8", "pld_unsharp_u8_workspace_size", "pld_unsharp_u8",
       "pld_tile_hausdorff", "pld_tile_nth_edge", "pld_al_oracle"]


@pytest.fixture(scope="module")
def ag():
    return np.load(os.path.join(ROOT, "tests", "golden", "active_golden.npz"))


def test_golden_shape(ag):
    assert int(ag["n"]) == len(A.FIXTURES) + 2
    for f in range(int(ag["n"])):
        tied, both = ag[f"f{f}_tied"]
        assert both > 0 and 6 * tied <= both, (f, tied, both)


def test_yardstick_tiles_match_reference(ag):
    for f, (e_in, e_pred, split) in enumerate(A.fixtures()):
        table = A.hausdorff_table(e_in, e_pred, split)
        A.check_table(table, e_in, e_pred, split, ag[f"f{f}_hd2"], ag[f"f{f}_pair"])
        assert np.array_equal(table[:, 7] >= 0, ag[f"f{f}_pair"][:, 0] >= 0)


def test_handmade_tiles_by_hand():
    a, b = A.handmade_edges()
    t = A.hausdorff_table(a[0], b[0], 2)
    assert t[0].tolist() == [0, -1, -1, -1, -1, 0, 0, -1]            # all empty
    assert t[1].tolist() == [-1, -1, -1, -1, -1, 6, 0, -1]           # input only
    assert t[2].tolist() == [-1, -1, -1, -1, -1, 0, 28, -1]          # prediction only
    # one input pixel (8, 18) against a full tile: hBA is the far corner (31, 0)
    assert t[3].tolist() == [23 * 23 + 18 * 18, 8, 18, 31, 0, 1, 1024, 0]
    t = A.hausdorff_table(a[1], b[1], 2)
    assert t[0].tolist() == [0, 0, 0, 0, 0, 1024, 1024, 0]           # equal sets: branch 0
    assert t[1].tolist() == [21 * 21 + 21 * 21, 31, 0, 10, 21, 1024, 1, 1]
    assert t[3].tolist() == [2 * 31 * 31, 31, 31, 0, 0, 1, 1, 0]


def test_active_sampling_matches_reference(ag):
    for f, (e_in, e_pred, split) in enumerate(A.fixtures()):
        h = e_in.shape[0]
        waived = A.waived_tiles(e_in, e_pred, split, ag[f"f{f}_pair"])
        np.random.seed(7)
        pos, pts, mean, var = A.active_sampling(e_in, e_pred, split, [h, h, 3],
                                                in_override=waived)
        assert pos.dtype == np.uint32 and pts.dtype == np.uint32
        assert np.array_equal(A.multiset(pos, pts), A.multiset(ag[f"f{f}_pos"], ag[f"f{f}_pts"]))
        assert [mean, var] == ag[f"f{f}_stat"].tolist()
        st = np.random.get_state()
        assert np.array_equal(st[1], ag[f"f{f}_rng"]) and st[2] == int(ag[f"f{f}_rng_pos"])


def test_oracle_matches_reference(ag):
    for f, (e_in, _, _) in enumerate(A.fixtures()):
        h = e_in.shape[0]
        gt = np.random.default_rng(900 + f).random((h, h)).astype(np.float32)
        for L in (3, 4):
            np.random.seed(11 + L)
            pxy = ag[f"f{f}_pts"].copy()
            got = A.oracle(gt, pxy, L, [h, h, 3])
            want = ag[f"f{f}_oracle{L}"]
            assert got.dtype == np.float32 and np.array_equal(got, want), (f, L)
            assert np.random.get_state()[2] == int(ag[f"f{f}_oracle{L}_rng_pos"])
            P = len(pxy)
            if P % L == 0:
                assert not want[-1].any()  # the reference's loop bound
                assert len(want) == 1 or want[-2].any()
            else:
                assert want[-1].any()


def test_unsharp_matches_reference(ag):
    for k in range(2):
        assert np.array_equal(A.unsharp_mask(ag[f"u{k}_x"]), ag[f"u{k}_sharp"])
    taps = A.gaussian_taps(1.0)
    assert taps.dtype == np.float32 and abs(float(taps.sum()) - 1) < 1e-6 and taps[2] > taps[1]
    flat = np.full((6, 7), 93.0, np.float32)
    assert np.all(A.unsharp_mask(flat) == 93)  # taps sum to 1 within rounding: 372 - 279


def test_median_yardstick():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (9, 11)).astype(np.uint8)
    m = A.median_blur(img, 3)
    p = np.pad(img, 1, mode="edge")
    assert m[0, 0] == np.median(p[0:3, 0:3]) and m[4, 5] == np.median(img[3:6, 4:7])
    assert m[8, 10] == np.median(p[8:11, 10:13])


# ---------------------------------------------------------------- ABI and host-side surface
def test_active_signatures_load():
    from pldepth_amd import _lib
    lib = _lib.lib()
    for s in NEW:
        assert s in _lib._SIGS and callable(getattr(lib, s)), s
        assert len(getattr(lib._dll, s).argtypes) == len(_lib._SIGS[s][1])
    assert set(NEW) <= set(_lib.declared_symbols())
    hdr = open(_lib.HEADER).read()
    for macro in ("PLD_TILE_MAX 32", "PLD_MEDIAN_MAX_KSIZE 15", "PLD_ORACLE_MAX_L 16"):
        assert "#define " + macro in hdr
    assert lib.pld_unsharp_u8_workspace_size(3) == 3 * 64 * 2 * 4
    assert lib.pld_unsharp_u8_workspace_size(0) == 0
    for call in (lambda: lib.pld_gray_f32(None, 1, 8, None, None),
                 lambda: lib.pld_median_blur_u8(None, 1, 8, 8, 3, None, None),
                 lambda: lib.pld_unsharp_u8(None, 1, 8, 8, 1, 1.0, 3.0, None, None, None),
                 lambda: lib.pld_tile_hausdorff(None, None, 1, 8, 8, 1, None, None),
                 lambda: lib.pld_tile_nth_edge(None, 1, 8, 8, 1, None, None, None),
                 lambda: lib.pld_al_oracle(None, 1, 8, 8, None, 4, 2, 8, None, None)):
        with pytest.raises(_lib.PLDError, match=r"\(1\).*bad args"):
            call()


def test_split_image_and_guards():
    from pldepth.active_learning import preprocess_utils as PU
    img = np.arange(36 * 36).reshape(36, 36)
    s = PU.splitImage(img, 6)
    assert s.shape == (36, 6, 6) and np.array_equal(s, A.split_image(img, 6))
    assert np.array_equal(s[7], img[6:12, 6:12])
    with pytest.raises(ValueError):
        PU.splitImage(img, 5)
    x = np.zeros((8, 8), np.float32)
    with pytest.raises(NotImplementedError):
        PU.unsharp_mask(x, kernel_size=(3, 3))
    with pytest.raises(NotImplementedError):
        PU.unsharp_mask(x, threshold=1)


def test_import_paths_and_docstrings():
    import inspect

    import pldepth.active_learning.active_learning_method as M
    import pldepth.active_learning.metrics as AM
    import pldepth.run_scripts.active_PLDepth as RS
    assert M.__name__ == "pldepth_amd.active_learning.active_learning_method"
    for name in ("get_edge_pixel", "active_sampling", "oracle", "active_learning_data_provider",
                 "select_batch"):
        assert callable(getattr(M, name)), name
    assert list(inspect.signature(M.active_learning_data_provider).parameters) == [
        "img_arr", "img_gts_arr", "model", "batch_size", "ranking_size", "split_num", "sigma",
        "img_size"]
    assert list(inspect.signature(M.oracle).parameters) == [
        "img", "img_gts", "pos_xy", "ranking_size", "img_size"]
    assert 'kind="stable"' in M.__doc__ and M.img_shape == [224, 224, 3]
    for name in ("hausdorff_distance", "hausdorf_dist", "hausdorff_pair"):
        assert callable(getattr(AM, name)), name
    assert "not part of this build" not in AM.__doc__
    assert callable(RS.run_active_rounds)
    big = np.zeros((33, 33), np.uint8)
    with pytest.raises(ValueError):
        AM.hausdorff_pair(big, big)


def test_dataset_repeats_and_drops_the_remainder():
    import torch
    from pldepth_amd.active_learning.active_learning_method import ActiveDataset
    x, y = torch.arange(5.0)[:, None], torch.arange(5.0)[:, None] * 10
    ds = ActiveDataset(x, y, 2, [1.0] * 5, [0.0] * 5)
    assert len(ds) == 2
    it = iter(ds)
    got = [next(it)[0][:, 0].tolist() for _ in range(5)]
    assert got == [[0, 1], [2, 3], [0, 1], [2, 3], [0, 1]]
    assert [b[1][0, 0].item() for b, _ in zip(iter(ds), range(2))] == [0, 20]  # re-iterable
    assert list(ActiveDataset(x[:1], y[:1], 2, [], [])) == []


def test_cli_help():
    p = subprocess.run([sys.executable, "-m", "pldepth_amd.run_scripts.active_PLDepth", "--help"],
                       cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    for opt in ("--model_name", "--epochs", "--batch_size", "--seed", "--ranking_size",
                "--rankings_per_image", "--initial_lr", "--equality_threshold",
                "--model_checkpoints", "--load_model_path", "--augmentation", "--warmup",
                "--sampling_type", "--lr_multi", "--ds_size"):
        assert opt in p.stdout, opt
