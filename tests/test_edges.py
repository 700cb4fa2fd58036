"""Depth-edge metric, CPU side: the NumPy yardstick (tests/edge_ref.py) against answers derived
by hand, its two arithmetic forms against each other and against the reference's own results
(tests/golden/edge_golden.npz), and the ctypes signatures of the new entry points."""
import math
import os

import numpy as np
import pytest

import edge_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D1 = 62587 / 65536  # one edge step of the chamfer transform


@pytest.fixture(scope="module")
def eg():
    return np.load(os.path.join(ROOT, "tests", "golden", "edge_golden.npz"))


def _step(col, h=12, w=16):
    a = np.zeros((h, w, 1), np.float32)
    a[:, col:] = 200
    return a


# ---------------------------------------------------------------- known answers
def test_step_image_by_hand():
    """Columns 0-7 = 0, 8-15 = 200: u8 values 0 / 255, median 127.5, thresholds (0, 255);
    |dx| = 1020 on columns 7 and 8, and the row rule (m > left and m >= right) keeps column 7."""
    img = R.minmax_u8(_step(8)[..., 0])
    assert set(np.unique(img)) == {0, 255}
    assert R.auto_thresholds(img) == (0, 255)
    E = R.auto_canny(img)
    want = np.zeros((12, 16), np.uint8)
    want[:, 7] = 255
    assert np.array_equal(E, want)
    dt = R.chamfer_dt3(E)
    assert dt.dtype == np.float32
    assert np.array_equal(dt, np.where(want, np.float32(D1), np.float32(0)))
    assert abs(D1 - 0.95500183) < 1e-8


def test_metric_known_answers():
    assert R.exact(_step(8), _step(8)) == (D1, D1)
    assert R.exact(_step(8), _step(10)) == (0.0, 0.0)  # edges at columns 7 and 9: no overlap
    const = np.full((12, 16, 1), 3.0, np.float32)
    b, c = R.exact(const, _step(8))
    assert math.isnan(b) and c == 0.0
    b, c = R.exact(_step(8), const)
    assert b == 0.0 and math.isnan(c)
    b, c = R.as_reference(const, _step(8))
    assert math.isnan(b) and c == 0.0


def test_median_of_even_count_is_half_integer():
    img = np.array([[10, 10, 11, 200]], np.uint8)  # median 10.5
    assert R.auto_thresholds(img, 1.8) == (0, int(2.8 * 10.5))
    assert R.auto_thresholds(img, 0.5) == (int(0.5 * 10.5), int(1.5 * 10.5))


def test_hysteresis_keeps_only_connected_weak_pixels():
    lab = np.zeros((5, 9), np.uint8)
    lab[2, 1] = 2
    lab[2, 2:5] = 1   # chain attached to the strong pixel
    lab[1, 5] = 1     # diagonal continuation
    lab[4, 8] = 1     # isolated weak pixel
    E = R.hysteresis(lab)
    want = np.zeros_like(lab)
    want[2, 1:5] = 255
    want[1, 5] = 255
    assert np.array_equal(E, want)


# ---------------------------------------------------------------- chamfer transform
def _masks():
    rng = np.random.default_rng(11)
    block = np.zeros((40, 40), np.uint8)
    block[5:35, 5:35] = 255
    return {"random": (rng.random((20, 24)) < 0.6).astype(np.uint8) * 255, "block": block,
            "full": np.full((12, 12), 255, np.uint8)}


def test_chamfer_two_pass_equals_per_pixel_form():
    """The kernels evaluate the transform per pixel over a 21 x 21 window; wherever the two-pass
    result is at most 10 (11 steps of 0.955 are more) the two agree bit for bit."""
    for name, m in _masks().items():
        two = R.chamfer_two_pass_fixed(m)
        win = R.chamfer_window_fixed(m, 10)
        near = two <= 10 * 65536
        assert np.array_equal(two[near], win[near]), name
        assert np.all(win[~near] > 10 * 65536), name


def test_chamfer_cut_and_full_mask():
    m = _masks()
    dt = R.chamfer_dt3(m["block"])
    raw = R.chamfer_two_pass_fixed(m["block"]) / 65536
    assert abs(raw.max() - 14.3) < 0.05 and np.count_nonzero(raw > 10) == 100
    assert np.count_nonzero(dt > 10) == 0 and np.all(dt[raw > 10] == 0)
    assert dt[5, 5] == np.float32(D1) and dt[6, 6] == np.float32(2 * 62587 / 65536)
    assert np.all(R.chamfer_dt3(m["full"]) == 0)  # no zero pixel anywhere


# ---------------------------------------------------------------- the reference's arithmetic
def _close(a, b, rel=1e-5):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= rel * abs(b)


def test_exact_matches_reference_results(eg):
    """Integer sums against the reference's float32 np.sum (pairwise: about (128 + log2 n)
    roundings of 2^-24, below 1e-5 relative for n <= 2e5) on its recorded results."""
    n = int(eg["n"])
    assert n >= 7
    for c in range(n):
        op, gt = eg[f"c{c}_op"], eg[f"c{c}_gt"]
        E_op, E_gt = R.edge_maps(op, gt)
        assert np.array_equal(E_op, eg[f"c{c}_e_op"]) and np.array_equal(E_gt, eg[f"c{c}_e_gt"])
        thr = [R.auto_thresholds(R.minmax_u8(a[..., 0])) for a in (op, gt)]
        assert np.array_equal(np.array(thr), eg[f"c{c}_thr"])
        ex, ar, res = R.exact(op, gt), R.as_reference(op, gt), eg[f"c{c}_res"]
        for k in range(2):
            assert _close(ex[k], float(res[k])), (c, k, ex, res)
            assert _close(ex[k], ar[k]), (c, k, ex, ar)
            assert ar[k] == float(res[k]) or (math.isnan(ar[k]) and math.isnan(res[k]))


def test_exact_matches_as_reference_at_metric_size():
    gt = R.scene(224, 224, 7)
    op = np.roll(gt, 1, axis=1)
    ex, ar = R.exact(op, gt), R.as_reference(op, gt)
    assert ex[0] > 0 and ex[1] > 0
    assert _close(ex[0], ar[0]) and _close(ex[1], ar[1])


# ---------------------------------------------------------------- ABI
def test_edge_signatures_load():
    from pldepth_amd import _lib
    lib = _lib.lib()
    names = ["pld_minmax_u8_workspace_size", "pld_minmax_u8", "pld_canny_workspace_size",
             "pld_canny_u8", "pld_auto_canny_u8", "pld_chamfer_dt3", "pld_depth_edge_metric"]
    for s in names:
        assert s in _lib._SIGS and callable(getattr(lib, s)), s
        assert len(getattr(lib._dll, s).argtypes) == len(_lib._SIGS[s][1])
    assert set(names) <= set(_lib.declared_symbols())
    # host-only parts: workspace sizes, and argument checks that fail before any launch
    assert lib.pld_minmax_u8_workspace_size(3) == 3 * 64 * 2 * 4
    assert lib.pld_canny_workspace_size(2, 224, 224) == (2 * 256 + 2 * 2 * 224 * 8) * 4
    assert lib.pld_canny_workspace_size(1, 512, 512) == (256 + 2 * 512 * 16) * 4
    assert lib.pld_canny_workspace_size(0, 8, 8) == 0
    for call in (lambda: lib.pld_depth_edge_metric(None, None, 1, 8, 8, None, None),
                 lambda: lib.pld_canny_u8(None, 1, 8, 8, 0, 255, None, None, None, None),
                 lambda: lib.pld_chamfer_dt3(None, 1, 8, 8, 10.0, None, None)):
        with pytest.raises(_lib.PLDError, match="bad args"):
            call()


def test_api_no_longer_placeholder():
    import inspect

    from pldepth.active_learning.preprocess_utils import auto_canny
    from pldepth_amd.active_learning import metrics as AM
    assert auto_canny.__module__ == "pldepth_amd.active_learning.preprocess_utils"
    for fn in (AM.depth_edge_metric, AM.calc_depth_metrics):
        assert "NotImplementedError" not in inspect.getsource(fn)
    assert list(inspect.signature(AM.depth_edge_metric).parameters) == ["op", "gt", "imsize"]
