"""Generate depth-edge metric golden vectors from the REFERENCE function (container-only script).

Runs the reference's ``depth_edge_metric`` (pldepth/active_learning/metrics.py:123-144, which
calls ``auto_canny``, preprocess_utils.py:4-13) on seeded synthetic depth maps and writes the
inputs, the edge maps and the two results to ``edge_golden.npz``. Only arrays are written; no
reference source is copied.

OpenCV is not installed here. A placeholder ``cv2`` module is registered whose ``normalize``,
``Canny`` and ``distanceTransform`` are the restatements of tests/edge_ref.py (unpinned). What
this pins is the reference's own part: the median thresholds and their int() truncation, the
``> 10`` cut, the float32 products, the sums and the division, nan for an empty edge map
included. scipy (cKDTree, imported by metrics.py at module level) is real.

Run:  python tests/golden/make_edge_golden.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
import edge_ref as R  # noqa: E402


def _cv2_stub(seen):
    m = types.ModuleType("cv2")
    m.NORM_MINMAX = 32
    m.DIST_L2 = 2

    def normalize(src, dst, alpha, beta, norm_type):
        assert norm_type == m.NORM_MINMAX and dst is None and alpha == 0
        src = np.asarray(src, np.float32)
        return R.minmax_f32(src, float(beta)).reshape(src.shape)

    def Canny(image, threshold1, threshold2):
        assert image.dtype == np.uint8
        e = R.canny(image.reshape(image.shape[:2]), threshold1, threshold2)
        seen.append((int(threshold1), int(threshold2), e))
        return e

    def distanceTransform(src, distance_type, mask_size):
        assert distance_type == m.DIST_L2 and mask_size == 3 and src.dtype == np.uint8
        return R.chamfer_dt3(src, np.inf)

    m.normalize, m.Canny, m.distanceTransform = normalize, Canny, distanceTransform
    return m


def _import_reference_metrics(seen):
    sys.modules["cv2"] = _cv2_stub(seen)
    sys.path.insert(0, REF)
    from pldepth.active_learning import metrics  # noqa: E402
    assert metrics.__file__.startswith(REF), metrics.__file__
    return metrics


def cases():
    """(prediction, ground truth) pairs, (H, W, 1) float32."""
    step = np.zeros((12, 16, 1), np.float32)
    step[:, 8:] = 200
    step10 = np.zeros((12, 16, 1), np.float32)
    step10[:, 10:] = 200
    const = np.full((12, 16, 1), 3.0, np.float32)
    out = [(step, step), (step, step10), (const, step), (step, const)]
    for c, (h, w) in enumerate([(33, 47), (64, 64), (96, 80)]):
        gt = R.scene(h, w, 100 + c)
        op = np.roll(gt, 1, axis=1) + 0.01 * np.random.default_rng(c).standard_normal(
            gt.shape).astype(np.float32)
        out.append((op.astype(np.float32), gt))
    return out


def main():
    seen = []
    M = _import_reference_metrics(seen)
    out = {}
    for c, (op, gt) in enumerate(cases()):
        del seen[:]
        with np.errstate(invalid="ignore"):
            b, d = M.depth_edge_metric(op, gt)
        (lo_o, hi_o, e_op), (lo_g, hi_g, e_gt) = seen
        out[f"c{c}_op"], out[f"c{c}_gt"] = op, gt
        out[f"c{c}_thr"] = np.array([[lo_o, hi_o], [lo_g, hi_g]], np.int32)
        out[f"c{c}_e_op"], out[f"c{c}_e_gt"] = e_op, e_gt
        out[f"c{c}_res"] = np.array([b, d], np.float64)
    out["n"] = np.int32(len(cases()))
    np.savez_compressed(os.path.join(HERE, "edge_golden.npz"), **out)
    print({k: v.tolist() for k, v in out.items() if k.endswith(("_res", "_thr"))})


if __name__ == "__main__":
    main()
