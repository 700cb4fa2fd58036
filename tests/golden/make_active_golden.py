"""Generate active-learning golden vectors from the REFERENCE functions (container-only script).

Runs the reference's ``hausdorf_dist`` / ``hausdorff_pair`` (pldepth/active_learning/
metrics.py:9-57, scipy's real cKDTree), ``active_sampling`` and ``oracle``
(active_learning_method.py:22-76) and ``unsharp_mask`` (preprocess_utils.py:16-26) on the seeded
fixtures of tests/al_ref.py and writes their results to ``active_golden.npz``. Only arrays are
written; no reference source is copied. The edge maps themselves are not stored: the tests
rebuild them from the same seeds.

OpenCV, TensorFlow and wandb are not installed here. Placeholder modules are registered: ``cv2``
with ``GaussianBlur`` = the restatement of tests/al_ref.py (unpinned), ``tensorflow`` empty, and
``wandb`` whose ``log`` does nothing.

The reference's chosen input pixel depends on cKDTree's tie order where the nearest input pixel
is not unique; equality is waived on those tiles only, and this script asserts that they stay at
most 1/6 of the tiles with edges in both maps, per fixture.

Run:  python tests/golden/make_active_golden.py
"""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
import al_ref as A  # noqa: E402

TIE_CAP = 1.0 / 6.0


def _import_reference():
    cv2 = types.ModuleType("cv2")

    def GaussianBlur(src, ksize, sigmaX):
        assert tuple(ksize) == (5, 5) and src.dtype == np.float32
        return A.gaussian5(src, sigmaX)

    cv2.GaussianBlur = GaussianBlur
    sys.modules["cv2"] = cv2
    tf = types.ModuleType("tensorflow")
    tfk = types.ModuleType("tensorflow.keras")
    tfku = types.ModuleType("tensorflow.keras.utils")
    tfku.Sequence = object
    tf.keras, tfk.utils = tfk, tfku
    sys.modules.update({"tensorflow": tf, "tensorflow.keras": tfk, "tensorflow.keras.utils": tfku})
    wandb = types.ModuleType("wandb")
    wandb.log = lambda *a, **k: None
    sys.modules["wandb"] = wandb
    sys.path.insert(0, REF)
    from pldepth.active_learning import active_learning_method as M  # noqa: E402
    from pldepth.active_learning import metrics, preprocess_utils  # noqa: E402
    for m in (M, metrics, preprocess_utils):
        assert m.__file__.startswith(REF), m.__file__
    return M, metrics, preprocess_utils


def per_tile(metrics, e_in, e_pred, split):
    """[split^2] squared hausdorf_dist (-1 for inf) and [split^2][4] hausdorff_pair (-1: none)."""
    si, sp = A.split_image(e_in, split), A.split_image(e_pred, split)
    hd2 = np.zeros(len(si), np.int64)
    pair = np.full((len(si), 4), -1, np.int64)
    tied = both = 0
    for i in range(len(si)):
        d = metrics.hausdorf_dist(si[i], sp[i])
        hd2[i] = -1 if np.isinf(d) else int(round(d * d))
        assert hd2[i] < 0 or abs(np.sqrt(float(hd2[i])) - d) == 0.0
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            pa, pb = metrics.hausdorff_pair(si[i], sp[i])
        if len(pa):
            both += 1
            pair[i] = [pa[0], pa[1], pb[0], pb[1]]
            t = A.tied_inputs(si[i], sp[i])
            tied += t is not None and len(t) > 1
    return hd2, pair, tied, both


def main():
    M, metrics, PU = _import_reference()
    out = {}
    maps = [A.fixture_edges(s) + (A.FIXTURES[s][1],) for s in range(len(A.FIXTURES))]
    ha, hb = A.handmade_edges()
    maps += [(ha[k], hb[k], 2) for k in range(len(ha))]
    for f, (e_in, e_pred, split) in enumerate(maps):
        hd2, pair, tied, both = per_tile(metrics, e_in, e_pred, split)
        assert both > 0 and tied <= TIE_CAP * both, (f, tied, both)
        out[f"f{f}_hd2"], out[f"f{f}_pair"] = hd2.astype(np.int32), pair.astype(np.int32)
        out[f"f{f}_tied"] = np.array([tied, both], np.int32)
        h = e_in.shape[0]
        np.random.seed(7)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            pos, pts, mean, var = M.active_sampling(e_in, e_pred, split, [h, h, 3])
        out[f"f{f}_pos"], out[f"f{f}_pts"] = pos, pts
        out[f"f{f}_stat"] = np.array([mean, var], np.float64)
        out[f"f{f}_rng"] = np.random.get_state()[1].copy()
        out[f"f{f}_rng_pos"] = np.int64(np.random.get_state()[2])
        gt = np.random.default_rng(900 + f).random((h, h)).astype(np.float32)  # no equal depths
        for L in (3, 4):
            np.random.seed(11 + L)
            pxy = pts.copy()
            out[f"f{f}_oracle{L}"] = M.oracle(None, gt, pxy, L, [h, h, 3])
            out[f"f{f}_oracle{L}_rng_pos"] = np.int64(np.random.get_state()[2])
    rng = np.random.default_rng(3)
    for k, shape in enumerate([(5, 5), (20, 33)]):
        x = (rng.random(shape) * 255).astype(np.float32)
        out[f"u{k}_x"], out[f"u{k}_sharp"] = x, PU.unsharp_mask(x)
    out["n"] = np.int32(len(maps))
    np.savez_compressed(os.path.join(HERE, "active_golden.npz"), **out)
    print({k: v.tolist() for k, v in out.items() if k.endswith(("_tied", "_stat"))})
    print(os.path.getsize(os.path.join(HERE, "active_golden.npz")), "bytes")


if __name__ == "__main__":
    main()
