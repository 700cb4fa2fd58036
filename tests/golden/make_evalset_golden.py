"""Generate the evaluation goldens from the REFERENCE providers (container-only script).

Like make_sampler_golden.py this runs only where the reference checkout exists and writes arrays
only: ``evalset_golden.npz`` next to itself holds inputs, the ``np.random.randint`` draws the
reference consumed, its outputs, and the next value of the global numpy RNG after each call.

Reference code exercised (read-only):
  * ``pldepth/data/providers/generic_ranking_provider.py:80-111`` ``generate_ordinal_pairs``
  * ``pldepth/data/providers/generic_ranking_provider.py:180-215`` ``generate_rankings``
  * ``pldepth/data/depth_utils.py:5-21`` ``get_depth_relation``
The resize cases are not the reference's code but the rule its ``skimage.transform.resize`` calls
follow (scikit-image >= 0.19, not installed here: unpinned), composed from scipy.ndimage in
float64: ``gaussian_filter(mode='mirror')`` with sigma = max(0, (in / out - 1) / 2) per axis when
an axis shrinks, then ``zoom(order=1, mode='mirror', grid_mode=True)``.

TensorFlow is not installed: a placeholder module carries what the provider module touches
(``tf.data.experimental.cardinality`` = ``len``, ``tf.float32`` for a default argument), and the
datasets are lists with ``as_numpy_iterator``. ``np.int`` (removed from NumPy) is set to ``int``
for the call, as the reference predates NumPy 2.

Run:  python tests/golden/make_evalset_golden.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def _import_reference_provider():
    for name in ("tensorflow", "tensorflow.python", "tensorflow.python.keras",
                 "tensorflow.python.keras.backend"):
        sys.modules.setdefault(name, types.ModuleType(name))
    tf = sys.modules["tensorflow"]
    tf.float32 = "float32"
    tf.data = types.SimpleNamespace(experimental=types.SimpleNamespace(cardinality=len))
    sys.path.insert(0, REF)
    from pldepth.data.providers import generic_ranking_provider as grp
    assert grp.__file__.startswith(REF), grp.__file__
    return grp


class _Params:
    def __init__(self, **p):
        self.p = p

    def get_parameter(self, name, default=None):
        return self.p.get(name, default)


class _ListDataset(list):
    def as_numpy_iterator(self):
        return iter(self)


def _recorded(fn):
    """fn() with every np.random.randint result recorded; (result, draws, next RNG value)."""
    orig, draws = np.random.randint, []

    def rec(*a, **k):
        v = orig(*a, **k)
        draws.append(int(v))
        return v

    np.random.randint = rec
    had_int = hasattr(np, "int")
    if not had_int:
        np.int = int
    try:
        res = fn()
    finally:
        np.random.randint = orig
        if not had_int:
            del np.int
    return res, np.asarray(draws, np.int32), np.int64(np.random.randint(1 << 30))


def eight_bit_gts(n, h, w, seed):
    """Smooth depth maps quantised to 8 bits; the top four rows are constant."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    codes = np.empty((n, h, w), np.uint8)
    for i in range(n):
        f = np.zeros((h, w))
        for _ in range(4):
            fy, fx = rng.uniform(0.3, 3.0, 2)
            ph = rng.uniform(0, 2 * np.pi, 2)
            f += rng.uniform(0.2, 1.0) * np.sin(2 * np.pi * fy * yy + ph[0]) * \
                np.cos(2 * np.pi * fx * xx + ph[1])
        f = (f - f.min()) / (f.max() - f.min())
        codes[i] = np.round(255 * f)
        codes[i, :4] = codes[i, 4, 0]
    return codes


def resize_rule_f64(x, oh, ow):
    from scipy import ndimage as ndi
    y = x.astype(np.float64)
    h, w = y.shape[:2]
    if oh < h or ow < w:
        y = ndi.gaussian_filter(y, [max(0.0, (h / oh - 1) / 2), max(0.0, (w / ow - 1) / 2), 0.0],
                                mode="mirror")
    y = ndi.zoom(y, (oh / h, ow / w, 1), order=1, mode="mirror", grid_mode=True)
    assert y.shape == (oh, ow, x.shape[2]), y.shape
    return y


def main():
    grp = _import_reference_provider()
    N, H, W, P, R, SEED = 3, 24, 40, 50, 20, 3
    out = {"shape": np.array([N, H, W, P, R, SEED], np.int64)}
    codes = eight_bit_gts(N, H, W, seed=11)
    gts8 = codes.astype(np.float32) / np.float32(255.0)
    gtsc = np.random.default_rng(12).random((N, H, W), dtype=np.float32)
    out["codes"], out["gts_cont"] = codes, gtsc
    imgs = np.zeros((N, H, W, 3), np.float32)

    def dataset(gts):
        return _ListDataset((imgs[i], gts[i]) for i in range(N))

    mp = _Params(dataset="SINTEL", val_rankings_per_img=P)
    for inv in (0, 1):
        prov = grp.GenericHourglassPairRelationDataProvider(mp, SEED, bool(inv), threshold=0.03)
        np.random.seed(SEED)
        res, draws, nxt = _recorded(lambda: prov.generate_ordinal_pairs(
            dataset(gts8), invert_relation_sign=bool(inv)))
        rel = res[..., 2]
        counts = [(rel == v).sum() for v in (-1, 0, 1)]
        assert min(counts) >= 1, counts
        out[f"pairs_inv{inv}"], out[f"pairs_inv{inv}_next"] = res, nxt
        if inv == 0:
            out["pairs_draws"] = draws.reshape(N, P, 4)
        else:
            assert np.array_equal(out["pairs_draws"], draws.reshape(N, P, 4))
        print(f"pairs invert={inv}: -1/0/+1 = {counts}, next {nxt}")
    for gname, gts in (("q8", gts8), ("cont", gtsc)):
        for L in (5, 40):
            for inv in (0, 1):
                prov = grp.GenericHourglassRankingDataProvider(mp, L, SEED, bool(inv))
                np.random.seed(SEED)
                res, draws, nxt = _recorded(lambda: prov.generate_rankings(
                    dataset(gts), invert_relation_sign=bool(inv), val_rankings_per_img=R))
                key = f"rank_{gname}_L{L}_inv{inv}"
                out[key], out[key + "_next"] = res, nxt
                out[f"rank_draws_L{L}"] = draws.reshape(N, R, L)
                # a pixel drawn twice gives two identical rows; a tie is two DIFFERENT pixels of
                # one list with the same depth
                ties = sum(len(np.unique(l[:, 1])) < len(np.unique(l[:, 0]))
                           for l in res.reshape(-1, L, 2))
                assert gname == "q8" or ties == 0, (key, ties)
                print(f"{key}: lists with ties {ties}/{N * R}, next {nxt}")
    rng = np.random.default_rng(13)
    for k, (h, w, c, oh, ow) in enumerate([(37, 53, 1, 16, 24), (30, 44, 3, 16, 16),
                                           (12, 10, 1, 16, 24), (40, 12, 1, 16, 24)]):
        x = rng.random((h, w, c), dtype=np.float32)
        out[f"resize{k}_in"], out[f"resize{k}_out"] = x, resize_rule_f64(x, oh, ow)
    path = os.path.join(HERE, "evalset_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
