"""Generate golden vectors of the REFERENCE numpy samplers run with non-default arguments
(container-only script; ``/root/reference`` does not exist on the GPU box).

Like make_sampler_golden.py, it writes arrays only (``sampler_params_golden.npz`` next to
itself): inputs as 8-bit gt codes and a packed validity mask, the exact ``np.random.randint``
sequence the reference consumed, and the reference's outputs. No reference source or bytecode is
copied.

Reference code exercised (read-only):
  * ``pldepth/data/sampling.py:89-103``  ``RandomSamplingStrategy.sample_points_batch``
  * ``pldepth/data/sampling.py:111-150`` masked rankings with x_scale / y_scale, Purely masked
  * ``pldepth/data/sampling.py:179-208`` Thresholded(threshold, equality_penalty)
  * ``pldepth/data/sampling.py:212-239`` Information score(threshold, equality_penalty)
each with a per-call ``batch_size_factor``.

TensorFlow is replaced by an empty placeholder module as in make_sampler_golden.py. The unmasked
path reads ``np.int``, an alias NumPy removed: it is set to ``int`` before the import.

Every output is compared, tie-insensitively, with the restatement tests/sampler_params_ref.py at
generation time. The reference orders equal scores machine-dependently (unstable argsort): if a
seed puts a tie across the top-R cut the assertion fails; change SEED, never drop a case.

Run:  python tests/golden/make_sampler_params_golden.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))                    # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the repository (oracle/)
import sampler_params_ref as P  # noqa: E402

SEED = 2  # 1 ties the unmasked L = 70 case's scores (max - min of 70 codes) across the cut
# (H, W, mask_h, mask_w, L, R, tau, penalty, factor)
CASES = [(24, 32, 24, 32, 5, 20, 0.1, -2.5, 2.2),
         (24, 32, 12, 16, 9, 10, 0.3, -1000, 1.5),
         (20, 28, 40, 14, 70, 6, 0.01, -7, 3),
         (16, 16, 16, 16, 3, 15, 0.5, -0.1, 1.0)]
STRATEGIES = ("thresh", "info", "pure", "random")


def _import_reference_sampling():
    for name in ("tensorflow", "tensorflow.python", "tensorflow.python.keras",
                 "tensorflow.python.keras.backend"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["tensorflow"].float32 = "float32"
    np.int = int  # sampling.py:67,94 (removed in NumPy 1.24)
    sys.path.insert(0, REF)
    from pldepth.data import sampling  # noqa: E402
    assert sampling.__file__.startswith(REF), sampling.__file__
    return sampling


class _Params:
    def __init__(self, ranking_size):
        self.p = {"ranking_size": ranking_size, "downscaling_factor": 1}

    def get_parameter(self, name, default=None):
        return self.p.get(name, default)


def case_inputs(ci, h, w, mh, mw):
    """Uniform 8-bit depth codes on the image grid, a Bernoulli(0.8) mask on its own grid."""
    rng = np.random.default_rng(SEED + ci)
    codes = rng.integers(0, 256, (h, w), dtype=np.uint8)
    mask = rng.random((mh, mw)) < 0.8
    return codes, mask


def generate(sampling):
    # run (case ci, strategy number si of STRATEGIES) starts from np.random.seed(seed+100*ci+si)
    out = {"cases": np.array(CASES, np.float64), "seed": np.array(SEED, np.int64)}
    orig_randint = np.random.randint
    for ci, (h, w, mh, mw, L, R, tau, pen, factor) in enumerate(CASES):
        codes, mask = case_inputs(ci, h, w, mh, mw)
        gt = codes.astype(np.float32) / np.float32(255.0)
        maskf = mask.astype(np.float32)
        image = np.zeros((h, w, 3), np.float32)
        out[f"c{ci}_codes"] = codes
        out[f"c{ci}_mask"] = np.packbits(mask)
        p = _Params(L)
        runs = {
            "thresh": lambda: sampling.ThresholdedMaskedRandomSamplingStrategy(
                p, tau, pen).sample_masked_point_batch(image, maskf, gt, R, factor),
            "info": lambda: sampling.InformationScoreBasedSampling(
                p, tau, pen).sample_masked_point_batch(image, maskf, gt, R, factor),
            "pure": lambda: sampling.PurelyMaskedRandomSamplingStrategy(
                p).sample_masked_point_batch(image, maskf, gt, R, factor),
            "random": lambda: sampling.RandomSamplingStrategy(
                p).sample_points_batch(image, gt, R, factor),
        }
        for si, sname in enumerate(STRATEGIES):
            draws = []

            def rec(*a, **k):
                v = orig_randint(*a, **k)
                draws.append(int(v))
                return v

            np.random.seed(SEED + 100 * ci + si)
            np.random.randint = rec
            try:
                res = np.asarray(runs[sname](), np.float32)
            finally:
                np.random.randint = orig_randint
            d = np.asarray(draws, np.int32)
            out[f"c{ci}_{sname}_draws"] = d
            out[f"c{ci}_{sname}_out"] = res
            # the restatement reproduces the reference (ties aside) for these very draws
            if sname == "random":  # randint(H), randint(W) per slot -> flat pixel
                d = d[0::2].astype(np.int64) * w + d[1::2]
            mine = P.sample_point_batch(sname, maskf, gt, R, L, d, tau, pen, factor)
            assert mine.shape == res.shape, (ci, sname, mine.shape, res.shape)
            assert np.array_equal(P.canonical_lists(mine), P.canonical_lists(res)), (
                f"case {ci} {sname}: the restatement and the reference keep different lists "
                "(a score tie across the top-R cut?): change SEED")
            print(f"case{ci} {h}x{w} mask {mh}x{mw} L={L} R={R} {sname}: draws={len(draws)} "
                  f"out={res.shape}")
    return out


def main():
    out = generate(_import_reference_sampling())
    np.savez_compressed(os.path.join(HERE, "sampler_params_golden.npz"), **out)
    print("wrote", os.path.join(HERE, "sampler_params_golden.npz"))


if __name__ == "__main__":
    main()
