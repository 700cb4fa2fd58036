"""Ranking samplers (mirrors pldepth/data/sampling.py) backed by the GPU sampler.

Same class names, hierarchy, constructors and per-image entry points as the reference:
``Strategy(model_params[, threshold, equality_penalty]).sample_masked_point_batch(image, mask, gt,
batch_size[, batch_size_factor])`` and, unmasked, ``RandomSamplingStrategy(model_params)
.sample_points_batch(image, gt, batch_size[, batch_size_factor])`` -> float32 [R', L, 2] (flat
pixel index row*W+col, depth), the best-scoring R of int(R * batch_size_factor) candidate lists.
Masked lists are sorted by depth descending, unmasked ones keep their draw order. The consistency
mask may have another resolution than gt: a drawn mask position maps to the pixel
(int(row * H / mask_h), int(col * W / mask_w)), sampling.py:115-116,125-129.

Like the reference, the per-image calls consume the global NumPy RNG —
``np.random.randint(n_valid)`` once per list slot, list-major (sampling.py:113), or
``randint(H)`` then ``randint(W)`` per slot for the unmasked sampler (sampling.py:94) — and ship
the draws to the rank kernels, so a seeded run reproduces the reference's rankings (ties aside,
which the reference itself orders machine-dependently).

The batched GPU path (``sample_batch_gpu``) keeps draws on the device (Philox counter keyed by
seed/step/image: independent of the GPU count) and is what the training step uses. A strategy
with the reference's default arguments and a mask at the image's resolution runs
pld_sampler_rank; any other tau, penalty, factor or mask grid, and the unmasked sampler, run
pld_sampler_rank_ex, the same kernels with those values as arguments.

Not built: ``RandomSamplingStrategy.sample_points`` (sampling.py:75-87), a sequential rejection
loop whose draw count depends on the data and that nothing in the reference calls.
"""
import numpy as np
import torch

from .. import kernels as K
from .depth_utils import get_depth_relation  # noqa: F401  (re-exported like the reference)

DEFAULT_THRESHOLD, DEFAULT_PENALTY = 0.03, -1000


class SamplingStrategy(object):
    def __init__(self, model_params):
        self.num_points_per_sample = model_params.get_parameter("ranking_size")

    @property
    def num_points_per_sample(self):
        return self._num_points_per_sample

    @num_points_per_sample.setter
    def num_points_per_sample(self, value):
        self._num_points_per_sample = value

    @staticmethod
    def calculate_depth_differences(depth_values):
        """sampling.py:33-42: the sum of adjacent gaps of the depths sorted descending."""
        depth_values = np.asarray(depth_values)
        sorted_depths = depth_values[np.argsort(depth_values, kind="stable")[::-1]]
        tmp_dist = 0
        for j in range(len(sorted_depths) - 1):
            tmp_dist += abs(sorted_depths[j] - sorted_depths[j + 1])
        return tmp_dist

    def __str__(self):
        return "{}(num_points_per_sample={})".format(self.__class__.__name__,
                                                    self._num_points_per_sample)


class RandomSamplingStrategy(SamplingStrategy):
    """sampling.py:48-103: unmasked; 1.5 R candidate lists of uniformly drawn pixels, kept in draw
    order and scored by calculate_depth_differences."""
    NAME, FACTOR = "random", 1.5
    equality_penalty = DEFAULT_PENALTY

    def __init__(self, model_params):
        super(RandomSamplingStrategy, self).__init__(model_params)
        self.threshold = DEFAULT_THRESHOLD
        self.downscaling_factor = model_params.get_parameter("downscaling_factor")
        # the factor of calls that name none (the batched GPU path): the reference's per-call
        # default unless set on the instance
        self.batch_size_factor = self.FACTOR

    def initialize_buffers(self, batch_size, batch_size_factor):
        result_matrix = np.zeros([int(batch_size * batch_size_factor),
                                  self._num_points_per_sample, 2], dtype=np.float32)
        gts_buffer = np.zeros(result_matrix.shape[1])
        point_buffer = np.zeros([self._num_points_per_sample])
        dists = np.zeros(result_matrix.shape[0])
        return result_matrix, gts_buffer, point_buffer, dists

    def sample_points(self, image, gt):
        raise NotImplementedError("sample_points (the sequential rejection loop of "
                                  "sampling.py:75-87) is not built; use sample_points_batch")

    # ---------------------------------------------------------------- GPU batch entry
    def rank_arguments(self, batch_size, batch_size_factor=None):
        """(n_cand, r_out, default) of a call: int(R * factor) candidates (sampling.py:55),
        min(n_cand, R) lists kept (``[:batch_size]``), and whether tau, penalty and factor are
        all the reference's defaults (pld_sampler_rank's)."""
        factor = self.batch_size_factor if batch_size_factor is None else batch_size_factor
        nc = int(batch_size * factor)
        if nc <= 0:
            raise ValueError(f"batch_size {batch_size} x factor {factor} leaves no candidate")
        default = (self.NAME != "random" and factor == self.FACTOR
                   and self.threshold == DEFAULT_THRESHOLD
                   and self.equality_penalty == DEFAULT_PENALTY)
        return nc, min(nc, batch_size), default

    def sample_batch_gpu(self, gt, mask, batch_size, seed=0, step=0, image_offset=0,
                         draws=None, batch_size_factor=None):
        """gt [B,H,W], mask [B,mask_h,mask_w] device tensors (mask None for the unmasked
        sampler) -> [B, R', L, 2] device tensor (Philox draws, or explicit draws [B, n_cand, L]
        int32: positions in np.where(mask > 0), flat pixels for the unmasked sampler)."""
        B, H, W = gt.shape
        L = self._num_points_per_sample
        dev = gt.device
        nc, r_out, default = self.rank_arguments(batch_size, batch_size_factor)
        gt = gt.contiguous()
        out = torch.empty(B, r_out, L, 2, device=dev)
        if mask is None or self.NAME == "random":  # unmasked: a draw is a pixel
            if draws is None:
                nv = torch.full((B,), H * W, dtype=torch.int32, device=dev)
                draws = torch.empty(B, nc, L, dtype=torch.int32, device=dev)
                K.sampler_draw(nv, nc, L, seed, step, image_offset, draws)
            return K.sampler_rank_ex(gt, None, None, None, draws.contiguous(), batch_size, L,
                                     "random", out, nc)
        mh, mw = mask.shape[1:]
        same_grid = (mh, mw) == (H, W)
        vi = torch.empty(B, mh * mw, dtype=torch.int32, device=dev)
        nv = torch.empty(B, dtype=torch.int32, device=dev)
        mm = torch.empty(B, 2, device=dev)
        if same_grid:
            K.sampler_compact(mask.contiguous(), gt, vi, nv, mm)
        else:  # positions of the mask's grid; the Info bounds stay those of the whole gt
            K.sampler_compact(mask.contiguous(), None, vi, nv, None)
            K.sampler_minmax(gt, mm)
        if draws is None:
            draws = torch.empty(B, nc, L, dtype=torch.int32, device=dev)
            K.sampler_draw(nv, nc, L, seed, step, image_offset, draws)
        if default and same_grid:
            return K.sampler_rank(gt, vi, nv, mm, draws.contiguous(), batch_size, L, self.NAME,
                                  out)
        return K.sampler_rank_ex(gt, vi, nv, mm, draws.contiguous(), batch_size, L, self.NAME,
                                 out, nc, self.threshold, self.equality_penalty, (mh, mw))

    # ---------------------------------------------------------------- reference entry
    def sample_points_batch(self, image, gt, batch_size, batch_size_factor=1.5):
        gt = np.asarray(gt, np.float32)
        H, W = gt.shape[:2]
        L = self._num_points_per_sample
        nc = int(batch_size * batch_size_factor)
        draws = np.empty(nc * L, np.int32)
        for i in range(nc * L):  # sampling.py:94: randint(H) then randint(W) per slot
            r = np.random.randint(H)
            draws[i] = r * W + np.random.randint(W)
        dev = torch.device("cuda", torch.cuda.current_device())
        out = self.sample_batch_gpu(
            torch.from_numpy(gt.reshape(1, H, W)).to(dev), None, batch_size,
            draws=torch.from_numpy(draws).view(1, nc, L).to(dev),
            batch_size_factor=batch_size_factor)
        return out[0].cpu().numpy()


class PurelyMaskedRandomSamplingStrategy(RandomSamplingStrategy):
    """sampling.py:106-150: floor(0.8 R) lists, no scoring."""
    NAME, FACTOR = "pure", 0.8

    @staticmethod
    def determine_x_y_scales(image, mask):
        return image.shape[0] / mask.shape[0], image.shape[1] / mask.shape[1]

    def sample_masked_point_batch(self, image, mask, gt, batch_size, batch_size_factor=None):
        mask = np.asarray(mask, np.float32)
        gt = np.asarray(gt, np.float32)
        H, W = gt.shape[:2]
        L = self._num_points_per_sample
        nc = self.rank_arguments(batch_size, batch_size_factor)[0]
        n_valid = int((mask > 0).sum())
        draws = np.random.randint(n_valid, size=nc * L).astype(np.int32)  # sampling.py:113
        dev = torch.device("cuda", torch.cuda.current_device())
        out = self.sample_batch_gpu(torch.from_numpy(gt.reshape(1, H, W)).to(dev),
                                    torch.from_numpy(mask)[None].to(dev), batch_size,
                                    draws=torch.from_numpy(draws).view(1, nc, L).to(dev),
                                    batch_size_factor=batch_size_factor)
        return out[0].cpu().numpy()


class MaskedRandomSamplingStrategy(PurelyMaskedRandomSamplingStrategy):
    """sampling.py:153-170: 1.5 R candidates scored by the sum of adjacent depth gaps."""
    NAME, FACTOR = "masked", 1.5


def _checked(threshold, equality_penalty):
    if threshold is None:
        raise ValueError("threshold=None (get_depth_relation's exact comparison) is not a "
                         "sampler threshold: pass tau >= 0")
    if not (np.isfinite(threshold) and threshold >= 0 and np.isfinite(equality_penalty)):
        raise ValueError(f"threshold {threshold!r} must be finite and not negative, "
                         f"equality_penalty {equality_penalty!r} finite")
    return threshold, equality_penalty


class ThresholdedMaskedRandomSamplingStrategy(MaskedRandomSamplingStrategy):
    """sampling.py:172-208: as Masked, equality_penalty per adjacent pair within tau."""
    NAME, FACTOR = "thresh", 1.5

    def __init__(self, model_params, threshold=DEFAULT_THRESHOLD,
                 equality_penalty=DEFAULT_PENALTY):
        super().__init__(model_params)
        self.threshold, self.equality_penalty = _checked(threshold, equality_penalty)

    def __str__(self):
        return "{}(num_points_per_sample={}, threshold={}, equality_penalty={})".format(
            self.__class__.__name__, self._num_points_per_sample, self.threshold,
            self.equality_penalty)


class InformationScoreBasedSampling(MaskedRandomSamplingStrategy):
    """sampling.py:211-242: 5 R candidates scored by -sum (g - e)^2 / e against an evenly spaced
    expected list, equality_penalty per near-equal adjacent pair (the PLDepth.py default)."""
    NAME, FACTOR = "info", 5

    def __init__(self, model_params, threshold=DEFAULT_THRESHOLD,
                 equality_penalty=DEFAULT_PENALTY):
        super().__init__(model_params)
        self.threshold, self.equality_penalty = _checked(threshold, equality_penalty)

    def __str__(self):
        return "{}(num_points_per_sample={}, threshold={})".format(
            self.__class__.__name__, self._num_points_per_sample, self.threshold)
