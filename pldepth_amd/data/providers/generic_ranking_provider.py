"""Drop-in for ``pldepth/data/providers/generic_ranking_provider.py``: the ordinal pair tables and
the held-out rankings a trained model is evaluated on (Ibims, Sintel, DIODE, TUM, HR-WSI).

Same classes, constructor arguments, methods and ``.npy`` cache file names as the reference
(:12-111 pairs, :114-223 rankings), so a cache written by either side loads in the other.

``base_ds`` is what this build's DAOs return: ``(imgs, gts)`` arrays or device tensors, or a list
of ``(img, gt)`` pairs (all of one size). The result of ``provide_val_dataset`` /
``provide_test_dataset`` is an ``EvalDataset``: iterating it gives ``(image, table)`` elements
like the reference's zipped dataset, ``.images`` / ``.targets`` are the stacked device tensors,
and ``.batch(B)`` gives ``(x, y)`` batches for ``model.evaluate``.

Randomness stays on the host, in the global numpy RNG and in the reference's order:
``np.random.seed(self.seed)``, then ONE vectorised call that consumes the generator exactly as
the reference's scalar calls do (same values, same end state; tests/test_evalset.py):
  pairs     np.random.randint(0, [H, W, H, W] * (N * P))   for :92-96's x0, y0, x1, y1 per pair
  rankings  np.random.randint(0, H * W, size=(N, R, L))     for :192-196's L draws per list
The gather, the relation, and the per-list sort run on the GPU (``pld_ordinal_pairs`` /
``pld_depth_rankings``), one launch for the whole set. Tie rule of the rankings:
ascending order is a stable sort by list position, descending is that order reversed; the
reference leaves ties to ``np.argsort``'s default (unstable) sort.
"""
import logging
import os

import numpy as np
import torch

from ... import kernels as K
from ..data_meta import TFDatasetDataProvider
from ..depth_utils import get_depth_relation


class EvalDataset(object):
    """A re-iterable of ``(image, table)`` elements over device tensors ``images`` [N, H, W, 3]
    and ``targets`` [N, ...]."""

    def __init__(self, images, targets):
        assert len(images) == len(targets), (len(images), len(targets))
        self.images, self.targets = images, targets

    def __len__(self):
        return len(self.images)

    def __iter__(self):
        return iter(zip(self.images, self.targets))

    def cache(self):
        return self

    def batch(self, batch_size, drop_remainder=True):
        """``(x [B, H, W, 3], y [B, ...])`` batches as a list. The model runs at its compiled
        batch size, so the remainder is dropped unless asked for."""
        n = len(self) // batch_size * batch_size if drop_remainder else len(self)
        return [(self.images[i:i + batch_size], self.targets[i:i + batch_size])
                for i in range(0, n, batch_size)]


def _device(a):
    if isinstance(a, torch.Tensor):
        return a.to(device="cuda", dtype=torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def split_base_ds(base_ds):
    """(images [N, H, W, 3], gts [N, H, W]) float32 device tensors of ``base_ds``."""
    if isinstance(base_ds, EvalDataset):
        imgs, gts = base_ds.images, base_ds.targets
    elif isinstance(base_ds, tuple) and len(base_ds) == 2:
        imgs, gts = base_ds
    else:
        pairs = list(base_ds)
        if not pairs:
            raise ValueError("the base dataset is empty")
        imgs, gts = [torch.stack(c) if isinstance(c[0], torch.Tensor) else np.stack(c)
                     for c in zip(*pairs)]
    imgs, gts = _device(imgs), _device(gts)
    if gts.dim() == 4 and gts.shape[-1] == 1:  # np.squeeze(elem[1])
        gts = gts[..., 0]
    if gts.dim() != 3 or len(gts) != len(imgs):
        raise ValueError(f"expected gts [N, H, W] for {len(imgs)} images, got {tuple(gts.shape)}")
    return imgs, gts.contiguous()


def draw_pair_coords(n, h, w, pairs_per_img):
    """[n, P, 4] = (x0, y0, x1, y1) from the global numpy RNG, as :92-96 draws them one by one."""
    return np.random.randint(0, np.tile([h, w, h, w], n * pairs_per_img)).reshape(
        n, pairs_per_img, 4)


def draw_ranking_indices(n, hw, rankings_per_img, ranking_size):
    """[n, R, L] flat pixel indices from the global numpy RNG, as :192-196 draws them."""
    return np.random.randint(0, hw, size=(n, rankings_per_img, ranking_size))


def _cached(path, save_on_disk, generate):
    if not save_on_disk:
        return generate()
    if not os.path.exists(path):
        table = generate()
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.save(path, table)
        return table
    return np.load(path)


class GenericHourglassPairRelationDataProvider(TFDatasetDataProvider):
    def __init__(self, model_params, seed, invert_relation_sign, threshold=0.03,
                 cache_val_data=True, save_pairs_on_disk=False, config=None):
        super().__init__(model_params)
        self.seed = seed
        self.invert_relation_sign = invert_relation_sign
        self.threshold = threshold
        self.cache_val_data = cache_val_data
        self.dataset_name = model_params.get_parameter("dataset")
        self.save_pairs_on_disk = save_pairs_on_disk
        if self.save_pairs_on_disk:
            assert config is not None, "If the generated pairs should be saved, a configuration " \
                                       "specifying the cache location must be given!"
        self.config = config

    def provide_train_dataset(self, base_ds, base_ds_gts=None):
        raise NotImplementedError("Training provision is not implemented yet.")

    def _cache_path(self, *parts):
        if self.config is None:  # only read when save_pairs_on_disk (checked in __init__)
            return None
        return os.path.join(self.config["DATA"]["CACHE_PATH_PREFIX"],
                            "ordinal_pair_cache/{}.npy".format("_".join(str(p) for p in parts)))

    def _provide(self, base_ds, cache_path):
        np.random.seed(self.seed)
        base = split_base_ds(base_ds)
        pairs = self.retrieve_ordinal_pairs(base, cache_path)
        if len(pairs) != len(base[0]):
            raise ValueError(f"{cache_path}: a table for {len(pairs)} images, the dataset holds "
                             f"{len(base[0])}")
        return EvalDataset(base[0], _device(pairs))

    def provide_val_dataset(self, base_ds, base_ds_gts=None):
        logging.debug("Retrieving validation rankings...")
        return self._provide(base_ds, self._cache_path(
            self.dataset_name, "val", self.model_params.get_parameter("val_rankings_per_img"),
            self.seed))

    def provide_test_dataset(self, base_ds):
        logging.debug("Retrieving test rankings...")
        return self._provide(base_ds, self._cache_path(
            self.dataset_name, self.model_params.get_parameter("val_rankings_per_img"),
            self.seed))

    def retrieve_ordinal_pairs(self, base_ds, cache_path):
        ordinal_pairs = _cached(cache_path, self.save_pairs_on_disk,
                                lambda: self.generate_ordinal_pairs(
                                    base_ds, invert_relation_sign=self.invert_relation_sign))
        logging.debug("Number of unequal relations: {}".format(
            np.sum(ordinal_pairs[:, :, 2] != 0)))
        logging.debug("Number of equal relations: {}".format(np.sum(ordinal_pairs[:, :, 2] == 0)))
        return ordinal_pairs

    def generate_ordinal_pairs(self, base_ds_imgs_gts, invert_relation_sign=False):
        """[N, val_rankings_per_img, 5] float32 (host): (point0, point1, relation, z0, z1)."""
        _, gts = split_base_ds(base_ds_imgs_gts)
        n, h, w = gts.shape
        coords = draw_pair_coords(n, h, w, self.model_params.get_parameter("val_rankings_per_img"))
        return K.ordinal_pairs(gts, coords, self.threshold, invert_relation_sign).cpu().numpy()


class GenericHourglassRankingDataProvider(TFDatasetDataProvider):
    def __init__(self, model_params, query_ranking_size, seed, invert_relation_sign,
                 threshold=0.03, cache_val_data=True, save_rankings_on_disk=False, config=None):
        super().__init__(model_params)
        self.query_ranking_size = query_ranking_size
        self.seed = seed
        self.invert_relation_sign = invert_relation_sign
        self.threshold = threshold
        self.cache_val_data = cache_val_data
        self.dataset_name = model_params.get_parameter("dataset")
        self.save_rankings_on_disk = save_rankings_on_disk
        if self.save_rankings_on_disk:
            assert config is not None, "If the generated rankings should be saved, a " \
                                       "configuration specifying the cache location must be given!"
        self.config = config

    def provide_train_dataset(self, base_ds, base_ds_gts=None):
        raise NotImplementedError("Providing training data is not supported.")

    def _cache_path(self, *parts):
        if self.config is None:
            return None
        return os.path.join(self.config["DATA"]["CACHE_PATH_PREFIX"],
                            "ranking_cache/{}.npy".format("_".join(str(p) for p in parts)))

    def _provide(self, base_ds, cache_path):
        np.random.seed(self.seed)
        base = split_base_ds(base_ds)
        rankings = self.retrieve_rankings(base, cache_path)
        if len(rankings) != len(base[0]):
            raise ValueError(f"{cache_path}: rankings for {len(rankings)} images, the dataset "
                             f"holds {len(base[0])}")
        return EvalDataset(base[0], _device(rankings))

    def provide_val_dataset(self, base_ds, base_ds_gts=None):
        logging.debug("Generating validation rankings...")
        return self._provide(base_ds, self._cache_path(
            self.dataset_name, "val", 100, self.seed, self.query_ranking_size))

    def provide_test_dataset(self, base_ds):
        logging.debug("Generating test rankings...")
        return self._provide(base_ds, self._cache_path(
            self.dataset_name, 100, self.seed, self.query_ranking_size))

    def retrieve_rankings(self, base_ds, cache_path):
        return _cached(cache_path, self.save_rankings_on_disk,
                       lambda: self.generate_rankings(
                           base_ds, invert_relation_sign=self.invert_relation_sign))

    def generate_rankings(self, base_ds_imgs_gts, invert_relation_sign=False,
                          val_rankings_per_img=100):
        """[N, val_rankings_per_img, query_ranking_size, 2] float32 (host): (index, depth) per
        list, closest first."""
        _, gts = split_base_ds(base_ds_imgs_gts)
        n, h, w = gts.shape
        idx = draw_ranking_indices(n, h * w, val_rankings_per_img, self.query_ranking_size)
        return K.depth_rankings(gts, idx, invert_relation_sign).cpu().numpy()

    @staticmethod
    def assure_no_equal_relation(distances, curr_depth, position_idx, threshold):
        no_equal_relation = True
        for i in range(position_idx):
            if get_depth_relation(distances[i], curr_depth, threshold=threshold) == 0:
                no_equal_relation = False
        return no_equal_relation
