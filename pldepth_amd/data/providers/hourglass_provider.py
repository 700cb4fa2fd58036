"""Training / validation batch provider (mirrors pldepth/data/providers/hourglass_provider.py).

The reference builds a tf.data pipeline: zip(img, mask, gt) -> random joint horizontal flip ->
shuffle(1024) -> tf.numpy_function(sampler) per image -> batch(drop_remainder) -> prefetch ->
repeat (provide_train_dataset, :29-62), and pre-generates validation rankings once with the
Thresholded sampler (provide_val_dataset / generate_validation_rankings, :64-73, :179-193).

Here the datasets are in-memory arrays (images [N,H,W,3] in [0,1], gts [N,H,W], masks [N,H,W]);
flips and shuffling are host index work, and the rankings of a whole batch come from ONE GPU
sampler launch (Philox draws keyed by seed / batch counter / image position) instead of a
per-image Python call under the GIL. Batches are (x [B,H,W,3], y [B,R,L,2]) device tensors.

With ``device_resident=True`` the arrays are uploaded once and the gather and flip of a batch are
one kernel as well (pld_batch_gather_flip); the host keeps only the index work. Consistency masks
of another resolution than the images (the sampler scales their positions, sampling.py:125-129)
take a second launch of that kernel.

``sampling_eq_threshold`` is the training sampler's tau; the validation sampler keeps the default
0.03, as in the reference (:21-22).

Data parallel (``rank``, ``world``): ``batch_size`` stays the per-replica batch B and the global
batch is G = world * B. Every rank holds the whole dataset and runs the same host RNG stream; rank
r takes images [r*B, (r+1)*B) of each global batch (dp.shard's layout) and samples them with
``image_offset = r*B``, so its (x, y) are, bit for bit, that slice of what one process with batch
G produces.
"""
import numpy as np
import torch

from ... import kernels as K
from ..sampling import ThresholdedMaskedRandomSamplingStrategy


UPLOAD_CHUNK = 256  # images per host-to-device copy of a resident dataset


def _resident(arrays, dev):
    """float32 device copies of the host arrays, uploaded UPLOAD_CHUNK images at a time so the
    host never holds a second full-size (converted / contiguous) copy. All or nothing: when the
    device runs out of memory what was uploaded is freed and MemoryError raised."""
    need = sum(int(np.prod(a.shape)) * 4 for a in arrays)
    out = []
    try:
        for a in arrays:
            t = torch.empty(tuple(a.shape), dtype=torch.float32, device=dev)
            out.append(t)
            for i in range(0, len(a), UPLOAD_CHUNK):
                t[i:i + UPLOAD_CHUNK].copy_(torch.from_numpy(
                    np.ascontiguousarray(a[i:i + UPLOAD_CHUNK], np.float32)))
    except torch.cuda.OutOfMemoryError:
        del out[:]
        t = None
        torch.cuda.empty_cache()
        raise MemoryError(
            f"device_resident=True needs {need} bytes of device memory for the dataset and "
            f"{torch.cuda.mem_get_info(dev)[0]} are free; device_resident=False keeps the "
            "dataset on the host") from None
    return out


def _epoch_batches(rng, n, B, world=1, rank=0, augment=False):
    """One epoch's index work: yields (idx [B], flip [B] bool or None) per global batch, rank
    ``rank``'s slice of it. The draws from ``rng`` do not depend on the rank: one permutation of
    the n images, then per global batch of G = world * B one flip draw of G when augmenting
    (drop_remainder: the last n % G images of the permutation are not used)."""
    G = world * B
    lo = rank * B
    order = rng.permutation(n)
    for i in range(0, n - G + 1, G):
        flip = rng.random(G) > 0.5 if augment else None
        yield order[i + lo:i + lo + B], None if flip is None else flip[lo:lo + B]


class HourglassLargeScaleDataProvider(object):
    """``device_resident=True``: the datasets are uploaded once, when provide_*_dataset is
    called, and every training batch is gathered (and flipped) on the device by
    kernels.batch_gather_flip: the same batches, bit for bit, as the host path for a seed."""

    def __init__(self, model_params, train_consistency_masks, val_consistency_masks,
                 loss_type=None, augmentation=False, sampling_eq_threshold=0.03, bs_factor=5,
                 seed=0, rank=0, world=1, device_resident=False):
        if not 0 <= rank < world:
            raise ValueError(f"rank {rank} outside a world of {world}")
        self.model_params = model_params
        self.train_consistency_masks = np.asarray(train_consistency_masks, np.float32)
        self.val_consistency_masks = (None if val_consistency_masks is None else
                                      np.asarray(val_consistency_masks, np.float32))
        self.random_sampler = ThresholdedMaskedRandomSamplingStrategy(model_params,
                                                                     sampling_eq_threshold)
        self.val_random_sampler = ThresholdedMaskedRandomSamplingStrategy(model_params)
        self.augmentation = augmentation
        self.loss_type = loss_type
        self.bs_factor = bs_factor
        self.seed = seed
        self.rank, self.world = rank, world
        self.device_resident = device_resident

    def provide_train_dataset(self, base_ds, base_ds_gts=None):
        if self.device_resident:
            dev = torch.device("cuda", torch.cuda.current_device())
            return _ResidentTrainIterable(self, *_resident(
                [np.asarray(base_ds), np.asarray(base_ds_gts), self.train_consistency_masks], dev))
        return _TrainIterable(self, np.asarray(base_ds, np.float32),
                              np.asarray(base_ds_gts, np.float32))

    def provide_val_dataset(self, base_ds, base_ds_gts=None):
        B = self.model_params.get_parameter("batch_size")
        R = self.model_params.get_parameter("val_rankings_per_img")
        G, lo = self.world * B, self.rank * B  # global batches of G; this rank's B of each
        dev = torch.device("cuda", torch.cuda.current_device())
        batches = []
        if self.device_resident:  # one upload of the full batches; x is a slice of it
            n = len(base_ds) // G * G
            imgs, gts, masks = _resident([np.asarray(base_ds)[:n], np.asarray(base_ds_gts)[:n],
                                          self.val_consistency_masks[:n]], dev)
            for i in range(lo, n, G):
                y = self.val_random_sampler.sample_batch_gpu(
                    gts[i:i + B], masks[i:i + B], R, seed=self.seed + 7919, step=0,
                    image_offset=i)
                batches.append((imgs[i:i + B], y))
            return batches
        imgs = np.asarray(base_ds, np.float32)
        gts = np.asarray(base_ds_gts, np.float32)
        for i in range(lo, len(imgs) - G + lo + 1, G):  # batch(drop_remainder=True) + cache()
            y = self.val_random_sampler.sample_batch_gpu(
                torch.from_numpy(gts[i:i + B]).to(dev),
                torch.from_numpy(self.val_consistency_masks[i:i + B]).to(dev), R,
                seed=self.seed + 7919, step=0, image_offset=i)
            batches.append((torch.from_numpy(imgs[i:i + B]).to(dev), y))
        return batches


class _ResidentTrainIterable(object):
    """_TrainIterable over device tensors: the same host RNG stream (one permutation per epoch,
    one flip draw per batch) and sampler step counter, the batch from one gather kernel."""

    def __init__(self, prov, imgs, gts, masks):
        self.p, self.imgs, self.gts, self.masks = prov, imgs, gts, masks

    def __iter__(self):
        p = self.p
        B = p.model_params.get_parameter("batch_size")
        R = p.model_params.get_parameter("rankings_per_image")
        strategy = p.model_params.get_parameter("sampling_strategy") or p.random_sampler
        rng = np.random.default_rng(p.seed)
        n = len(self.imgs)
        step = 0
        own_grid = self.masks.shape[1:] != self.gts.shape[1:]  # masks of another resolution
        while True:  # repeat()
            for idx, flip in _epoch_batches(rng, n, B, p.world, p.rank, p.augmentation):
                if own_grid:  # gathered and flipped by a call of their own, as 1-channel images
                    x, g, _ = K.batch_gather_flip(self.imgs, self.gts, None, idx, flip)
                    m = K.batch_gather_flip(self.masks.unsqueeze(-1), None, None, idx,
                                            flip)[0].squeeze(-1)
                else:
                    x, g, m = K.batch_gather_flip(self.imgs, self.gts, self.masks, idx, flip)
                y = strategy.sample_batch_gpu(g, m, R, seed=p.seed, step=step,
                                              image_offset=p.rank * B)
                step += 1
                yield x, y


class _TrainIterable(object):
    def __init__(self, prov, imgs, gts):
        self.p, self.imgs, self.gts = prov, imgs, gts
        self.masks = prov.train_consistency_masks

    def __iter__(self):
        p = self.p
        B = p.model_params.get_parameter("batch_size")
        R = p.model_params.get_parameter("rankings_per_image")
        strategy = p.model_params.get_parameter("sampling_strategy") or p.random_sampler
        rng = np.random.default_rng(p.seed)
        dev = torch.device("cuda", torch.cuda.current_device())
        n = len(self.imgs)
        step = 0
        while True:  # repeat()
            for idx, flip in _epoch_batches(rng, n, B, p.world, p.rank, p.augmentation):
                x, g, m = self.imgs[idx], self.gts[idx], self.masks[idx]
                if flip is not None:  # joint random horizontal flip, p = 0.5 (:35-49)
                    x = np.where(flip[:, None, None, None], x[:, :, ::-1], x)
                    g = np.where(flip[:, None, None], g[:, :, ::-1], g)
                    m = np.where(flip[:, None, None], m[:, :, ::-1], m)
                gd = torch.from_numpy(np.ascontiguousarray(g)).to(dev)
                md = torch.from_numpy(np.ascontiguousarray(m)).to(dev)
                y = strategy.sample_batch_gpu(gd, md, R, seed=p.seed, step=step,
                                              image_offset=p.rank * B)
                step += 1
                yield torch.from_numpy(np.ascontiguousarray(x)).to(dev), y
