"""Drop-in for ``pldepth/data/dao/tum.py``: ``<root>/*.h5`` files with the image in
``gt/img_1`` and the depth in ``gt/pp_depth``, read through the in-tree HDF5 reader
(util/hdf5.py; a layout it does not read raises its NotImplementedError). Both go through the
anti-aliased resize of skimage.transform.resize on the GPU (``pld_resize_antialias``).
Evaluation only: ``get_test_dataset`` returns ``(image [H, W, 3], gt [H, W])`` pairs in sorted
file order (``zip_ds=False``: the stacked arrays)."""
import glob
import os

import numpy as np

from ...util import hdf5
from ..data_meta import TESTING_ONLY_STR, TFDataAccessObject
from .eval_common import decode_all, resize_all, target_hw


class TUMTFDataAccessObject(TFDataAccessObject):
    def __init__(self, root_path, target_shape):
        self.root_path = root_path
        self.target_shape = target_hw(target_shape)

    def get_training_dataset(self):
        raise NotImplementedError(TESTING_ONLY_STR.format("TUM", "training"))

    def get_validation_dataset(self):
        raise NotImplementedError(TESTING_ONLY_STR.format("TUM", "validation"))

    @staticmethod
    def read_h5(file_path):
        h5_file = hdf5.load(file_path)
        image = np.asarray(h5_file["gt/img_1"].data, np.float32)
        gt = np.asarray(h5_file["gt/pp_depth"].data, np.float32)  # tum.py:31: not the raw depth
        return image, gt

    def get_test_dataset(self, zip_ds=True):
        raw = decode_all(self.read_h5, sorted(glob.glob(os.path.join(self.root_path, "*.h5"))))
        imgs = resize_all([r[0] for r in raw], self.target_shape, "antialias")
        gts = resize_all([r[1] for r in raw], self.target_shape, "antialias")[..., 0]
        return list(zip(imgs, gts)) if zip_ds else (imgs, gts)
