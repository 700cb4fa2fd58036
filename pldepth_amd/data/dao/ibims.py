"""Drop-in for ``pldepth/data/dao/ibims.py``: ``<root>/*.mat`` files whose ``data`` struct holds
the RGB image (field 2; 8-bit values are scaled to [0, 1] as skimage does) and the depth map
(field 3). Both go through the anti-aliased resize of skimage.transform.resize on the GPU
(``pld_resize_antialias``). scipy reads the files and is imported when the first one is read.
Evaluation only: ``get_test_dataset`` returns ``(image [H, W, 3], gt [H, W])`` pairs in sorted
file order (``zip_ds=False``: the stacked arrays)."""
import glob
import os

import numpy as np

from ..data_meta import TESTING_ONLY_STR, TFDataAccessObject
from .eval_common import decode_all, resize_all, target_hw


class IbimsTFDataAccessObject(TFDataAccessObject):
    def __init__(self, root_path, target_shape):
        self.root_path = root_path
        self.target_shape = target_shape
        self.file_names = sorted(glob.glob(os.path.join(self.root_path, "*.mat")))

    @staticmethod
    def read_raw_mat(file_path):
        """(rgb [h, w, 3] in [0, 1], depth [h, w]) float32, not yet resized."""
        from scipy import io
        raw_data = io.loadmat(file_path)["data"]
        image, gt = raw_data[0][0][2], raw_data[0][0][3]
        if image.dtype == np.uint8:
            image = image.astype(np.float32) / np.float32(255.0)
        return np.asarray(image, np.float32), np.asarray(gt, np.float32)

    def get_training_dataset(self):
        raise NotImplementedError(TESTING_ONLY_STR.format("Ibims", "training"))

    def get_validation_dataset(self):
        raise NotImplementedError(TESTING_ONLY_STR.format("Ibims", "validation"))

    def get_test_dataset(self, zip_ds=True):
        raw = decode_all(self.read_raw_mat, self.file_names)
        hw = target_hw(self.target_shape)
        imgs = resize_all([r[0] for r in raw], hw, "antialias")
        gts = resize_all([r[1] for r in raw], hw, "antialias")[..., 0]
        return list(zip(imgs, gts)) if zip_ds else (imgs, gts)
