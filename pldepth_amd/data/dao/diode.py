"""Drop-in for ``pldepth/data/dao/diode.py``: ``<root>/*/*/*/*.png`` images, each with its depth
map in ``<name>_depth.npy``. Images are resized bilinearly (tf.image.resize), depth maps with the
anti-aliased resize of skimage.transform.resize (``pld_resize_antialias``), both on the GPU.
Evaluation only: ``get_test_dataset`` returns ``(image [H, W, 3], gt [H, W])`` pairs in sorted
file order (``zip_ds=False``: the stacked arrays)."""
import glob
import os

import numpy as np

from ..data_meta import TESTING_ONLY_STR, TFDataAccessObject
from .eval_common import decode_all, resize_all, target_hw


class DIODETFDataAccessObject(TFDataAccessObject):
    def __init__(self, root_path, target_shape):
        self.root_path = root_path
        self.target_shape = target_hw(target_shape)

    def get_training_dataset(self):
        raise NotImplementedError(TESTING_ONLY_STR.format("DIODE", "training"))

    def get_validation_dataset(self):
        raise NotImplementedError(TESTING_ONLY_STR.format("DIODE", "validation"))

    def get_test_dataset(self, zip_ds=True):
        file_name_images = sorted(glob.glob(os.path.join(self.root_path, "*/*/*/*.png")))
        file_name_depths = [s.replace(".png", "_depth.npy") for s in file_name_images]

        def read_depth(file_path):
            return np.squeeze(np.load(file_path)).astype(np.float32)

        imgs = resize_all(decode_all(self.read_file_png, file_name_images), self.target_shape,
                          "bilinear")
        gts = resize_all(decode_all(read_depth, file_name_depths), self.target_shape,
                         "antialias")[..., 0]
        return list(zip(imgs, gts)) if zip_ds else (imgs, gts)
