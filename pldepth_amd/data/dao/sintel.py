"""Drop-in for ``pldepth/data/dao/sintel.py``: ``<root>/images/*/*.png`` with the depth
visualisations under ``depth_viz`` at the same relative path (one channel, scaled back to
0..255). Both are resized bilinearly on the GPU (tf.image.resize, ``pld_resize_bilinear``).
Evaluation only: ``get_test_dataset`` returns ``(image [H, W, 3], gt [H, W])`` pairs in sorted
file order (``zip_ds=False``: the stacked arrays), like HR-WSI's."""
import glob
import os

import numpy as np

from ..data_meta import TESTING_ONLY_STR, TFDataAccessObject
from .eval_common import decode_all, resize_all, target_hw


class SintelTFDataAccessObject(TFDataAccessObject):
    def __init__(self, root_path, target_shape):
        self.root_path = root_path
        self.target_shape = target_hw(target_shape)

    def get_training_dataset(self):
        raise NotImplementedError(TESTING_ONLY_STR.format("Sintel", "training"))

    def get_validation_dataset(self):
        raise NotImplementedError(TESTING_ONLY_STR.format("Sintel", "validation"))

    def get_test_dataset(self, zip_ds=True):
        file_names_imgs = sorted(glob.glob(os.path.join(self.root_path, "images/*/*.png")))
        file_names_gts = [s.replace("/images/", "/depth_viz/") for s in file_names_imgs]

        def png_fn(file):
            return self.read_file_png(file, num_channels=1) * np.float32(255.)

        imgs = resize_all(decode_all(self.read_file_png, file_names_imgs), self.target_shape,
                          "bilinear")
        gts = resize_all(decode_all(png_fn, file_names_gts), self.target_shape,
                         "bilinear")[..., 0]
        return list(zip(imgs, gts)) if zip_ds else (imgs, gts)
