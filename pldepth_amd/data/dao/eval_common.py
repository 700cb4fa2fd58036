"""What the evaluation-only DAOs (sintel, diode, ibims, tum) share: files are decoded on the host
in a thread pool and resized on the GPU, equal shapes batched per launch (as hr_wsi.py does)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ... import kernels as K


def target_hw(target_shape):
    shape = tuple(int(s) for s in target_shape)
    return shape[:2]


def decode_all(fn, file_names):
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        return list(ex.map(fn, file_names))


def resize_all(arrays, target_shape, method):
    """[h, w] or [h, w, c] float32 arrays -> [N, H, W, c] float32 (host). ``method``: 'bilinear'
    (tf.image.resize) or 'antialias' (skimage.transform.resize, see pld_resize_antialias)."""
    H, W = target_shape
    arrays = [np.asarray(a, np.float32) for a in arrays]
    arrays = [a[..., None] if a.ndim == 2 else a for a in arrays]
    out = np.empty((len(arrays), H, W, arrays[0].shape[-1] if arrays else 1), np.float32)
    i = 0
    while i < len(arrays):
        j = i
        while j < len(arrays) and arrays[j].shape == arrays[i].shape and j - i < 64:
            j += 1
        x = torch.from_numpy(np.stack(arrays[i:j])).cuda()
        y = K.resize_antialias(x, H, W) if method == "antialias" else K.resize(x, H, W, method)
        out[i:j] = y.cpu().numpy()
        i = j
    return out
