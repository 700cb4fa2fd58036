"""Drop-in for the edge detector of ``pldepth/active_learning/preprocess_utils.py``.

  * ``auto_canny(image, sigma=1.8)``   preprocess_utils.py:4-13

Canny between ``int(max(0, (1 - sigma) * median))`` and ``int(min(255, (1 + sigma) * median))``,
computed by ``pld_auto_canny_u8`` (OpenCV is not available to this build; its Canny is restated
there). The blur / sharpening / tiling helpers of the reference module feed the active-learning
pipeline and are not part of this build.
"""
import numpy as np
import torch

from .. import kernels as K


def auto_canny(image, sigma=1.8):
    """image: uint8 (H, W) array or tensor -> uint8 (H, W) edge map holding 0 / 255 (a numpy
    array for a numpy image, a device tensor for a tensor)."""
    as_numpy = not isinstance(image, torch.Tensor)
    t = torch.from_numpy(np.ascontiguousarray(image)) if as_numpy else image
    if t.dtype != torch.uint8 or t.dim() != 2:
        raise ValueError(f"auto_canny: expected a uint8 (H, W) image, got {t.dtype} "
                         f"{tuple(t.shape)}")
    edges, _ = K.auto_canny(t.cuda().contiguous()[None], sigma)
    return edges[0].cpu().numpy() if as_numpy else edges[0]
