"""Drop-in for ``pldepth/active_learning/preprocess_utils.py``.

  * ``auto_canny(image, sigma=1.8)``                              preprocess_utils.py:4-13
  * ``unsharp_mask(image, kernel_size=(5, 5), sigma=1.0, amount=3.0, threshold=0)``   :16-26
  * ``splitImage(img, n=32)``                                     :29-42

Canny between ``int(max(0, (1 - sigma) * median))`` and ``int(min(255, (1 + sigma) * median))``,
computed by ``pld_auto_canny_u8`` (OpenCV is not available to this build; its Canny is restated
there). ``unsharp_mask`` runs ``pld_unsharp_u8`` (a restated 5 x 5 ``cv2.GaussianBlur``, then the
reference's own arithmetic) on the image as it is; the batched selection path has the same kernel
also perform the 0..255 min-max scaling the reference applies just before
(active_learning_method.py:103). ``splitImage`` is a host reshape.
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


def unsharp_mask(image, kernel_size=(5, 5), sigma=1.0, amount=3.0, threshold=0):
    """image: float (H, W) array or tensor with values in 0..255 (the output of
    cv2.normalize(pred, None, 0, 255, NORM_MINMAX), as the reference passes it) -> uint8 (H, W)
    sharpened image: (amount + 1) * image - amount * GaussianBlur(image), clamped to 0..255 and
    rounded. Only the reference's own call is built: kernel_size (5, 5), threshold 0."""
    if tuple(kernel_size) != (5, 5):
        raise NotImplementedError(f"unsharp_mask: kernel_size {tuple(kernel_size)} (only (5, 5), "
                                  "the reference's call, is built)")
    if threshold > 0:
        raise NotImplementedError("unsharp_mask: threshold > 0 (the reference never passes it)")
    as_numpy = not isinstance(image, torch.Tensor)
    t = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)) if as_numpy else image
    if t.dim() != 2 or not t.is_floating_point():
        raise ValueError(f"unsharp_mask: expected a float (H, W) image, got {t.dtype} "
                         f"{tuple(t.shape)}")
    out = K.unsharp(t.to(device="cuda", dtype=torch.float32).contiguous()[None], sigma, amount,
                    normalize=False)
    return out[0].cpu().numpy() if as_numpy else out[0]


def splitImage(img, n=32):
    """img (H, W) cut into n x n pieces of int(H / n) pixels a side -> [n * n, t, t] in row-major
    tile order (a view-based reshape; H and W must be multiples of n, as in every reference
    call)."""
    t = int(img.shape[0] / n)
    if t * n != img.shape[0] or t * n != img.shape[1]:
        raise ValueError(f"splitImage: a {tuple(img.shape[:2])} image does not split into "
                         f"{n} x {n} equal tiles")
    tiles = img.reshape(n, t, n, t)
    if isinstance(img, torch.Tensor):
        return tiles.permute(0, 2, 1, 3).reshape(n * n, t, t)
    return np.ascontiguousarray(tiles.transpose(0, 2, 1, 3)).reshape(n * n, t, t)
