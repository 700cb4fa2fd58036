"""Drop-in for ``pldepth/active_learning/metrics.py`` (the metrics ``PLDepth.py:189-192`` reports
after training), computed on the GPU for whole batches of images.

Same names, arguments and results as the reference:
  * ``ordinal_error(op, gt, imsize=(448, 448), num=5000)``   metrics.py:60-70
  * ``calc_err(model, test_im, test_gt, img_size=(448, 448))`` metrics.py:73-80
  * ``calcDCG(rel_list)``                                      metrics.py:83-89
  * ``calc_d(op, gt, imsize=(224, 224), list_size=200)``      metrics.py:92-109
  * ``dcg_metric(model, test_im, test_gt, list_size=200)``    metrics.py:112-120
  * ``depth_edge_metric(op, gt, imsize=(224, 224))``          metrics.py:123-144
  * ``calc_depth_metrics(model, test_im, test_gt)``           metrics.py:147-156
and, beyond the reference's module, ``ordinal_pair_error(model_or_pred, images, pairs, ...)``: the
ordinal error over the pair tables of GenericHourglassPairRelationDataProvider
(``pld_ordinal_pair_error``; pldepth_amd/test_data_eval.py reports it).
The random pixel pairs / lists are drawn on the host with the reference's exact numpy calls
(``np.random.seed(10)`` / ``np.random.seed(69)`` + ``np.random.choice(..., replace=False)``, which
also leave the global numpy RNG in the same state); the comparisons, min-max normalisation,
sorting and DCG sums run in ``pld_ordinal_error`` / ``pld_dcg_ratio``. Reference quirks kept:
``dcg_metric`` calls ``calc_d`` without ``imsize``, so lists are drawn from the first 224*224
pixels whatever the image size.

The edge metrics run one launch sequence per batch of images: ``pld_minmax_u8`` (8-bit maps),
``pld_auto_canny_u8`` (median thresholds, Canny) and ``pld_depth_edge_metric`` (chamfer distance
sums). OpenCV is not available to this build, so the 8-bit normalisation, Canny and the distance
transform are restatements of its algorithms (unpinned, like ``calc_d``'s normalisation); the
reference's own part (thresholds, the ``> 10`` cut, sums and division) is pinned by
``tests/golden/edge_golden.npz``. Reference quirks kept: the distance transform is taken of the
edge map itself (distance from an edge pixel to the nearest non-edge pixel), and a map without
edges gives nan.

The Hausdorff helpers of metrics.py:9-57, for one pair of maps of at most 32 x 32 pixels (the
tiles ``active_sampling`` hands them), run ``pld_tile_hausdorff`` with one tile:
  * ``hausdorff_distance(image0, image1)`` / ``hausdorf_dist(i1, i2)``   metrics.py:9-28
  * ``hausdorff_pair(image0, image1)``                                     metrics.py:31-57
The distance is the square root of an integer and equals the reference's; the pair equals the
reference's except where the nearest point is not unique: the reference then returns whatever
cKDTree finds first, this build the lowest row-major index.
"""
import warnings

import numpy as np
import torch

from .. import kernels as K


def _hausdorff_row(image0, image1):
    """pld_tile_hausdorff's eight numbers for one pair of (H, H) maps, H <= 32."""
    maps = []
    for im in (image0, image1):
        t = im if isinstance(im, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(im))
        if t.dim() != 2 or t.shape[0] != t.shape[1] or t.shape[0] > K.TILE_MAX:
            raise ValueError(f"hausdorff: expected a square map of at most {K.TILE_MAX} x "
                             f"{K.TILE_MAX} pixels, got {tuple(t.shape)}")
        maps.append((t != 0).to(device="cuda", dtype=torch.uint8).contiguous()[None])
    if maps[0].shape != maps[1].shape:
        raise ValueError("hausdorff: the two maps differ in size")
    return K.tile_hausdorff(maps[0], maps[1], 1)[0, 0].tolist()


def hausdorff_distance(image0, image1):
    """Hausdorff distance between the non-zero pixels of the two maps: 0 when both are empty,
    inf when one is."""
    row = _hausdorff_row(image0, image1)
    if row[0] < 0:
        return np.inf
    return 0 if row[5] == 0 else np.sqrt(float(row[0]))


def hausdorf_dist(i1, i2):
    return hausdorff_distance(i1, i2)


def hausdorff_pair(image0, image1):
    """The pair of points (one per map) that are the Hausdorff distance apart, as two int64
    (r, c) arrays; (), () with a warning when a map is empty."""
    row = _hausdorff_row(image0, image1)
    if row[7] < 0:
        warnings.warn("One or both of the images is empty.", stacklevel=2)
        return (), ()
    return np.array(row[1:3], np.int64), np.array(row[3:5], np.int64)


def _pairs(imsize, num):
    np.random.seed(10)
    idx = np.random.choice(list(range(imsize[0] * imsize[1])), num * 2, replace=False)
    idx0, idx1 = np.split(idx, 2)
    return idx0, idx1


def _list_ids(imsize, list_size):
    np.random.seed(69)
    return np.random.choice(np.arange(imsize[0] * imsize[1]), size=list_size, replace=False)


def _dev(a, dtype=torch.float32):
    if isinstance(a, torch.Tensor):
        return a.to(device="cuda", dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.float32 if dtype ==
                                                 torch.float32 else np.int32)).cuda()


def _flat(a):
    t = _dev(a)
    return t.reshape(1, -1) if t.dim() <= 3 else t.reshape(t.shape[0], -1)


def _check_ids(ids, hw, who):
    if ids.size and (ids.max() >= hw or ids.min() < 0):
        raise ValueError(f"{who}: sampled index {int(ids.max())} outside an image of {hw} pixels")


def ordinal_error(op, gt, imsize=(448, 448), num=5000):
    """1 - fraction of `num` random pixel pairs whose predicted depth order (op[a] > op[b])
    matches the ground-truth order."""
    idx0, idx1 = _pairs(imsize, num)
    p, g = _flat(op), _flat(gt)
    _check_ids(np.concatenate([idx0, idx1]), p.shape[1], "ordinal_error")
    e = K.ordinal_error(p, g, _dev(idx0, torch.int32), _dev(idx1, torch.int32))
    return float(e[0].item())


def _predict_batches(model, test_im):
    """Inference-mode predictions, device-resident, one engine batch at a time."""
    x = test_im if isinstance(test_im, torch.Tensor) else np.asarray(test_im, np.float32)
    B = model.engine.B
    for i in range(0, x.shape[0], B):
        xb = x[i:i + B]
        k = xb.shape[0]
        if k < B:  # pad the tail batch
            if isinstance(xb, torch.Tensor):
                xb = torch.cat([xb, torch.zeros((B - k,) + tuple(xb.shape[1:]), device=xb.device)])
            else:
                xb = np.concatenate([xb, np.zeros((B - k,) + tuple(xb.shape[1:]), np.float32)])
        yield i, k, model(xb, training=False)[:k]


def calc_err(model, test_im, test_gt, img_size=(448, 448)):
    """Mean ordinal error of the model's predictions over a test set."""
    idx0, idx1 = _pairs(img_size, 5000)
    i0, i1 = _dev(idx0, torch.int32), _dev(idx1, torch.int32)
    errs = []
    for i, k, pred in _predict_batches(model, test_im):
        p = pred.reshape(k, -1).contiguous()
        _check_ids(np.concatenate([idx0, idx1]), p.shape[1], "calc_err")
        g = _dev(np.asarray(test_gt[i:i + k]) if not isinstance(test_gt, torch.Tensor)
                 else test_gt[i:i + k]).reshape(k, -1)
        errs.append(K.ordinal_error(p, g, i0, i1).cpu().numpy())
    return float(np.mean(np.concatenate(errs))) if errs else float("nan")


def ordinal_pair_error(model_or_pred, images, pairs, threshold=None, invert=False):
    """The ordinal error over the pair tables of GenericHourglassPairRelationDataProvider
    (``pairs`` [N, P, 5]: point0, point1, relation, z0, z1), in ``pld_ordinal_pair_error``.

    ``model_or_pred``: a model, which then predicts ``images`` batch by batch, or the predictions
    [N, H, W(, 1)] themselves (``images`` is not read). ``threshold=None`` takes the table's
    relations; a number recomputes them from the table's depths at that threshold and ``invert``
    (the provider's ``invert_relation_sign``). Returns ``(error, per_image_error, counted)``:
    error = sum(wrong) / sum(counted) over the pairs whose relation is not 'equal', the same per
    image (nan where an image has no such pair) and the per-image counts."""
    pairs = _dev(pairs)
    if hasattr(model_or_pred, "engine"):
        wrong, counted = [], []
        for i, k, pred in _predict_batches(model_or_pred, images):
            w, c = K.ordinal_pair_error(pred.reshape(k, -1).contiguous(),
                                        pairs[i:i + k].contiguous(), threshold, invert)
            wrong.append(w)
            counted.append(c)
        if not wrong:
            return float("nan"), np.zeros(0), np.zeros(0, np.int64)
        wrong, counted = torch.cat(wrong), torch.cat(counted)
    else:
        pred = _dev(model_or_pred)
        wrong, counted = K.ordinal_pair_error(pred.reshape(pred.shape[0], -1), pairs, threshold,
                                              invert)
    wrong, counted = wrong.cpu().numpy().astype(np.int64), counted.cpu().numpy().astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        per_image = wrong / counted
        error = float(wrong.sum() / counted.sum()) if counted.sum() else float("nan")
    return error, per_image, counted


def calcDCG(rel_list):
    log_i_1 = np.log2(np.arange(np.shape(rel_list)[0]) + 2)
    return (rel_list / log_i_1).sum()


def calc_d(op, gt, imsize=(224, 224), list_size=200):
    """nDCG-style ratio of the sorted (min-max normalised) predicted depths of `list_size` random
    pixels against the sorted ground truth of the same pixels."""
    ids = _list_ids(imsize, list_size)
    p, g = _flat(op), _flat(gt)
    _check_ids(ids, p.shape[1], "calc_d")
    return float(K.dcg_ratio(p, g, _dev(ids, torch.int32))[0].item())


def dcg_metric(model, test_im, test_gt, list_size=200):
    """Mean calc_d over a test set (lists drawn from the first 224*224 pixels, as the reference's
    call without imsize does)."""
    ids = _list_ids((224, 224), list_size)
    idd = _dev(ids, torch.int32)
    out = []
    for i, k, pred in _predict_batches(model, test_im):
        p = pred.reshape(k, -1).contiguous()
        _check_ids(ids, p.shape[1], "dcg_metric")
        g = _dev(np.asarray(test_gt[i:i + k]) if not isinstance(test_gt, torch.Tensor)
                 else test_gt[i:i + k]).reshape(k, -1)
        out.append(K.dcg_ratio(p, g, idd).cpu().numpy())
    return float(np.mean(np.concatenate(out))) if out else float("nan")


def _maps(a):
    """One map as [H, W] or [H, W, 1], or a batch as [n, H, W] or [n, H, W, 1] -> [n, H, W]
    float32 device maps."""
    t = _dev(a)
    if t.dim() == 3 and t.shape[-1] == 1:
        t = t[..., 0]
    elif t.dim() == 4:
        t = t.reshape(t.shape[:3])
    return (t[None] if t.dim() == 2 else t).contiguous()


def _edge_metric_batch(p, g):
    """p, g: [n, H, W] float32 device maps -> [n, 2] float64 (boundary, completeness)."""
    e_op, _ = K.auto_canny(K.minmax_u8(p))
    e_gt, _ = K.auto_canny(K.minmax_u8(g))
    return K.depth_edge_metric(e_op, e_gt)


def depth_edge_metric(op, gt, imsize=(224, 224)):
    """(depth_boundary_error, completeness_error): both maps min-max scaled to 8 bit, their
    auto_canny edges, and the mean over one map's edge pixels of the other edge map's chamfer
    distance transform (values above 10 zeroed). `imsize` is unused, as in the reference; a map
    without edges gives nan."""
    d = _edge_metric_batch(_maps(op), _maps(gt))[0].cpu().numpy()
    return float(d[0]), float(d[1])


def calc_depth_metrics(model, test_im, test_gt):
    """Mean depth_edge_metric of the model's predictions over a test set (a plain mean: one nan
    makes the mean nan)."""
    out = []
    for i, k, pred in _predict_batches(model, test_im):
        g = _maps(np.asarray(test_gt[i:i + k]) if not isinstance(test_gt, torch.Tensor)
                  else test_gt[i:i + k])
        out.append(_edge_metric_batch(pred.reshape(g.shape).contiguous(), g).cpu().numpy())
    if not out:
        return float("nan"), float("nan")
    d = np.concatenate(out)
    return float(np.mean(d[:, 0])), float(np.mean(d[:, 1]))
