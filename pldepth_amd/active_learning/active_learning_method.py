"""Drop-in for ``pldepth/active_learning/active_learning_method.py``: the selection pass of the
active-learning round (run_scripts/active_PLDepth.py:160-185), on the GPU for whole batches of
images.

Same names, arguments and results as the reference:
  * ``get_edge_pixel(img)``                                            :12-20
  * ``active_sampling(in_edges, pred_edges, split_num, img_size)``     :22-56
  * ``oracle(img, img_gts, pos_xy, ranking_size, img_size)``           :59-76
  * ``active_learning_data_provider(img_arr, img_gts_arr, model, batch_size, ranking_size=6,
    split_num=32, sigma=1.8, img_size)``                               :79-119
Behind them sits one batched path, ``select_batch``: gray -> 8-bit min-max -> median 15 ->
``auto_canny(1.8)`` for the input image, ``unsharp`` -> ``auto_canny(sigma)`` for the prediction,
one ``pld_tile_hausdorff`` over every tile of every image, the table's trip to the host for the
random draws, ``pld_tile_nth_edge`` for the drawn pixels (their coordinates come back for the
host's sort), the host shuffle, and ``pld_al_oracle``.

Randomness stays on the host, with the reference's own calls in the reference's order: per image,
tiles in order, ``np.random.choice(n_in)`` only for a tile without a Hausdorff pair whose input
tile has edges; then ``np.random.shuffle`` for that image's points. Given the same edge maps the
global numpy RNG ends in the reference's state.

Reference quirks kept: the fallback distance ``sqrt(2 * (224 / split_num)^2)`` uses the module's
``img_shape``, not the image at hand; the fallback point of an input tile without edges is the
float ``(t / 2, t / 2)``; ``pos`` is computed from the float points before the ``uint32`` cast;
the oracle's loop stops at ``P - L``, so with ``L`` dividing ``P`` the last ranking stays zero.

Two rules are this build's where the reference leaves the answer to a library: several nearest
pixels resolve to the lowest row-major index (pld_tile_hausdorff), and the points are ordered by
``np.argsort(dist, kind="stable")`` (the reference's default sort orders equal distances
differently from one numpy build to the next).

wandb is optional: the statistics are logged through it only when it is importable and a run is
active, and are always kept on the returned dataset (``.hd_mean``, ``.hd_var``).
"""
import warnings

import numpy as np
import torch

from .. import kernels as K
from .metrics import _predict_batches

img_shape = [224, 224, 3]


def _wandb_log(values):
    try:
        import wandb
    except ImportError:
        return
    if getattr(wandb, "run", None) is not None:
        wandb.log(values)


def _edges_dev(a):
    """One (H, W) map or a batch [n, H, W], numpy or tensor -> [n, H, W] uint8 device maps."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    t = t.to(device="cuda")
    t = t if t.dtype == torch.uint8 else (t != 0).to(torch.uint8)
    return (t[None] if t.dim() == 2 else t).contiguous()


def _tile_side(h, w, split_num):
    t = int(h / split_num)
    if h != w or t * split_num != h or t > K.TILE_MAX:
        raise ValueError(f"active sampling: a {h} x {w} map in {split_num} x {split_num} tiles "
                         f"(square maps, equal tiles of at most {K.TILE_MAX} pixels a side)")
    return t


def get_edge_pixel(img):
    """A random non-zero pixel (r, c) of the tile, or its centre (x / 2, y / 2) as floats when
    it has none."""
    x, y = img.shape
    e = _edges_dev(img)
    n = int(torch.count_nonzero(e))
    if n != 0:
        _tile_side(x, y, 1)
        k = torch.tensor([[int(np.random.choice(n))]], dtype=torch.int32, device="cuda")
        rc = torch.full((1, 1, 2), -1, dtype=torch.int32, device="cuda")
        r, c = K.tile_nth_edge(e, 1, k, rc)[0, 0].tolist()
        return r, c
    return x / 2, y / 2


def _draw_tiles(table):
    """One image's draws, tiles in order: k[tile] = np.random.choice(n_in) for a tile without a
    pair whose input tile has edges, -1 elsewhere."""
    k = np.full(table.shape[0], -1, np.int32)
    for i in np.nonzero((table[:, 7] < 0) & (table[:, 5] > 0))[0]:
        k[i] = np.random.choice(int(table[i, 5]))
    return k


def _assemble(table, rc, split_num, t, img_size):
    """active_learning_method.py:28-56 for one image from its tile table [P, 8] and the drawn
    pixels rc [P, 2]: (pos, pts, mean, var)."""
    P = table.shape[0]
    i = np.arange(P)
    origin = np.stack([(i // split_num) * t, (i % split_num) * t], 1)
    has = table[:, 7] >= 0
    if not has.all():
        warnings.warn("One or both of the images is empty.", stacklevel=3)
    dist = np.where(has, np.sqrt(np.maximum(table[:, 0], 0).astype(np.float64)),
                    np.sqrt(2 * (img_shape[0] / split_num) ** 2))
    local = np.where(has[:, None], table[:, 1:3],
                     np.where((table[:, 5] > 0)[:, None], rc, t / 2)).astype(np.float64)
    pts = origin + local
    idx = np.argsort(dist, kind="stable")
    dist, pts = dist[idx], pts[idx]
    pos = pts[:, 0] * img_size[0] + pts[:, 1]
    mean, var = np.mean(dist), np.var(dist)
    _wandb_log({'hausdorf_dist_mean': mean, 'hausdorf_dist_variance': var})
    return pos.astype(np.uint32), pts.astype(np.uint32), mean, var


def _sample_batch(in_edges, pred_edges, split_num, img_size, shuffle):
    """in_edges, pred_edges: [n, H, H] uint8 device maps -> per image (pos, pts, mean, var), and
    with `shuffle` the oracle's permutation of the points, drawn right after the image's own
    draws as the reference's provider does."""
    n, h, w = in_edges.shape
    t = _tile_side(h, w, split_num)
    P = split_num * split_num
    table = K.tile_hausdorff(in_edges, pred_edges, split_num).cpu().numpy()
    k = np.empty((n, P), np.int32)
    perms = []
    for i in range(n):
        k[i] = _draw_tiles(table[i])
        if shuffle:
            perm = np.zeros((P, 2), np.int64)  # two columns: np.random.shuffle's path for pos_xy
            perm[:, 0] = np.arange(P)
            np.random.shuffle(perm)
            perms.append(perm[:, 0])
    rc = np.full((n, P, 2), -1, np.int32)
    if (k >= 0).any():
        rc_dev = torch.from_numpy(rc).cuda()
        rc = K.tile_nth_edge(in_edges, split_num, torch.from_numpy(k).cuda(), rc_dev).cpu().numpy()
    return [_assemble(table[i], rc[i], split_num, t, img_size) for i in range(n)], perms


def active_sampling(in_edges, pred_edges, split_num, img_size=[224, 224, 3]):
    """The edge maps of the input image and of the predicted depth map, cut into split_num x
    split_num tiles: per tile the input-edge pixel of the tile's Hausdorff pair (a random input
    edge pixel, or the tile centre, where there is no pair), ordered by the tile's Hausdorff
    distance (``np.argsort(dist, kind="stable")``) -> (pos, pos_xy, mean, variance)."""
    out, _ = _sample_batch(_edges_dev(in_edges), _edges_dev(pred_edges), split_num, img_size,
                           shuffle=False)
    return out[0]


def _gt_maps(gts, n):
    g = gts if isinstance(gts, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(np.asarray(gts, np.float32)))
    g = g.to(device="cuda", dtype=torch.float32)
    if g.dim() == 4 or (g.dim() == 3 and n == 1 and g.shape[-1] == 1):  # a trailing channel axis
        g = g[..., 0]
    return (g[None] if g.dim() == 2 else g).contiguous()


def oracle(img, img_gts, pos_xy, ranking_size, img_size=[224, 224, 3]):
    """Shuffles pos_xy (in place, like the reference) and ranks every group of ranking_size
    points by ground-truth depth, deepest first -> [P // L, L, 2] float32 (flat index, depth)."""
    np.random.shuffle(pos_xy)
    pts = torch.from_numpy(np.ascontiguousarray(pos_xy).astype(np.int32)).cuda()[None]
    return K.al_oracle(_gt_maps(img_gts, 1), pts, ranking_size, img_size[0])[0].cpu().numpy()


def input_edges(imgs):
    """imgs [n, H, W, 3] float32 device tensor -> the reference's input edge maps
    (active_learning_method.py:94-98)."""
    return K.auto_canny(K.median_blur(K.minmax_u8(K.gray(imgs)), 15), 1.8)[0]


def prediction_edges(preds, sigma=1.8):
    """preds [n, H, W] float32 device tensor -> the reference's prediction edge maps
    (active_learning_method.py:102-105)."""
    return K.auto_canny(K.unsharp(preds), sigma)[0]


def select_batch(imgs, gts, preds, ranking_size=6, split_num=32, sigma=1.8,
                 img_size=[224, 224, 3]):
    """One selection pass for n images: imgs [n, H, W, 3], gts [n, H, W(, 1)] and the model's
    predictions preds [n, H, W(, 1)] (host or device) -> (y [n, P // L, L, 2] device rankings,
    per-image Hausdorff mean list, variance list)."""
    x = torch.as_tensor(imgs, dtype=torch.float32).cuda().contiguous()
    n, h, w = x.shape[:3]
    p = torch.as_tensor(preds, dtype=torch.float32).cuda().reshape(n, h, w).contiguous()
    out, perms = _sample_batch(input_edges(x), prediction_edges(p, sigma), split_num, img_size,
                               shuffle=True)
    pos_xy = np.stack([o[1][perm] for o, perm in zip(out, perms)]).astype(np.int32)
    y = K.al_oracle(_gt_maps(gts, n), torch.from_numpy(pos_xy).cuda(), ranking_size, img_size[0])
    return y, [o[2] for o in out], [o[3] for o in out]


class ActiveDataset(object):
    """The provider's result: a re-iterable, repeating sequence of (x [B, H, W, 3],
    y [B, P // L, L, 2]) device batches (tf.data's zip().batch(drop_remainder=True).repeat()),
    with the per-image Hausdorff statistics of the pass."""

    def __init__(self, x, y, batch_size, hd_mean, hd_var):
        self.x, self.y, self.batch_size = x, y, batch_size
        self.hd_mean, self.hd_var = hd_mean, hd_var

    def __len__(self):
        return self.x.shape[0] // self.batch_size

    def __iter__(self):
        B = self.batch_size
        while len(self):
            for i in range(len(self)):
                yield self.x[i * B:(i + 1) * B], self.y[i * B:(i + 1) * B]


def active_learning_data_provider(img_arr, img_gts_arr, model, batch_size, ranking_size=6,
                                  split_num=32, sigma=1.8, img_size=[224, 224, 3]):
    """img_arr / img_gts_arr: the pool's images and ground truths (lists or arrays). Predicts
    every image with the model's inference forward (one engine batch at a time), selects
    split_num^2 pixels per image and lets the oracle rank them -> ActiveDataset."""
    imgs = img_arr if isinstance(img_arr, torch.Tensor) else np.asarray(img_arr, np.float32)
    gts = img_gts_arr if isinstance(img_gts_arr, torch.Tensor) else np.asarray(img_gts_arr,
                                                                                np.float32)
    xs, ys, stat_mean, stat_var = [], [], [], []
    for i, k, pred in _predict_batches(model, imgs):
        x = torch.as_tensor(imgs[i:i + k], dtype=torch.float32).cuda()
        y, m, v = select_batch(x, gts[i:i + k], pred, ranking_size, split_num, sigma, img_size)
        xs.append(x)
        ys.append(y)
        stat_mean += m
        stat_var += v
    _wandb_log({'avg_hd_mean': np.mean(stat_mean), 'avg_hd_var': np.mean(stat_var)})
    return ActiveDataset(torch.cat(xs), torch.cat(ys), batch_size, stat_mean, stat_var)
