"""Plain-NumPy restatement of the active-learning selection pass (TEST INFRASTRUCTURE ONLY: the
yardstick of tests/test_active.py and tests/test_active_gpu.py; the product path is
pldepth_amd/csrc/active.hip).

  active_sampling, oracle            pldepth/active_learning/active_learning_method.py:12-76
  hausdorff_distance, hausdorff_pair pldepth/active_learning/metrics.py:9-57
  unsharp_mask                       pldepth/active_learning/preprocess_utils.py:16-26

The reference calls OpenCV for four operators. OpenCV is not installed here, so they are restated
from its documented algorithms and are unpinned:
  gray          cv2.cvtColor(img, COLOR_RGB2GRAY) on float32
  median_blur   cv2.medianBlur(img, ksize): replicated border
  minmax_f32    cv2.normalize(x, None, 0, 255, NORM_MINMAX) as float32 (tests/edge_ref.py)
  gaussian5     cv2.GaussianBlur(img, (5, 5), sigma): BORDER_REFLECT_101, rows then columns
The reference's own part is pinned by tests/golden/active_golden.npz
(tests/golden/make_active_golden.py), with two rules of this build where the reference leaves
the answer to a library's tie order: among several nearest points the lowest row-major index
(cKDTree returns any), and a stable np.argsort.
"""
import numpy as np

import edge_ref as R

IMG_SHAPE = [224, 224, 3]  # the reference module's img_shape (active_learning_method.py:9)


def gray(rgb):
    rgb = np.asarray(rgb, np.float32)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    return (r * np.float32(0.299) + g * np.float32(0.587)) + b * np.float32(0.114)


def median_blur(img, ksize):
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    rad = ksize // 2
    p = np.pad(img, rad, mode="edge")
    win = np.stack([p[dy:dy + h, dx:dx + w] for dy in range(ksize) for dx in range(ksize)])
    return np.sort(win, axis=0)[ksize * ksize // 2]


def gaussian_taps(sigma):
    d = np.arange(5, dtype=np.float64) - 2
    g = np.exp(-(d * d) / (2.0 * float(sigma) * float(sigma)))
    return (g / g.sum()).astype(np.float32)


def gaussian5(x, sigma):
    """Separable 5-tap Gaussian on float32, every product and sum rounded to float32, taps
    summed from the lowest index up, rows (along x) first."""
    x = np.asarray(x, np.float32)
    h, w = x.shape
    wt = gaussian_taps(sigma)
    p = np.pad(x, 2, mode="reflect")
    rows = p[:, 0:w] * wt[0]
    for k in range(1, 5):
        rows = rows + p[:, k:k + w] * wt[k]
    out = rows[0:h] * wt[0]
    for k in range(1, 5):
        out = out + rows[k:k + h] * wt[k]
    assert out.dtype == np.float32
    return out


def unsharp_mask(image, sigma=1.0, amount=3.0, blur=gaussian5):
    """preprocess_utils.py:16-22 with kernel_size (5, 5) and threshold 0, on float32."""
    image = np.asarray(image, np.float32)
    blurred = blur(image, sigma)
    sharpened = np.float32(float(amount + 1)) * image - np.float32(float(amount)) * blurred
    sharpened = np.minimum(np.maximum(sharpened, 0), 255)
    return sharpened.round().astype(np.uint8)


def unsharp_u8(x, sigma=1.0, amount=3.0):
    """What pld_unsharp_u8 computes: the 0..255 float scaling, then unsharp_mask."""
    return unsharp_mask(R.minmax_f32(x), sigma, amount)


def split_image(img, n):
    t = img.shape[0] // n
    return np.array([img[r:r + t, c:c + t] for r in range(0, img.shape[0], t)
                     for c in range(0, img.shape[1], t)])


def _nearest(p, pts):
    """(squared distance, index of the nearest of pts to p: the lowest index among equals)."""
    d2 = ((pts - p) ** 2).sum(axis=1)
    return int(d2.min()), int(np.argmin(d2))


def tile_hausdorff(a_img, b_img):
    """The eight outputs of pld_tile_hausdorff for one tile, by brute force."""
    A = np.transpose(np.nonzero(a_img)).astype(np.int64)
    B = np.transpose(np.nonzero(b_img)).astype(np.int64)
    na, nb = len(A), len(B)
    if na == 0 or nb == 0:
        return [0 if na == nb else -1, -1, -1, -1, -1, na, nb, -1]
    ab = [_nearest(a, B) for a in A]
    ba = [_nearest(b, A) for b in B]
    hab, hba = max(d for d, _ in ab), max(d for d, _ in ba)
    if hab > hba:
        ia = next(i for i, (d, _) in enumerate(ab) if d == hab)
        pin, ppred, br = A[ia], B[ab[ia][1]], 1
    else:
        ib = next(i for i, (d, _) in enumerate(ba) if d == hba)
        pin, ppred, br = A[ba[ib][1]], B[ib], 0
    return [max(hab, hba), int(pin[0]), int(pin[1]), int(ppred[0]), int(ppred[1]), na, nb, br]


def tied_inputs(a_img, b_img):
    """For a tile with both sets non-empty and branch 0: every input pixel at the nearest
    distance from the chosen prediction pixel (more than one: the reference's answer depends on
    cKDTree's tie order). None in branch 1 or with an empty set."""
    t = tile_hausdorff(a_img, b_img)
    if t[7] != 0:
        return None
    A = np.transpose(np.nonzero(a_img)).astype(np.int64)
    d2 = ((A - np.array(t[3:5])) ** 2).sum(axis=1)
    return A[d2 == d2.min()]


def tied_preds(a_img, b_img):
    """The mirror case in branch 1: every prediction pixel at the nearest distance from the
    chosen input pixel. The input pixel, the only one active_sampling uses, is not affected; the
    reference's prediction pixel is cKDTree's pick among these. None in branch 0 or with an
    empty set."""
    t = tile_hausdorff(a_img, b_img)
    if t[7] != 1:
        return None
    B = np.transpose(np.nonzero(b_img)).astype(np.int64)
    d2 = ((B - np.array(t[1:3])) ** 2).sum(axis=1)
    return B[d2 == d2.min()]


def hausdorff_table(in_edges, pred_edges, split):
    """[split^2][8] int32 for one pair of maps."""
    si, sp = split_image(in_edges, split), split_image(pred_edges, split)
    return np.array([tile_hausdorff(a, b) for a, b in zip(si, sp)], np.int32)


def nth_edge(tile, k):
    idx = np.nonzero(tile)
    return (int(idx[0][k]), int(idx[1][k])) if 0 <= k < idx[0].size else (-1, -1)


def active_sampling(in_edges, pred_edges, split_num, img_size=(224, 224, 3), in_override=None):
    """active_learning_method.py:22-56 with the rules above; draws from the global numpy RNG
    like the reference (np.random.choice per tile without a pair whose input tile has edges).
    in_override: {tile: (r, c)} input points that replace the lowest-index choice (the
    reference's own choice on a tile whose nearest input pixel is tied)."""
    si, sp = split_image(in_edges, split_num), split_image(pred_edges, split_num)
    t = si.shape[1]
    dist = np.zeros(si.shape[0])
    pts = np.zeros((si.shape[0], 2))
    for i in range(si.shape[0]):
        row = tile_hausdorff(si[i], sp[i])
        if in_override and i in in_override:
            row[1:3] = in_override[i]
        if row[7] >= 0:
            st_r = (int(i / split_num) * t) + row[1]
            st_c = int((i % split_num) * t + row[2])
            dist[i] = np.sqrt(float(row[0]))
        else:
            if row[5]:
                r, c = nth_edge(si[i], np.random.choice(row[5]))
            else:
                r, c = t / 2, t / 2
            st_r = int(i / split_num) * t + r
            st_c = int((i % split_num) * t) + c
            dist[i] = np.sqrt(2 * (IMG_SHAPE[0] / split_num) ** 2)
        pts[i] = np.array([st_r, st_c])
    idx = np.argsort(dist, kind="stable")
    dist, pts = dist[idx], pts[idx]
    pos = pts[:, 0] * img_size[0] + pts[:, 1]
    return pos.astype(np.uint32), pts.astype(np.uint32), np.mean(dist), np.var(dist)


def oracle_rows(gt, pos_xy, L, row_stride):
    """active_learning_method.py:61-76 without the shuffle (what pld_al_oracle computes)."""
    gt = np.asarray(gt, np.float32).reshape(np.shape(gt)[:2])
    P = pos_xy.shape[0]
    out = np.zeros([P // L, L, 2], np.float32)
    buf = np.zeros((L, 2))
    j = 0
    for i in range(0, P - L, L):
        for k in range(L):
            r, c = int(pos_xy[i + k, 0]), int(pos_xy[i + k, 1])
            buf[k] = (r * row_stride + c, gt[r, c])
        out[j] = buf[np.argsort(buf[:, 1], kind="stable")[::-1]]
        j += 1
    return out


def oracle(gt, pos_xy, L, img_size=(224, 224, 3)):
    """With the reference's in-place np.random.shuffle of pos_xy."""
    np.random.shuffle(pos_xy)
    return oracle_rows(gt, pos_xy, L, img_size[0])


def multiset(dist, pts):
    """(dist, r, c) rows in a canonical order: the comparison that does not depend on how a sort
    orders equal distances."""
    a = np.column_stack([np.asarray(dist, np.float64), np.asarray(pts, np.float64)])
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


# ------------------------------------------------------- fixtures and the reference comparison
FIXTURES = [(64, 4), (56, 8), (64, 8), (96, 6), (112, 16)]  # (h, split): tiles of 16, 7, 8, 16, 7


def fixture_depths(s):
    """(input map, prediction map) float32 (h, h) of seeded fixture s."""
    h, _ = FIXTURES[s]
    gt = R.scene(h, h, 100 + s)[..., 0]
    rng = np.random.default_rng(s)
    pred = np.roll(gt, 2, axis=1) + 0.02 * rng.standard_normal((h, h)).astype(np.float32)
    return gt, pred.astype(np.float32)


def fixture_edges(s):
    gt, pred = fixture_depths(s)
    return R.auto_canny(R.minmax_u8(gt)), R.auto_canny(R.minmax_u8(pred))


def handmade_edges():
    """Two pairs of 64 x 64 maps, split 2 (tiles of 32). Pair 0: an all-empty tile, an input-only
    tile, a prediction-only tile, and a single input pixel against a full 32 x 32 prediction
    tile. Pair 1: full against full, a full input tile against one prediction pixel, a diagonal
    against a column, and one pixel each in the far corners."""
    a = np.zeros((2, 64, 64), np.uint8)
    b = np.zeros((2, 64, 64), np.uint8)
    a[0, 3:9, 40] = 255              # tile 1: input only
    b[0, 50, 2:30] = 255             # tile 2: prediction only
    a[0, 40, 50] = 255               # tile 3: one input pixel against a full prediction tile
    b[0, 32:, 32:] = 255
    a[1, :32, :32] = 255             # tile 0: full against full
    b[1, :32, :32] = 255
    a[1, :32, 32:] = 255             # tile 1: full input against one prediction pixel
    b[1, 10, 32 + 21] = 255
    for i in range(32):              # tile 2: a diagonal against a column
        a[1, 32 + i, i] = 255
    b[1, 32:, 16] = 255
    a[1, 32 + 31, 32 + 31] = 255     # tile 3: one pixel each, the far corners
    b[1, 32, 32] = 255
    return a, b


def fixtures():
    """(input edges, prediction edges, split) of every golden fixture, in the golden's order."""
    out = [fixture_edges(s) + (FIXTURES[s][1],) for s in range(len(FIXTURES))]
    ha, hb = handmade_edges()
    return out + [(ha[k], hb[k], 2) for k in range(len(ha))]


def waived_tiles(e_in, e_pred, split, pair):
    """{tile: the reference's input point} for the tiles whose nearest input pixel is tied; the
    reference's point must be one of the tied pixels."""
    si, sp = split_image(e_in, split), split_image(e_pred, split)
    out = {}
    for i in range(len(si)):
        tied = tied_inputs(si[i], sp[i])
        if tied is not None and len(tied) > 1:
            assert any(np.array_equal(pair[i, :2], p) for p in tied), (i, pair[i], tied)
            out[i] = (int(pair[i, 0]), int(pair[i, 1]))
    return out


def check_table(table, e_in, e_pred, split, hd2, pair):
    """A [P][8] tile table against the reference's per-tile results under the waiver: the
    squared distance on every tile; the input point on every tile whose nearest input pixel is
    unique (branch 1: always) and inside the tied set otherwise. The prediction point, which
    active_sampling does not use, is the mirror image: in branch 1 it is the nearest prediction
    pixel of the input point, equal where that is unique and inside its tied set otherwise."""
    waived = waived_tiles(e_in, e_pred, split, pair)
    si, sp = split_image(e_in, split), split_image(e_pred, split)
    assert np.array_equal(table[:, 0], hd2)
    for i in range(len(table)):
        if i not in waived:
            assert np.array_equal(table[i, 1:3], pair[i, :2]), (i, table[i], pair[i])
        tied = tied_preds(si[i], sp[i])
        if tied is not None and len(tied) > 1:
            assert any(np.array_equal(pair[i, 2:], p) for p in tied), (i, pair[i], tied)
        else:
            assert np.array_equal(table[i, 3:5], pair[i, 2:]), (i, table[i], pair[i])
    return waived
