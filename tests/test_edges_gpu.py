"""Depth-edge metric on the GPU: every stage of pldepth_amd/csrc/edges.hip against the NumPy
yardstick (tests/edge_ref.py), bit for bit, then the reference-shaped API. Everything after the
8-bit conversion is integer arithmetic and the conversion rounds like NumPy's, so the
comparisons are exact (== on the final doubles, nan matching nan)."""
import math

import numpy as np
import pytest

import edge_ref as R

pytestmark = pytest.mark.gpu


def _pair(h, w, seed):
    gt = R.scene(h, w, seed)[..., 0]
    rng = np.random.default_rng(seed + 1000)
    op = np.roll(gt, 1, axis=1) + 0.01 * rng.standard_normal((h, w)).astype(np.float32)
    return op.astype(np.float32)[None], gt[None]


def _step(col, h=12, w=16):
    a = np.zeros((1, h, w), np.float32)
    a[..., col:] = 200
    return a


def _batch3():
    op, gt = _pair(40, 56, 5)
    op2, gt2 = _pair(40, 56, 6)
    const = np.full((1, 40, 56), -2.5, np.float32)
    return np.concatenate([op, const, op2]), np.concatenate([gt, gt2, const])


CASES = {
    "step12x16": lambda: (_step(8), _step(8)),
    "33x47": lambda: _pair(33, 47, 1),
    "64x64": lambda: _pair(64, 64, 2),
    "batch3_const": _batch3,
    "224x224": lambda: _pair(224, 224, 3),
    "448x448": lambda: _pair(448, 448, 4),
}
_REF = {}


def _reference(name):
    """Inputs and every stage of the yardstick for one case, computed once."""
    if name not in _REF:
        op, gt = CASES[name]()
        r = {"op": op, "gt": gt}
        for k, x in (("op", op), ("gt", gt)):
            r[k + "_u8"] = np.stack([R.minmax_u8(a) for a in x])
            r[k + "_thr"] = np.array([R.auto_thresholds(a) for a in r[k + "_u8"]], np.int32)
            r[k + "_E"] = np.stack([R.auto_canny(a) for a in r[k + "_u8"]])
            r[k + "_dt"] = np.stack([R.chamfer_dt3(a) for a in r[k + "_E"]])
        r["metric"] = np.array([R.metric_exact_from_edges(a, b)
                                for a, b in zip(r["op_E"], r["gt_E"])], np.float64)
        _REF[name] = r
    return _REF[name]


def _same(a, b):
    """== with nan matching nan."""
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


@pytest.mark.parametrize("name", list(CASES))
def test_stages_match_yardstick(cuda, name):
    import torch
    from pldepth_amd import kernels as K
    r = _reference(name)
    E = {}
    for k in ("op", "gt"):
        u8 = K.minmax_u8(torch.from_numpy(r[k]).cuda())
        assert np.array_equal(u8.cpu().numpy(), r[k + "_u8"]), (name, k, "u8")
        sweeps = torch.full((u8.shape[0],), -1, dtype=torch.int32, device="cuda")
        E[k], thr = K.auto_canny(u8, sweeps=sweeps)
        assert np.array_equal(thr.cpu().numpy(), r[k + "_thr"]), (name, k, "thresholds")
        assert np.array_equal(E[k].cpu().numpy(), r[k + "_E"]), (name, k, "edges")
        h, w = u8.shape[1:]
        assert all(1 <= s <= h * w for s in sweeps.tolist()), sweeps.tolist()
        dt = K.chamfer_dt3(E[k]).cpu().numpy()
        assert dt.dtype == np.float32 and np.array_equal(dt, r[k + "_dt"]), (name, k, "dt")
    m = K.depth_edge_metric(E["op"], E["gt"]).cpu().numpy()
    assert _same(m, r["metric"]), (name, m, r["metric"])
    if name == "batch3_const":  # the constant maps have no edges
        assert math.isnan(m[1, 0]) and m[1, 1] == 0.0 and m[2, 0] == 0.0 and math.isnan(m[2, 1])
    if name == "step12x16":
        assert m[0, 0] == 62587 / 65536 == m[0, 1]


def test_explicit_thresholds(cuda):
    """cv2.Canny(img, lo, hi) with given thresholds, in either order."""
    import torch
    from pldepth_amd import kernels as K
    u8 = _reference("33x47")["gt_u8"]
    want = R.canny(u8[0], 30, 90)
    assert want.any() and not np.array_equal(want, _reference("33x47")["gt_E"][0])
    for lo, hi in ((30, 90), (90, 30)):
        got = K.canny(torch.from_numpy(u8).cuda(), lo, hi).cpu().numpy()
        assert np.array_equal(got[0], want), (lo, hi)


def test_hysteresis_depth(cuda):
    """A vertical step whose height falls from 80 to 6 grey levels down 200 rows, thresholds
    (20, 255): only the top rows are strong (4 * height > 255), the rest of the edge is reached
    by propagation through about 150 rows of weak pixels."""
    import torch
    from pldepth_amd import kernels as K
    img = np.zeros((200, 16), np.uint8)
    img[:, 8:] = np.round(np.linspace(80, 6, 200)).astype(np.uint8)[:, None]
    lab = R.canny_labels(img, 20, 255)
    strong_rows = np.nonzero((lab == 2).any(axis=1))[0]
    assert 30 < strong_rows.size < 60 and strong_rows.max() < 60
    want = R.canny(img, 20, 255)
    assert (want != 0).any(axis=1).all()  # the edge runs through every row
    sweeps = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = K.canny(torch.from_numpy(img[None]).cuda(), 20, 255, sweeps=sweeps).cpu().numpy()[0]
    assert np.array_equal(got, want)
    assert 1 < int(sweeps[0]) <= 200 * 16


def test_chamfer_on_plain_masks(cuda):
    """Masks that are not Canny output: random 60 % fill, a solid 30 x 30 block (distances above
    10 are cut to 0), and a mask without any zero pixel (all 0)."""
    import torch
    from pldepth_amd import kernels as K
    rng = np.random.default_rng(11)
    block = np.zeros((40, 40), np.uint8)
    block[5:35, 5:35] = 1  # any non-zero value marks the mask
    masks = [(rng.random((20, 24)) < 0.6).astype(np.uint8) * 255, block,
             np.full((12, 12), 255, np.uint8)]
    for m in masks:
        got = K.chamfer_dt3(torch.from_numpy(m[None]).cuda()).cpu().numpy()[0]
        assert np.array_equal(got, R.chamfer_dt3(m)), m.shape
    got = K.chamfer_dt3(torch.from_numpy(block[None]).cuda()).cpu().numpy()[0]
    assert np.count_nonzero(got) == 30 * 30 - 100 and got.max() <= 10
    assert not K.chamfer_dt3(torch.from_numpy(masks[2][None]).cuda()).any()
    # a smaller cut
    got = K.chamfer_dt3(torch.from_numpy(block[None]).cuda(), 3.0).cpu().numpy()[0]
    assert np.array_equal(got, R.chamfer_dt3(block, 3.0))


def test_size_limit_is_an_error(cuda):
    """Maps above PLD_EDGE_MAX_DIM: PLD_ERR_UNSUPPORTED (3) and nothing is launched."""
    import torch
    from pldepth_amd import _lib
    from pldepth_amd import kernels as K
    assert K.EDGE_MAX_DIM == 512
    lib = _lib.lib()
    for h, w in ((513, 16), (16, 513)):
        img = torch.zeros((1, h, w), dtype=torch.uint8, device="cuda")
        out = torch.full((1, h, w), 7, dtype=torch.uint8, device="cuda")
        thr = torch.full((1, 2), -5, dtype=torch.int32, device="cuda")
        ws = K.workspace(lib.pld_canny_workspace_size(1, h, w), "canny")
        with pytest.raises(_lib.PLDError, match=r"\(3\).*512 x 512 limit"):
            lib.pld_canny_u8(K.ptr(img), 1, h, w, 0, 255, K.ptr(out), None, K.ptr(ws), K.stream())
        with pytest.raises(_lib.PLDError, match=r"\(3\).*512 x 512 limit"):
            lib.pld_auto_canny_u8(K.ptr(img), 1, h, w, -0.8, 2.8, K.ptr(thr), K.ptr(out), None,
                                  K.ptr(ws), K.stream())
        torch.cuda.synchronize()
        assert bool((out == 7).all()) and bool((thr == -5).all())
    mask = torch.ones((1, 8, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.PLDError, match=r"\(3\)"):
        K.chamfer_dt3(mask, 11.0)
    # the largest supported map runs
    img = torch.zeros((1, 512, 512), dtype=torch.uint8, device="cuda")
    img[:, :, 300:] = 90
    e, thr = K.auto_canny(img)
    assert thr.tolist() == [[0, 0]] and bool((e[0, :, 299] == 255).all())
    assert int((e != 0).sum()) == 512


def test_depth_edge_metric_api(cuda):
    """depth_edge_metric on (H, W, 1) inputs and auto_canny through the reference's import
    path."""
    from pldepth.active_learning.preprocess_utils import auto_canny
    from pldepth_amd.active_learning import metrics as AM
    r = _reference("224x224")
    got = AM.depth_edge_metric(r["op"][0][..., None], r["gt"][0][..., None])
    assert isinstance(got[0], float) and _same(got, r["metric"][0])
    assert got[0] > 0 and got[1] > 0
    got = AM.depth_edge_metric(r["op"][0], r["gt"][0], imsize=(7, 7))  # (H, W); imsize unused
    assert _same(got, r["metric"][0])
    r = _reference("step12x16")
    b, c = AM.depth_edge_metric(np.full((12, 16, 1), 3.0, np.float32), r["gt"][0][..., None])
    assert math.isnan(b) and c == 0.0
    e = auto_canny(r["gt_u8"][0])
    assert isinstance(e, np.ndarray) and e.dtype == np.uint8 and np.array_equal(e, r["gt_E"][0])
    with pytest.raises(ValueError):
        auto_canny(r["gt"][0])  # float image


def test_calc_depth_metrics_on_model(cuda):
    """calc_depth_metrics over a test set of 5 images (a padded tail batch) through the model's
    inference forward, against the yardstick applied to model.predict."""
    from pldepth_amd.active_learning import metrics as AM
    from pldepth_amd.losses.losses_meta import DepthLossType
    from pldepth_amd.models.models_meta import ModelParameters, get_model_type_by_name
    from pldepth_amd.models.PLDepthNet import get_pl_depth_net
    mp = ModelParameters()
    mp.set_parameter("model_type", get_model_type_by_name("ff_effnet"))
    mp.set_parameter("ranking_size", 5)
    mp.set_parameter("rankings_per_image", 10)
    mp.set_parameter("batch_size", 2)
    mp.set_parameter("loss_type", DepthLossType.NLL)
    mp.set_parameter("seed", 0)
    H = W = 224
    model, pre = get_pl_depth_net(mp, [H, W, 3])
    rng = np.random.default_rng(3)
    x = pre(rng.random((5, H, W, 3), dtype=np.float32))
    gt = np.stack([R.scene(H, W, 20 + k) for k in range(5)])
    pred = model.predict(x)
    want = np.array([R.exact(pred[k], gt[k]) for k in range(5)])
    got = AM.calc_depth_metrics(model, x, gt)
    assert isinstance(got[0], float) and isinstance(got[1], float)
    assert _same(got, (np.mean(want[:, 0]), np.mean(want[:, 1]))), (got, want)
