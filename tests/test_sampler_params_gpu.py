"""GPU tests of the samplers' run-time arguments (pld_sampler_rank_ex): tau, penalty, candidate
factor, masks on another grid than the image's and the unmasked RandomSamplingStrategy, bit for
bit against tests/sampler_params_ref.py (itself pinned to the reference's recorded outputs by
tests/test_sampler_params.py) through every layer: the kernels, the per-image API, the batched
Philox path and the provider."""
import os

import numpy as np
import pytest
import torch

import sampler_params_ref as P
from oracle import philox as PH
from pldepth_amd import kernels as K
from pldepth_amd.data import sampling as PS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STRATEGIES, N_CASES = P.GOLDEN_STRATEGIES, P.GOLDEN_CASES


@pytest.fixture(scope="module")
def pgolden():
    return np.load(os.path.join(HERE, "golden", "sampler_params_golden.npz"))


def _compact(gt, mask, cuda):
    """(gt, valid_idx, nvalid, gt_minmax) device tensors of gt [B,H,W], mask [B,mh,mw]."""
    B = gt.shape[0]
    ggt = torch.from_numpy(gt).to(cuda)
    gmask = torch.from_numpy(mask).to(cuda)
    vi = torch.empty(B, mask.shape[1] * mask.shape[2], dtype=torch.int32, device=cuda)
    nv = torch.empty(B, dtype=torch.int32, device=cuda)
    mm = torch.empty(B, 2, device=cuda)
    if mask.shape == gt.shape:
        K.sampler_compact(gmask, ggt, vi, nv, mm)
    else:
        K.sampler_compact(gmask, None, vi, nv, None)
        K.sampler_minmax(ggt, mm)
    return ggt, vi, nv, mm


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("ci", range(N_CASES))
def test_rank_ex_bit_exact_vs_restatement_and_golden(cuda, pgolden, ci, strategy):
    gt, mask, L, R, tau, pen, factor = P.load_case(pgolden, ci)
    draws = P.case_draws(pgolden, ci, strategy, gt.shape[1])
    ref = P.sample_point_batch(strategy, mask, gt, R, L, draws, tau, pen, factor)
    nc = int(R * factor)
    B = 2  # two copies of the image: per-image strides of both grids
    ggt, vi, nv, mm = _compact(np.stack([gt, gt]), np.stack([mask, mask]), cuda)
    gd = torch.from_numpy(np.stack([draws, draws]).astype(np.int32)).to(cuda).view(B, nc, L)
    out = torch.full((B,) + ref.shape, float("nan"), device=cuda)
    if strategy == "random":
        K.sampler_rank_ex(ggt, None, None, None, gd, R, L, strategy, out, nc)
    else:
        K.sampler_rank_ex(ggt, vi, nv, mm, gd, R, L, strategy, out, nc, tau, pen, mask.shape)
    # the whole-image bounds, from either kernel that gives them
    mm2 = torch.empty_like(mm)
    K.sampler_minmax(ggt, mm2)
    torch.cuda.synchronize()
    assert mm.cpu().tolist() == mm2.cpu().tolist() == [[float(gt.min()), float(gt.max())]] * 2
    o = out.cpu().numpy()
    for b in range(B):
        assert np.array_equal(o[b], ref), (b, np.argwhere(o[b] != ref)[:5])
    assert np.array_equal(P.canonical_lists(o[0]),
                          P.canonical_lists(pgolden[f"c{ci}_{strategy}_out"]))


@pytest.mark.parametrize("strategy", ["thresh", "info", "pure", "masked"])
@pytest.mark.parametrize("ci", range(4))
def test_rank_ex_at_defaults_equals_rank(cuda, golden, ci, strategy):
    h, w, L, R = [int(v) for v in golden[f"c{ci}_shape"]]
    mask = np.unpackbits(golden[f"c{ci}_mask"])[: h * w].reshape(h, w).astype(np.float32)
    gt = golden[f"c{ci}_codes"].astype(np.float32) / np.float32(255)
    ggt, vi, nv, mm = _compact(gt[None], mask[None], cuda)
    nc = K.sampler_candidates(R, strategy)
    gd = torch.from_numpy(golden[f"c{ci}_{strategy}_draws"].astype(np.int32)).to(cuda)
    gd = gd.view(1, nc, L)
    r_out = min(nc, R)
    old = torch.full((1, r_out, L, 2), float("nan"), device=cuda)
    new = torch.full((1, r_out, L, 2), float("nan"), device=cuda)
    K.sampler_rank(ggt, vi, nv, mm, gd, R, L, strategy, old)
    K.sampler_rank_ex(ggt, vi, nv, mm, gd, R, L, strategy, new, nc, 0.03, -1000, (h, w))
    torch.cuda.synchronize()
    assert np.array_equal(old.cpu().numpy(), new.cpu().numpy())
    assert not torch.isnan(new).any()


@pytest.mark.parametrize("ci,strategy", [(1, "thresh"), (2, "info"), (1, "pure"), (0, "random"),
                                         (2, "random")])
def test_per_image_api_reproduces_the_reference(cuda, pgolden, ci, strategy):
    """Seeded like the generator, the classes consume the global NumPy RNG as the reference does
    and return its rankings (ties aside): scaled masks (cases 1, 2) and the unmasked sampler."""
    gt, mask, L, R, tau, pen, factor = P.load_case(pgolden, ci)
    mp = P.Params(ranking_size=L, downscaling_factor=1)
    image = np.zeros(gt.shape + (3,), np.float32)
    np.random.seed(int(pgolden["seed"]) + 100 * ci + STRATEGIES.index(strategy))
    if strategy == "random":
        out = PS.RandomSamplingStrategy(mp).sample_points_batch(image, gt, R, factor)
    elif strategy == "pure":
        out = PS.PurelyMaskedRandomSamplingStrategy(mp).sample_masked_point_batch(
            image, mask, gt, R, factor)
    else:
        cls = {"thresh": PS.ThresholdedMaskedRandomSamplingStrategy,
               "info": PS.InformationScoreBasedSampling}[strategy]
        out = cls(mp, tau, pen).sample_masked_point_batch(image, mask, gt, R, factor)
    ref = pgolden[f"c{ci}_{strategy}_out"]
    assert out.shape == ref.shape and out.dtype == np.float32
    assert np.array_equal(P.canonical_lists(out), P.canonical_lists(ref))


def _batch(seed, B, H, W, mh, mw, empty=None):
    rng = np.random.default_rng(seed)
    gt = (rng.integers(0, 256, (B, H, W)).astype(np.float32) / np.float32(255))
    mask = (rng.random((B, mh, mw)) < 0.8).astype(np.float32)
    if empty is not None:
        mask[empty] = 0
    return gt, mask


def _philox_reference(strategy, gt, mask, R, L, tau, pen, factor, seed, step, image_offset=0):
    """The restatement fed the Philox draws of (seed, step): float32 [B, R', L, 2]."""
    B, H, W = gt.shape
    nc = int(R * factor)
    if strategy == "random":
        nvalid = [H * W] * B
    else:
        nvalid = [int((mask[b] > 0).sum()) for b in range(B)]
    draws = PH.sampler_draws(nvalid, nc, L, seed, step, image_offset)
    return np.stack([P.sample_point_batch(strategy, None if strategy == "random" else mask[b],
                                          gt[b], R, L, draws[b].reshape(-1), tau, pen, factor)
                     for b in range(B)])


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("strategy", ["thresh", "info", "pure", "random"])
def test_sample_batch_gpu_philox_equals_restatement(cuda, strategy, scaled):
    B, H, W, L, R = 3, 24, 32, 5, 10
    tau, pen, factor = 0.1, -5, 2.2
    mh, mw = (12, 16) if scaled else (H, W)
    gt, mask = _batch(5, B, H, W, mh, mw, empty=1)
    mp = P.Params(ranking_size=L)
    st = {"thresh": lambda: PS.ThresholdedMaskedRandomSamplingStrategy(mp, tau, pen),
          "info": lambda: PS.InformationScoreBasedSampling(mp, tau, pen),
          "pure": lambda: PS.PurelyMaskedRandomSamplingStrategy(mp),
          "random": lambda: PS.RandomSamplingStrategy(mp)}[strategy]()
    out = st.sample_batch_gpu(torch.from_numpy(gt).to(cuda), torch.from_numpy(mask).to(cuda), R,
                              seed=77, step=3, image_offset=4, batch_size_factor=factor)
    ref = _philox_reference(strategy, gt, mask, R, L, tau, pen, factor, 77, 3, 4)
    o = out.cpu().numpy()
    assert o.shape == ref.shape == (B, R, L, 2)
    assert np.array_equal(o, ref)
    if strategy != "random":  # the empty mask: the defined all-invalid lists
        assert (o[1, :, :, 0] == 0).all() and (o[1, :, :, 1] == -1).all()
        assert (o[0, :, :, 1] >= 0).all() and (o[2, :, :, 1] >= 0).all()


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("resident", [False, True])
def test_provider_threshold_reaches_the_training_sampler(cuda, resident, half):
    from pldepth_amd.data.providers.hourglass_provider import (HourglassLargeScaleDataProvider,
                                                               _epoch_batches)
    n, H, W, B, L, R, tau = 6, 16, 20, 2, 4, 6, 0.1
    mh, mw = (H // 2, W // 2) if half else (H, W)
    gts, masks = _batch(21, n, H, W, mh, mw)
    imgs = np.random.default_rng(2).random((n, H, W, 3)).astype(np.float32)
    mp = P.Params(ranking_size=L, rankings_per_image=R, batch_size=B)
    prov = HourglassLargeScaleDataProvider(mp, masks, None, augmentation=True,
                                           sampling_eq_threshold=tau, seed=3,
                                           device_resident=resident)
    assert prov.random_sampler.threshold == tau and prov.val_random_sampler.threshold == 0.03
    x, y = next(iter(prov.provide_train_dataset(imgs, gts)))
    idx, flip = next(_epoch_batches(np.random.default_rng(3), n, B, augment=True))
    fl = lambda a: np.ascontiguousarray(  # noqa: E731
        np.where(flip.reshape((B,) + (1,) * (a.ndim - 1)), a[:, :, ::-1], a))
    assert np.array_equal(x.cpu().numpy(), fl(imgs[idx]))
    ref = _philox_reference("thresh", fl(gts[idx]), fl(masks[idx]), R, L, tau, -1000, 1.5, 3, 0)
    assert np.array_equal(y.cpu().numpy(), ref)
    dflt = _philox_reference("thresh", fl(gts[idx]), fl(masks[idx]), R, L, 0.03, -1000, 1.5, 3, 0)
    assert not np.array_equal(ref, dflt)  # the threshold matters on this data
