"""Device-resident data provider: pld_batch_gather_flip against NumPy bit for
bit, the wrapper's host index check, 64-bit source offsets, and the provider's device-resident
mode against its host path (pldepth/data/providers/hourglass_provider.py:29-73): the same
batches for the same seed, from device memory alone, feeding fit()."""
import numpy as np
import pytest
import torch

from pldepth_amd import kernels as K
from pldepth_amd.data.providers.hourglass_provider import HourglassLargeScaleDataProvider
from pldepth_amd.data.sampling import InformationScoreBasedSampling
from pldepth_amd.losses.losses_meta import DepthLossType
from pldepth_amd.losses.nll_loss import HourglassNegativeLogLikelihood
from pldepth_amd.models.models_meta import ModelParameters, get_model_type_by_name
from pldepth_amd.models.PLDepthNet import get_pl_depth_net
from pldepth_amd.optimizers import Adam
from pldepth_amd.PLDepth import synthetic_hrwsi

pytestmark = pytest.mark.gpu

N, B, H = 5, 4, 3
IDX = [4, 0, 4, 2]
# -0.0, NaNs with payloads (quiet +, quiet -, signalling), inf, a denormal
SPECIALS = np.array([0x80000000, 0x7fc00123, 0xffc0beef, 0x7f800001, 0x7f800000, 0x00000001],
                    np.uint32).view(np.int32)


def _source(shape, seed):
    """Normal draws with every third element one of SPECIALS in turn (so each image holds all)."""
    a = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    bits = a.reshape(-1).view(np.int32)
    k = len(bits[::3])
    bits[::3] = SPECIALS[np.arange(k) % len(SPECIALS)]
    return a


def _expect(src, idx, flip):
    out = src[np.asarray(idx)].copy()
    for b, f in enumerate(flip if flip is not None else []):
        if f:
            out[b] = out[b][:, ::-1].copy()
    return out


def _same_bits(t, ref):
    got = t.cpu().numpy()
    assert got.shape == ref.shape
    np.testing.assert_array_equal(got.view(np.int32), ref.view(np.int32))


@pytest.mark.parametrize("flip", [[1, 0, 1, 0], [0, 0, 0, 0], [1, 1, 1, 1], None],
                         ids=["alternate", "none", "all", "null"])
@pytest.mark.parametrize("w", [1, 4, 5, 6, 8, 13])
def test_kernel_matches_numpy_bitwise(cuda, w, flip):
    imgs, gts, masks = _source((N, H, w, 3), 1), _source((N, H, w), 2), _source((N, H, w), 3)
    d = [torch.from_numpy(a).to(cuda) for a in (imgs, gts, masks)]
    keep = [t.clone() for t in d]
    x, gt, mask = K.batch_gather_flip(d[0], d[1], d[2], IDX, flip)
    _same_bits(x, _expect(imgs, IDX, flip))
    _same_bits(gt, _expect(gts, IDX, flip))
    _same_bits(mask, _expect(masks, IDX, flip))
    # images alone (gts / masks NULL), into given outputs
    out = (torch.full_like(x, 7.0), None, None)
    x2, gt2, mask2 = K.batch_gather_flip(d[0], None, None, np.array(IDX), flip, out=out)
    assert x2 is out[0] and gt2 is None and mask2 is None
    _same_bits(x2, _expect(imgs, IDX, flip))
    for t, k in zip(d, keep):  # sources untouched
        assert torch.equal(t.view(torch.int32), k.view(torch.int32))


@pytest.mark.parametrize("w", [8, 13])
def test_kernel_single_channel_images(cuda, w):
    """c = 1 takes the vector kernel's other instance (w = 8) / the scalar kernel (w = 13)."""
    imgs = _source((N, H, w, 1), 4)
    x, _, _ = K.batch_gather_flip(torch.from_numpy(imgs).to(cuda), None, None, IDX, [1, 0, 1, 0])
    _same_bits(x, _expect(imgs, IDX, [1, 0, 1, 0]))


@pytest.mark.parametrize("w", [1024, 1023])
def test_kernel_grid_stride(cuda, w):
    """2 x 1032 x 1024 pixels are 2064 blocks of 4-pixel units: more than the 2048-block grid, so
    some threads take a second unit (w = 1023: the scalar kernel, 4 units per thread)."""
    n, h = 2, 1032
    rng = np.random.default_rng(5)
    imgs = rng.random((n, h, w, 3), dtype=np.float32)
    gts = rng.random((n, h, w), dtype=np.float32)
    idx, flip = [1, 0], [1, 0]
    x, gt, mask = K.batch_gather_flip(torch.from_numpy(imgs).to(cuda),
                                      torch.from_numpy(gts).to(cuda), None, idx, flip)
    assert mask is None
    _same_bits(x, _expect(imgs, idx, flip))
    _same_bits(gt, _expect(gts, idx, flip))


def test_wrapper_checks_indices_on_the_host(cuda):
    imgs = torch.zeros(N, H, 4, 3, device=cuda)
    out = (torch.full((2, H, 4, 3), 7.0, device=cuda), None, None)
    with pytest.raises(ValueError, match="outside a dataset of 5"):
        K.batch_gather_flip(imgs, None, None, [0, N], None, out=out)
    with pytest.raises(ValueError, match="index -1"):
        K.batch_gather_flip(imgs, None, None, [-1], None,
                            out=(torch.empty(1, H, 4, 3, device=cuda), None, None))
    torch.cuda.synchronize()
    assert bool((out[0] == 7.0).all())


def test_source_offsets_are_64_bit(cuda):
    """Image 3599 of 3600 x 448 x 448 x 3 starts at element 2.17e9 > 2^31."""
    if torch.cuda.mem_get_info()[0] < 16 << 30:
        pytest.skip("needs 16 GiB of free device memory")
    n, s = 3600, 448
    imgs = torch.empty(n, s, s, 3, device=cuda)  # 8.7 GB, uninitialised but for two images
    assert imgs.numel() > 1 << 31
    ramp = torch.arange(s * s * 3, dtype=torch.float32, device=cuda).view(s, s, 3)  # < 2^24: exact
    imgs[0] = ramp
    imgs[n - 1] = -ramp - 0.5
    x, _, _ = K.batch_gather_flip(imgs, None, None, [n - 1, 0], [1, 0])
    assert torch.equal(x[0], (-ramp - 0.5).flip(1))
    assert torch.equal(x[1], ramp)


# ------------------------------------------------------------------------------- provider
def _params(batch, R, L, size=None):
    mp = ModelParameters()
    mp.set_parameter("model_type", get_model_type_by_name("ff_effnet"))
    mp.set_parameter("ranking_size", L)
    mp.set_parameter("rankings_per_image", R)
    mp.set_parameter("val_rankings_per_img", R)
    mp.set_parameter("batch_size", batch)
    mp.set_parameter("loss_type", DepthLossType.NLL)
    mp.set_parameter("seed", 0)
    mp.set_parameter("sampling_strategy", InformationScoreBasedSampling(mp))
    return mp


def _providers(augmentation, n=10, size=16, batch=4, seed=11):
    """(host, resident) providers over private copies of one synthetic dataset, with the arrays
    each was built from: [imgs, gts, train masks, val masks]."""
    mp = _params(batch, 8, 3)
    imgs, gts, masks = synthetic_hrwsi(n, size, size, seed=seed)  # masks ~90 % valid
    out = []
    for resident in (False, True):
        arrs = [imgs.copy(), gts.copy(), masks.copy(), masks.copy()]
        prov = HourglassLargeScaleDataProvider(mp, arrs[2], arrs[3], augmentation=augmentation,
                                               seed=3, device_resident=resident)
        out.append((prov, arrs))
    return out


def _take(ds, k):
    it = iter(ds)
    return [next(it) for _ in range(k)]


@pytest.mark.parametrize("augmentation", [True, False])
def test_resident_provider_yields_the_host_batches(cuda, augmentation):
    (host, ha), (res, ra) = _providers(augmentation)
    hb = _take(host.provide_train_dataset(ha[0], ha[1]), 7)  # 2 batches per epoch: 3 reshuffles
    rb = _take(res.provide_train_dataset(ra[0], ra[1]), 7)
    for (hx, hy), (rx, ry) in zip(hb, rb):
        assert hx.shape == (4, 16, 16, 3) and hy.shape == (4, 8, 3, 2)
        assert torch.equal(hx, rx) and torch.equal(hy, ry)
    assert len({t.data_ptr() for t, _ in rb}) == 7  # fresh tensors: a consumer may keep them
    assert not torch.equal(hb[0][0], hb[2][0])      # (and the epochs do differ)
    hv, rv = host.provide_val_dataset(ha[0], ha[1]), res.provide_val_dataset(ra[0], ra[1])
    assert len(hv) == len(rv) == 2
    for (hx, hy), (rx, ry) in zip(hv, rv):
        assert torch.equal(hx, rx) and torch.equal(hy, ry)


def test_resident_provider_reads_device_memory_only(cuda):
    (host, ha), (res, ra) = _providers(True)
    ds = res.provide_train_dataset(ra[0], ra[1])
    val = res.provide_val_dataset(ra[0], ra[1])
    for a in ra:
        a[...] = 0
    assert not res.train_consistency_masks.any()  # the provider's own host masks are zero too
    for (hx, hy), (rx, ry) in zip(_take(host.provide_train_dataset(ha[0], ha[1]), 3),
                                  _take(ds, 3)):
        assert torch.equal(hx, rx) and torch.equal(hy, ry)
    for (hx, hy), (rx, ry) in zip(host.provide_val_dataset(ha[0], ha[1]), val):
        assert torch.equal(hx, rx) and torch.equal(hy, ry)


def test_upload_out_of_memory_is_a_memory_error(cuda, monkeypatch):
    """The device refuses the second of the three arrays: the first is freed again and the
    error names the bytes needed (10 x 16 x 16 x (3 + 1 + 1) floats) and the way out."""
    (_, _), (res, ra) = _providers(False)
    real, calls = torch.empty, []

    def empty(*args, **kwargs):
        calls.append(1)
        if len(calls) == 2:
            raise torch.cuda.OutOfMemoryError("HIP out of memory (injected)")
        return real(*args, **kwargs)

    before = torch.cuda.memory_allocated()
    monkeypatch.setattr(torch, "empty", empty)
    with pytest.raises(MemoryError, match=r"needs 51200 bytes.*device_resident=False"):
        res.provide_train_dataset(ra[0], ra[1])
    monkeypatch.undo()
    assert len(calls) == 2 and torch.cuda.memory_allocated() == before


def test_fit_from_resident_dataset(cuda, fixed_schedules):
    batch, size, L, R = 2, 64, 5, 8
    mp = _params(batch, R, L)
    model, pre = get_pl_depth_net(mp, [size, size, 3])
    model.compile(loss=HourglassNegativeLogLikelihood(L, batch), optimizer=Adam(1e-4, amsgrad=True))
    imgs, gts, masks = synthetic_hrwsi(6, size, size, seed=2)
    prov = HourglassLargeScaleDataProvider(mp, masks, None, augmentation=True, seed=0,
                                           device_resident=True)
    ds = prov.provide_train_dataset(pre(imgs), gts)
    losses, replays = [], []

    class Log(object):
        def on_batch_end(self, batch, logs=None):
            losses.append(logs["loss"])

    replay = model.trainer.step
    model.trainer.step = lambda *a, **k: (replays.append(1), replay(*a, **k))[1]
    model.fit(x=ds, epochs=1, steps_per_epoch=3, callbacks=[Log()], verbose=0)
    assert len(losses) == 3 and np.isfinite(losses).all(), losses
    assert len(replays) == 2  # step 1 runs eagerly and captures; steps 2 and 3 replay the graph
