"""Input-pipeline measurement for the device-resident provider. Not a test.

    timeout -k 10 600 python tools/provider_bench.py [--part a|b|ab] [--json PATH]

(a) pld_batch_gather_flip alone at cfg2's batch (32 of 64 resident images, 448 x 448, half of
    them flipped), HIP events on one stream, against a plain device-to-device copy_ of the same
    three output tensors: the floor any gather pays. Alternating windows; also the call through
    kernels.batch_gather_flip (index upload and three fresh output tensors included).
(b) fit() steps per second at cfg2's shape (ff_effnet, batch 32, 448 x 448, ranking_size 5, 100
    rankings per image, Info sampler, flips on) with the provider's host path against
    device_resident=True, same seed, wall clock over the steps after the capture step (fit
    reads the loss back every step, so each step ends in a device synchronise). Alternating
    rounds on one model.
Prints one JSON line (and writes it to --json).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pldepth_amd import kernels as K  # noqa: E402
from pldepth_amd._lib import lib  # noqa: E402


def part_a(n=64, B=32, size=448, windows=5, reps=20):
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(0)
    imgs = torch.rand(n, size, size, 3, device=dev, generator=g)
    gts = torch.rand(n, size, size, device=dev, generator=g)
    masks = (torch.rand(n, size, size, device=dev, generator=g) < 0.9).float()
    rng = np.random.default_rng(0)
    idx = rng.permutation(n)[:B]
    flip = np.arange(B) % 2
    idx_d = torch.from_numpy(idx.astype(np.int32)).to(dev)
    flip_d = torch.from_numpy(flip.astype(np.int32)).to(dev)
    out = [torch.empty(B, size, size, 3, device=dev), torch.empty(B, size, size, device=dev),
           torch.empty(B, size, size, device=dev)]
    dst = [torch.empty_like(t) for t in out]
    st = K.stream()

    def gather():
        lib().pld_batch_gather_flip(K.ptr(imgs), K.ptr(gts), K.ptr(masks), n, size, size, 3,
                                    K.ptr(idx_d), K.ptr(flip_d), B, K.ptr(out[0]), K.ptr(out[1]),
                                    K.ptr(out[2]), st)

    def copy():
        for d, s in zip(dst, out):
            d.copy_(s)

    def wrapped():
        K.batch_gather_flip(imgs, gts, masks, idx, flip)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / reps  # us per call

    fns = {"gather_kernel": gather, "copy_3_tensors": copy, "gather_wrapper": wrapped}
    for fn in fns.values():  # warm up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            us[k].append(window(fn))
    # the gather is right before it is timed as a yardstick
    x, gt, mask = K.batch_gather_flip(imgs, gts, masks, idx, flip)
    ref = imgs[torch.from_numpy(idx).to(dev)]
    ref[1::2] = ref[1::2].flip(2)
    assert torch.equal(x, ref) and torch.equal(out[0], ref)
    moved = 2 * sum(t.numel() * 4 for t in out)  # read once, written once
    res = {"shape": f"{B} of {n} images, {size}x{size}x(3+1+1) fp32, {B // 2} flipped",
           "bytes_moved": moved, "windows": windows, "calls_per_window": reps}
    for k, v in us.items():
        med = statistics.median(v)
        res[k] = {"us_median": round(med, 1), "us_min": round(min(v), 1),
                  "us_max": round(max(v), 1), "tb_per_s": round(moved / med / 1e6, 3)}
    res["gather_over_copy"] = round(res["gather_kernel"]["us_median"] /
                                    res["copy_3_tensors"]["us_median"], 3)
    return res


class _Clock(object):
    def __init__(self):
        self.t = []

    def on_batch_end(self, batch, logs=None):
        self.t.append(time.perf_counter())


def part_b(n=128, B=32, size=448, L=5, R=100, steps=20, rounds=2, seed=0):
    from pldepth_amd.data.providers.hourglass_provider import HourglassLargeScaleDataProvider
    from pldepth_amd.data.sampling import InformationScoreBasedSampling
    from pldepth_amd.losses.losses_meta import DepthLossType
    from pldepth_amd.losses.nll_loss import HourglassNegativeLogLikelihood
    from pldepth_amd.models.models_meta import ModelParameters, get_model_type_by_name
    from pldepth_amd.models.PLDepthNet import get_pl_depth_net
    from pldepth_amd.optimizers import Adam
    from pldepth_amd.PLDepth import synthetic_hrwsi

    n_sched = 0
    if os.path.exists(K.DEFAULT_SCHEDULES):  # bench.py's conv schedules, no timing-based tuning
        n_sched, _ = K.use_schedule_table()
    mp = ModelParameters()
    mp.set_parameter("model_type", get_model_type_by_name("ff_effnet"))
    mp.set_parameter("ranking_size", L)
    mp.set_parameter("rankings_per_image", R)
    mp.set_parameter("val_rankings_per_img", R)
    mp.set_parameter("batch_size", B)
    mp.set_parameter("loss_type", DepthLossType.NLL)
    mp.set_parameter("seed", seed)
    mp.set_parameter("sampling_strategy", InformationScoreBasedSampling(mp))
    model, pre = get_pl_depth_net(mp, [size, size, 3])
    model.compile(loss=HourglassNegativeLogLikelihood(L, B), optimizer=Adam(1e-4, amsgrad=True))
    imgs, gts, masks = synthetic_hrwsi(n, size, size, seed)
    ms = {"host": [], "device_resident": []}
    upload_s = None
    for _ in range(rounds):
        for mode in ms:
            prov = HourglassLargeScaleDataProvider(mp, masks, None, augmentation=True, seed=seed,
                                                   device_resident=mode == "device_resident")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ds = prov.provide_train_dataset(pre(imgs), gts)
            torch.cuda.synchronize()
            if mode == "device_resident":
                upload_s = time.perf_counter() - t0
            clock = _Clock()
            # the first step of a fit is the eager + capture step (round 1) or a warm-up
            model.fit(x=ds, epochs=1, steps_per_epoch=steps + 1, callbacks=[clock], verbose=0)
            ms[mode].append(1e3 * (clock.t[-1] - clock.t[0]) / steps)
            del ds, prov
    res = {"shape": f"ff_effnet {size}x{size}, batch {B}, ranking_size {L}, rankings_per_image "
                    f"{R}, Info sampler, flips on, {n} images", "timed_steps": steps,
           "rounds": rounds, "schedule_table_entries": n_sched,
           "resident_upload_s": round(upload_s, 3)}
    for mode, v in ms.items():
        res[mode] = {"ms_per_step": [round(x, 3) for x in v],
                     "steps_per_s": round(1e3 / statistics.median(v), 2)}
    res["speedup"] = round(res["device_resident"]["steps_per_s"] / res["host"]["steps_per_s"], 2)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab", choices=["a", "b", "ab"])
    ap.add_argument("--steps", type=int, default=20, help="timed fit() steps per round (b)")
    ap.add_argument("--images", type=int, default=128, help="train-set size (b)")
    ap.add_argument("--json", default="")
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "provider_bench.py measures on the GPU"
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0)}
    if "a" in a.part:
        out["a_kernel"] = part_a()
        print("[provider_bench] (a)", json.dumps(out["a_kernel"]), file=sys.stderr, flush=True)
    if "b" in a.part:
        out["b_fit"] = part_b(n=a.images, steps=a.steps)
    line = json.dumps(out)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
