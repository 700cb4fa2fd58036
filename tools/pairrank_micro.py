"""Times of the pairwise ranking loss beside ListMLE.

    python tools/pairrank_micro.py [--launches 40] [--no-step]

1. pld_pairrank_fwd_bwd ("all", "adjacent") and pld_listmle_fwd_bwd on the same inputs at the
   loss shapes of the bench's cfg2 (B 32, HW 448^2, R 100, L 5) and cfg5 (R 1000, L 64): HIP
   events around each launch, warm-up first, the three calls alternating, median and min / max
   over the launches.
2. The captured training step (sampler -> forward -> loss -> backward -> Adam-AMSGrad, one graph
   replay) at cfg2 with the ranking loss and with ListMLE: two trainers on the same batch and
   the bench's schedule table, timed in alternating blocks of replays between HIP events.
Prints one line per figure; needs the MI355X (no fallback).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pldepth_amd import kernels as K  # noqa: E402


def lists(rng, B, HW, R, L):
    """Sampler-shaped rankings: random pixels, 8-bit depths (ties and equal pairs as in the
    synthetic set), sorted by depth within a list as the masked samplers emit them."""
    idx = rng.integers(0, HW, (B, R, L))
    lab = np.sort(rng.integers(1, 256, (B, R, L)) / 255.0, axis=-1)[..., ::-1]
    return np.ascontiguousarray(np.stack([idx, lab], -1).astype(np.float32))


def time_calls(calls, launches, warmup=5):
    """{name: sorted ms per launch}; the calls alternate launch by launch."""
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in calls}
    for _ in range(launches):
        for name, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b))
    return {k: sorted(v) for k, v in out.items()}


def kernel_times(launches):
    rng = np.random.default_rng(0)
    B, H = 32, 448
    HW = H * H
    pred = torch.from_numpy(rng.standard_normal((B, HW)).astype(np.float32)).cuda()
    for name, R, L in (("cfg2", 100, 5), ("cfg5", 1000, 64)):
        y = torch.from_numpy(lists(rng, B, HW, R, L)).cuda()
        dpred = torch.empty_like(pred)
        per_list = torch.empty(B * R, device="cuda")
        loss = torch.empty(1, device="cuda")
        buf = dict(dpred=dpred, loss=loss)
        calls = {
            "listmle": lambda: K.listmle_fwd_bwd(pred, y, B, R, L, nll=per_list, **buf),
            "pairrank all": lambda: K.pairrank_fwd_bwd(pred, y, B, R, L, pair_mode="all",
                                                       per_list=per_list, **buf),
            "pairrank adjacent": lambda: K.pairrank_fwd_bwd(pred, y, B, R, L,
                                                            pair_mode="adjacent",
                                                            per_list=per_list, **buf),
        }
        for k, ms in time_calls(calls, launches).items():
            print("loss call %s B=%d HW=%d R=%d L=%d %-18s median %.1f us (min %.1f, max %.1f, "
                  "%d launches; zero + loss + reduce kernels)" % (
                      name, B, HW, R, L, k, 1e3 * ms[len(ms) // 2], 1e3 * ms[0], 1e3 * ms[-1],
                      len(ms)), flush=True)


def step_times(blocks=4, per_block=10):
    from bench import synthetic_batch
    from pldepth_amd.trainer import ReplicaTrainer
    n, sha = K.use_schedule_table()
    print("schedule table: %d entries, sha1 %s" % (n, sha), flush=True)
    B, H, L, R = 32, 448, 5, 100
    x, gt, mask = synthetic_batch(B, H, H, seed=1000)
    kinds = {"listmle": {}, "pairrank all": dict(loss_kind="pairrank", pair_args=dict(
        pair_mode="all", tau=0.03, invert=False, equal_weight=1.0))}
    trainers = {}
    for name, kw in kinds.items():
        tr = ReplicaTrainer((H, H, 3), B, L, R, 1, seed=0, **kw)
        tr.set_batch(torch.from_numpy(x).cuda(), torch.from_numpy(gt).cuda(),
                     torch.from_numpy(mask).cuda())
        tr.step_eager(0.01)
        tr.capture()
        for _ in range(5):
            tr.step(0.01)
        tr.synchronize()
        print("step %s: captured, loss %.4f" % (name, tr.loss_value()), flush=True)
        trainers[name] = tr
    ms = {k: [] for k in trainers}
    for _ in range(blocks):
        for name, tr in trainers.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(tr.stream):
                a.record()
            for _ in range(per_block):
                tr.step(0.01)
            with torch.cuda.stream(tr.stream):
                b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / per_block)
    for name, v in ms.items():
        v = sorted(v)
        print("training step cfg2 (ff_effnet B=32 448x448 L=5 R=100, graph replay) %-13s median "
              "%.2f ms (min %.2f, max %.2f; %d blocks of %d steps), loss %.4f" % (
                  name, v[len(v) // 2], v[0], v[-1], len(v), per_block,
                  trainers[name].loss_value()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.cuda.set_device(0)
    print("device: %s" % torch.cuda.get_device_name(0), flush=True)
    kernel_times(a.launches)
    if not a.no_step:
        step_times()


if __name__ == "__main__":
    main()
