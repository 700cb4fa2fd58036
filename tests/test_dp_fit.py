"""Data-parallel fit(), the parts that need no GPU: the provider's per-rank index work
(_epoch_batches), the launcher (dp.spawn_ranks, the CLI's --gpus), the steps-per-epoch arithmetic
and the mean-all-reduce helper over gloo on CPU tensors."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from pldepth_amd import dp
from pldepth_amd.data.providers.hourglass_provider import (HourglassLargeScaleDataProvider,
                                                           _epoch_batches)

B = 2


def _epochs(seed, n, batch, world, rank, augment, epochs=2):
    rng = np.random.default_rng(seed)
    out = [list(_epoch_batches(rng, n, batch, world, rank, augment)) for _ in range(epochs)]
    return out, rng.bit_generator.state


@pytest.mark.parametrize("augment", [True, False])
@pytest.mark.parametrize("n", [10, 11, 13])  # G = 4: remainders 2, 3, 1
def test_epoch_batches_ranks_tile_the_global_batch(n, augment):
    whole, state = _epochs(5, n, 2 * B, 1, 0, augment)
    r0, s0 = _epochs(5, n, B, 2, 0, augment)
    r1, s1 = _epochs(5, n, B, 2, 1, augment)
    assert s0 == s1 == state  # the ranks consume the host RNG exactly as one process does
    for ew, e0, e1 in zip(whole, r0, r1):
        assert len(ew) == len(e0) == len(e1) == n // (2 * B)
        for (iw, fw), (i0, f0), (i1, f1) in zip(ew, e0, e1):
            assert len(i0) == len(i1) == B
            np.testing.assert_array_equal(np.concatenate([i0, i1]), iw)
            if augment:
                assert f0.dtype == f1.dtype == np.bool_
                np.testing.assert_array_equal(np.concatenate([f0, f1]), fw)
            else:
                assert fw is None and f0 is None and f1 is None
    assert not np.array_equal(whole[0][0][0], whole[1][0][0])  # a new permutation per epoch


@pytest.mark.parametrize("augment", [True, False])
def test_epoch_batches_world1_is_the_single_replica_loop(augment):
    """The loop the provider's iterables ran before they could shard, restated literally."""
    n, batch = 11, 4
    rng = np.random.default_rng(3)
    want = []
    for _ in range(2):
        order = rng.permutation(n)
        for i in range(0, n - batch + 1, batch):
            idx = order[i:i + batch]
            flip = rng.random(batch) > 0.5 if augment else None
            want.append((idx, flip))
    got, state = _epochs(3, n, batch, 1, 0, augment)
    got = [b for e in got for b in e]
    assert len(got) == len(want) == 4
    for (gi, gf), (wi, wf) in zip(got, want):
        np.testing.assert_array_equal(gi, wi)
        if augment:
            np.testing.assert_array_equal(gf, wf)
        else:
            assert gf is None
    assert state == rng.bit_generator.state


def test_provider_rank_world_keywords():
    p = HourglassLargeScaleDataProvider(_Params(), np.zeros((1, 2, 2)), None, rank=1, world=2)
    assert (p.rank, p.world) == (1, 2)
    p = HourglassLargeScaleDataProvider(_Params(), np.zeros((1, 2, 2)), None)
    assert (p.rank, p.world) == (0, 1)
    with pytest.raises(ValueError, match="rank 2"):
        HourglassLargeScaleDataProvider(_Params(), np.zeros((1, 2, 2)), None, rank=2, world=2)


class _Params(object):
    def get_parameter(self, name):
        return {"ranking_size": 3, "equality_threshold": 0.03}.get(name)


# ------------------------------------------------------------------------------- launcher
def test_spawn_ranks_command_and_environment(monkeypatch):
    import subprocess
    seen = {}

    def call(cmd, env=None, **kw):
        seen.update(cmd=cmd, env=env)
        return 7

    monkeypatch.setattr(subprocess, "call", call)
    monkeypatch.delenv("OMP_NUM_THREADS", raising=False)
    monkeypatch.setenv("PLD_SOME_SETTING", "x")
    assert dp.spawn_ranks(3, ["--epochs", "2"], module="pldepth_amd.PLDepth") == 7
    cmd, env = seen["cmd"], seen["env"]
    port = cmd[cmd.index("--master-port") + 1]
    assert 1024 <= int(port) < 65536
    assert cmd == [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                   "--nproc-per-node", "3", "--master-addr", "127.0.0.1", "--master-port", port,
                   "-m", "pldepth_amd.PLDepth", "--epochs", "2"]
    assert env["OMP_NUM_THREADS"] == "4" and env["PLD_SOME_SETTING"] == "x"
    assert "WORLD_SIZE" not in env and "RANK" not in env  # the launcher sets them per rank
    monkeypatch.setenv("OMP_NUM_THREADS", "9")
    dp.spawn_ranks(2, [], module="m")
    assert seen["env"]["OMP_NUM_THREADS"] == "9"
    assert not torch.cuda.is_initialized()


def test_cli_gpus_only_launches(monkeypatch):
    """--gpus 2 without a launcher: the command hands its own arguments to spawn_ranks and exits
    with the child's status; nothing else of the run happens in this process."""
    from click.testing import CliRunner
    from pldepth_amd import PLDepth
    calls = []
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(PLDepth.dp, "spawn_ranks",
                        lambda n, argv, module: (calls.append((n, list(argv), module)), 5)[1])
    monkeypatch.setattr(PLDepth, "run_experiment",
                        lambda **kw: pytest.fail("the parent must not run the experiment"))
    res = CliRunner().invoke(PLDepth.perform_pldepth_experiment,
                             ["--gpus", "2", "--dist_backend", "gloo", "--batch_size", "2",
                              "--input_size", "64", "--augmentation", "false", "--save_path", "w.h5"])
    assert res.exit_code == 5
    assert not torch.cuda.is_initialized()
    (n, argv, module), = calls
    assert n == 2 and module == "pldepth_amd.PLDepth"
    # the child command line parses back to the same run, --gpus and the backend included
    ctx = PLDepth.perform_pldepth_experiment.make_context("PLDepth", list(argv))
    assert ctx.params["gpus"] == 2 and ctx.params["dist_backend"] == "gloo"
    assert ctx.params["batch_size"] == 2 and ctx.params["input_size"] == 64
    assert ctx.params["augmentation"] is False and ctx.params["save_path"] == "w.h5"
    assert ctx.params["ds_size"] is None and ctx.params["epochs"] == 50


def test_cli_rejects_gpus_that_disagree_with_the_launcher(monkeypatch):
    from click.testing import CliRunner
    from pldepth_amd import PLDepth
    monkeypatch.setenv("WORLD_SIZE", "4")
    monkeypatch.setattr(PLDepth, "run_experiment", lambda **kw: pytest.fail("must not run"))
    res = CliRunner().invoke(PLDepth.perform_pldepth_experiment, ["--gpus", "2"])
    assert res.exit_code == 2 and "WORLD_SIZE=4" in res.output


def test_cli_gpus_defaults_to_the_launchers_world(monkeypatch):
    """Under torch.distributed.run (WORLD_SIZE set) no --gpus is needed; without one it is 1."""
    from click.testing import CliRunner
    from pldepth_amd import PLDepth
    seen = []
    monkeypatch.setattr(PLDepth.dp, "exit_on_failure", lambda fn, world: seen.append(world) or 0)
    monkeypatch.setattr(PLDepth, "run_experiment", lambda **kw: seen.append(kw) or 0)
    monkeypatch.setenv("WORLD_SIZE", "8")
    assert CliRunner().invoke(PLDepth.perform_pldepth_experiment, []).exit_code == 0
    assert seen == [8]  # the rank body, not a second launch and not the single-replica run
    monkeypatch.delenv("WORLD_SIZE")
    assert CliRunner().invoke(PLDepth.perform_pldepth_experiment, ["--epochs", "1"]).exit_code == 0
    assert len(seen) == 2 and seen[1]["epochs"] == 1 and "rank" not in seen[1]


def test_cli_options():
    from pldepth_amd.PLDepth import perform_pldepth_experiment
    opts = {p.name: p for p in perform_pldepth_experiment.params}
    assert opts["gpus"].opts == ["--gpus"] and opts["gpus"].default is None
    assert opts["dist_backend"].opts == ["--dist_backend"]
    assert list(opts["dist_backend"].type.choices) == ["nccl", "gloo"]


def test_steps_per_epoch_counts_global_batches():
    from pldepth_amd.PLDepth import steps_per_epoch_for
    assert steps_per_epoch_for(32, 2) == 14           # int(29.87 / 2): the reference's line
    assert steps_per_epoch_for(32, 2, 2) == 7         # int(29.87 / 4)
    assert steps_per_epoch_for(20000, 32, 8) == 72    # int(18666.67 / 256)
    assert steps_per_epoch_for(20000, 32, 1) == 583
    assert steps_per_epoch_for(8, 4, 8) == 1          # never zero steps


# ------------------------------------------------------------------------------- collectives
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _mean_rank(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dp.init_group("gloo", rank, world, timeout_s=60)
    try:
        stats = torch.full((37,), float(rank + 1))
        out = dp.allreduce_mean(stats, world)
        loss = dp.allreduce_mean(torch.tensor([2.5 + rank]), world)
        bad = dp.allreduce_mean(torch.tensor([float("nan") if rank == 1 else 1.0]), world)
        inf = dp.allreduce_mean(torch.tensor([float("inf") if rank == 0 else 1.0]), world)
        q.put((rank, out is stats, stats.numpy(), float(loss), float(bad), float(inf)))
    finally:
        dist.destroy_process_group()


def test_allreduce_mean_gloo_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_mean_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    out = [q.get(timeout=240) for _ in ps]
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(o[0] for o in out) == [0, 1]
    for _, in_place, stats, loss, bad, inf in out:
        assert in_place
        np.testing.assert_array_equal(stats, np.full(37, 1.5, np.float32))
        assert loss == 3.0
        assert np.isnan(bad) and np.isinf(inf)  # non-finite on one rank: non-finite on both


def test_fit_refuses_unsharded_arrays_on_a_replica():
    import types
    from pldepth_amd.models.pl_hourglass import FullyFledgedModel
    model = FullyFledgedModel(types.SimpleNamespace(B=2))
    model.world = 2
    with pytest.raises(ValueError, match="every rank would train on the same batches"):
        model.fit(x=np.zeros((4, 8, 8, 3), np.float32), y=np.zeros((4, 1, 3, 2), np.float32))
