"""Fully fledged depth models with the reference's API (mirrors pldepth/models/pl_hourglass.py).

``FullyFledgedModel`` keeps the surface the reference's drivers use on its keras.Model
(pldepth/PLDepth.py:115-181, run_scripts/*, hyperopt/*): ``compile(loss, optimizer)``,
``fit(x, epochs, steps_per_epoch, callbacks, validation_data, verbose)``, ``train_on_batch``,
``evaluate``, ``predict``, ``__call__``, ``get_weights``/``set_weights``,
``save_weights``/``load_weights`` and the ``asc_depth_order`` property. Underneath, every step is
the HIP engine (EffNetFF) driven by a graph-captured ReplicaTrainer; inputs are NHWC float32
arrays (numpy or device tensors), outputs device tensors [B,H,W,1].

``EffNetFullyFledged.get_model_and_normalization(input_shape, ranking_size, loss_type)`` returns
``(model, preprocess_fn)`` like pl_hourglass.py:45-100; EfficientNet's preprocess_input is the
identity (its Rescaling/Normalization live inside the model).
"""
import abc
import logging
import math
import os

import numpy as np
import torch

from ..losses.losses_meta import DepthLossType

log = logging.getLogger(__name__)


def preprocess_input_effnet(x, data_format=None):
    """keras.applications.efficientnet.preprocess_input: a pass-through."""
    return x


class FullyFledgedModel(object):
    def __init__(self, engine, asc_depth_order=False, batch_size=None):
        self.engine = engine
        self.asc_depth_order = asc_depth_order
        self.batch_size = batch_size or engine.B
        self.loss = None
        self.optimizer = None
        self.trainer = None
        self.stop_training = False
        self.history = {}
        self.rank, self.world, self.distributed = 0, 1, False  # compile(distribute=...)

    # ------------------------------------------------------------------ properties
    @property
    def asc_depth_order(self):
        """True when closer points have LOWER depth values (NYUDv2, Ibims, ...); HR-WSI is
        descending (pl_hourglass.py:22-35)."""
        return self._asc_depth_order

    @asc_depth_order.setter
    def asc_depth_order(self, value):
        self._asc_depth_order = value

    @staticmethod
    @abc.abstractmethod
    def get_model_and_normalization(input_shape, ranking_size, loss_type=DepthLossType.NLL):
        pass

    # ------------------------------------------------------------------ compile / train
    def compile(self, loss=None, optimizer=None, distribute=None, **kwargs):
        """``distribute``: None takes (rank, world) from the launcher's environment
        (dp.env_rank_world: RANK / WORLD_SIZE), or an explicit ``(rank, world, process_group)``.
        With world > 1, or a group given, this model is one data-parallel replica: the trainer
        exchanges the gradient over the group (the initialised default group, else one created
        here: backend PLD_DP_BACKEND, default nccl = RCCL), and every rank must hold the same
        parameters and frozen weights (same seed or same weights file; checked, not broadcast).
        A group given at world 1 keeps the trainer's single-graph step (it has nothing to
        exchange); the loss and statistics collectives then run over that one rank.
        The training step takes the loss's lambda weights (``loss.rank_weights``) and reduction:
        ``"none"`` is refused (a step needs a scalar), and so is ``"sum"`` at world > 1, where
        the 1/world gradient scale would turn it into a mean over ranks. A loss without those
        attributes, or with both at their defaults, trains through the unweighted call.
        A loss whose ``kind`` attribute is ``"pairrank"`` (losses/ranking_loss.py) makes the step
        call the pairwise ranking loss with the loss object's ``pair_args``; without the
        attribute the step is ListMLE's."""
        from .. import dp
        from ..optimizers import Adam
        from ..trainer import ReplicaTrainer
        loss_kw = {}
        reduction = getattr(loss, "reduction", "mean")
        if reduction == "none":
            raise ValueError("compile(): a loss with reduction 'none' cannot drive training")
        if reduction != "mean":
            loss_kw["reduction"] = reduction
        if getattr(loss, "rank_weights", None) is not None:
            loss_kw["rank_weights"] = loss.rank_weights
        kind = getattr(loss, "kind", "nll")
        if kind != "nll":
            loss_kw["loss_kind"] = kind
            loss_kw["pair_args"] = loss.pair_args
        self.loss = loss
        self.optimizer = optimizer if optimizer is not None else Adam(amsgrad=True)
        eng = self.engine
        if distribute is None:
            distribute = dp.env_rank_world()[:2] + (None,)
        rank, world, pg = distribute
        if not 0 <= rank < world:
            raise ValueError(f"rank {rank} outside a world of {world}")
        if reduction == "sum" and world > 1:
            raise ValueError("compile(): reduction 'sum' on a data-parallel replica: the 1/world "
                             "gradient scale would turn it into a mean over ranks")
        self.rank, self.world = rank, world
        self.distributed = world > 1 or pg is not None
        dist_kw = {}
        if self.distributed:
            import torch.distributed as dist
            if pg is None:
                if not dist.is_initialized():
                    # bounded: a rank that dies or never arrives ends the job, not a hang
                    dp.init_group(os.environ.get("PLD_DP_BACKEND", "nccl"), rank, world,
                                  device=torch.device("cuda", torch.cuda.current_device()),
                                  timeout_s=float(os.environ.get("PLD_DP_TIMEOUT", "600")))
                pg = dist.group.WORLD
            if dist.get_world_size(pg) != world:
                raise ValueError(f"world {world} but the process group has "
                                 f"{dist.get_world_size(pg)} ranks")
            dist_kw = dict(rank=rank, world_size=world, process_group=pg)
            # the mean-loss scalar all-reduced after each step (outside the captured graphs)
            self._loss_mean = torch.zeros(1, device=eng.device)
        self.trainer = ReplicaTrainer((eng.H, eng.W, 3), eng.B, loss.ranking_size, 1,
                                      engine=eng, gpu_sampler=False,
                                      beta_1=self.optimizer.beta_1, beta_2=self.optimizer.beta_2,
                                      epsilon=self.optimizer.epsilon, **dist_kw, **loss_kw)
        if self.distributed:
            self._check_replicas()
        self._captured = False
        pending = getattr(self, "_pending_optimizer_state", None)
        if pending:  # a load_model()ed file: restore its Adam slots now that they exist
            from ..util import keras_h5
            keras_h5.load_optimizer_state(self, pending)
            self._pending_optimizer_state = None

    def train_on_batch(self, x, y, sample_weight=None, return_loss=True):
        """One optimizer step on (x [B,H,W,3], y [B,R,L,2]); returns the batch loss (float).
        ``sample_weight``: a scalar, one weight per list ([B*R] or [B*R,1]) or one per image
        ([B] or [B,1]), as the loss's own ``sample_weight``. The first step that gives weights
        after a capture made without them captures the step again, once; later steps without
        weights run the same captured step on weights of one."""
        if self.trainer is None:
            raise RuntimeError("compile() the model first")
        tr = self.trainer
        if self._captured and (torch.as_tensor(y).numel() != tr.y_true.numel()
                               or (sample_weight is not None and tr.list_w is None)):
            # another ranking count than the captured step's (the active-learning round's
            # second fit, run_scripts/active_PLDepth.py:182), or the first sample weights: one
            # eager step, then capture again
            tr.drop_graphs()
            self._captured = False
        tr.set_batch(x, None, None)
        tr.set_rankings(y)
        tr.set_sample_weight(sample_weight)
        if not self._captured:
            tr.step_eager(self.optimizer.lr)
            tr.capture()
            self._captured = True
        else:
            tr.step(self.optimizer.lr)
        self.optimizer.iterations += 1
        if not return_loss:
            return None
        return self._mean_loss() if self.distributed else tr.loss_value()

    def _mean_loss(self):
        """The global batch's loss: the mean over ranks of the replicas' losses, one 1-element
        all-reduce issued behind the step's exchange (between graph launches, like the bucket
        all-reduces), then the readback. Non-finite on one rank is non-finite on all, so
        TerminateOnNaN / stop_training agree everywhere."""
        from .. import dp
        tr = self.trainer
        with torch.cuda.stream(tr.stream):
            self._loss_mean.copy_(tr.loss)
            dp.allreduce_mean(self._loss_mean, self.world, tr.pg)
        torch.cuda.current_stream().wait_stream(tr.stream)
        return float(self._loss_mean.item())

    def sync_moving_stats(self):
        """Data parallel: replace every replica's BN moving statistics by their mean over the
        ranks (sum-all-reduce of the engine's flat statistics buffer, x 1/world, in place), so
        the inference-mode forward (evaluate, predict) and saved weights are the same on every
        rank. Per-epoch work (fit calls it at each epoch's end); nothing of it is in the step. A
        single replica: nothing to do."""
        if not self.distributed:
            return
        from .. import dp
        tr = self.trainer
        tr._order_after_caller()  # e.g. a set_weights on the caller's stream
        with torch.cuda.stream(tr.stream):
            dp.allreduce_mean(self.engine.stats.buf, self.world, tr.pg)
        torch.cuda.current_stream().wait_stream(tr.stream)

    def _check_replicas(self):
        """Every rank holds the same parameters and frozen weights, bit for bit, or raise."""
        from .. import dp
        torch.cuda.synchronize()
        for what in ("params", "frozen"):
            same, sums = dp.replicas_identical(getattr(self.engine, what).buf, self.trainer.pg)
            if not same:
                raise RuntimeError(
                    f"data-parallel replicas differ in their {what} (checksums {sums}): build "
                    "every rank's model from the same seed or load the same weights file")

    def fit(self, x=None, y=None, epochs=1, steps_per_epoch=None, callbacks=None,
            validation_data=None, verbose=1, initial_epoch=0, **kwargs):
        """Keras-style loop. ``x``: an iterable of (x_batch, y_batch) pairs (a provider dataset,
        repeated as needed), or an array with ``y`` given. Data parallel: the iterable yields
        this rank's shard of each global batch (the provider's ``rank=`` / ``world=``); arrays
        are refused at world > 1, since nothing would shard them."""
        callbacks = list(callbacks or [])
        for cb in callbacks:
            if hasattr(cb, "set_model"):
                cb.set_model(self)
            else:
                cb.model = self
        if x is not None and y is not None:
            if self.world > 1:
                raise ValueError("fit(x=array, y=array) on a data-parallel replica: every rank "
                                 "would train on the same batches; pass this rank's shard as an "
                                 "iterable of (x, y) batches")
            xs, ys = np.asarray(x), np.asarray(y)
            B = self.batch_size
            n = len(xs) // B
            data = [(xs[i * B:(i + 1) * B], ys[i * B:(i + 1) * B]) for i in range(n)]
            steps_per_epoch = steps_per_epoch or n
        else:
            data = x
        it = iter(data)

        def next_batch():
            nonlocal it
            try:
                return next(it)
            except StopIteration:
                it = iter(data)
                return next(it)

        self._cb("on_train_begin", callbacks)
        for epoch in range(initial_epoch, epochs):
            self._cb("on_epoch_begin", callbacks, epoch)
            losses = []
            for step in range(steps_per_epoch):
                self._cb("on_batch_begin", callbacks, step)
                xb, yb = next_batch()
                loss = self.train_on_batch(xb, yb)
                losses.append(loss)
                logs = {"loss": loss}
                self._cb("on_batch_end", callbacks, step, logs)
                if not math.isfinite(loss):
                    log.warning("Batch %d: invalid loss, terminating training", step)
                    self.stop_training = True
                if self.stop_training:
                    break
            logs = {"loss": float(np.mean(losses)) if losses else float("nan")}
            # before evaluate and on_epoch_end: validation and a checkpoint callback see the
            # reconciled BN moving statistics
            self.sync_moving_stats()
            if validation_data is not None:
                logs["val_loss"] = self.evaluate(validation_data, verbose=0)
            for k, v in logs.items():
                self.history.setdefault(k, []).append(v)
            if verbose and self.rank == 0:
                print(f"Epoch {epoch + 1}/{epochs} - " +
                      " - ".join(f"{k}: {v:.4f}" for k, v in logs.items()), flush=True)
            self._cb("on_epoch_end", callbacks, epoch, logs)
            if self.stop_training:
                break
        self.sync_moving_stats()
        self._cb("on_train_end", callbacks)
        return self

    @staticmethod
    def _cb(name, callbacks, *args):
        for cb in callbacks:
            fn = getattr(cb, name, None)
            if fn is not None:
                fn(*args)

    # ------------------------------------------------------------------ inference
    def __call__(self, x, training=False):
        eng = self.engine
        xb = torch.as_tensor(x, dtype=torch.float32)
        if xb.shape[0] != eng.B:
            raise ValueError(f"batch {xb.shape[0]} != compiled batch {eng.B}; use predict()")
        stream = self.trainer.stream if self.trainer is not None else torch.cuda.current_stream()
        with torch.cuda.stream(stream):
            eng.act["input"].copy_(xb.reshape(eng.act["input"].shape))
            out = eng.forward(training=training)
            res = out.clone()
        torch.cuda.current_stream().wait_stream(stream)
        return res

    def predict(self, x, batch_size=None, verbose=0):
        """Inference-mode forward (BN moving statistics) over any number of images."""
        x = np.asarray(x, np.float32) if not isinstance(x, torch.Tensor) else x
        n = x.shape[0]
        B = self.engine.B
        outs = []
        for i in range(0, n, B):
            xb = x[i:i + B]
            k = xb.shape[0]
            if k < B:  # pad the tail batch
                pad = (np.zeros((B - k,) + tuple(xb.shape[1:]), np.float32)
                       if not isinstance(xb, torch.Tensor) else
                       torch.zeros((B - k,) + tuple(xb.shape[1:]), device=xb.device))
                xb = np.concatenate([xb, pad]) if not isinstance(xb, torch.Tensor) \
                    else torch.cat([xb, pad])
            outs.append(self(xb, training=False)[:k].cpu().numpy())
        return np.concatenate(outs) if outs else np.zeros((0, self.engine.H, self.engine.W, 1))

    def evaluate(self, data, verbose=0):
        """Mean loss over (x, y) batches with BN in inference mode (Keras validation). Data
        parallel: ``data`` is this rank's shard of every global batch (the provider's val
        dataset); the result is the mean over ranks, exact since the shards hold equally many
        lists."""
        losses = []
        for xb, yb in data:
            pred = self(xb, training=False)
            losses.append(float(self.loss(yb, pred).item()))
        mean = float(np.mean(losses)) if losses else float("nan")
        if self.distributed:
            from .. import dp
            t = torch.tensor([mean], dtype=torch.float64, device=self.trainer.device)
            mean = float(dp.allreduce_mean(t, self.world, self.trainer.pg).item())
        return mean

    # ------------------------------------------------------------------ weights
    def get_weights(self):
        return self.engine.get_weights()

    def set_weights(self, weights):
        self.engine.set_weights(weights)

    def save_weights(self, path):
        """``.h5`` / ``.hdf5`` / ``.keras``: the Keras HDF5 weights format (util/keras_h5.py;
        what the reference's load_weights reads, PLDepth.py:136-137). Any other path: an .npz of
        Keras-named float32 arrays (HWIO kernels) plus the Adam slots, for exact resume (the
        reference writes a TF checkpoint there, a format this build does not implement)."""
        if path.endswith((".h5", ".hdf5", ".keras")):
            from ..util import keras_h5
            keras_h5.save_weights(self.engine, path)
            return
        w = self.get_weights()
        if self.trainer is not None:
            m, v, vh = self.engine.adam_state()
            for store, name in ((m, "m"), (v, "v"), (vh, "vhat")):
                w[f"__adam__/{name}"] = store.detach().cpu().numpy()
            w["__adam__/step"] = self.trainer.step_dev.cpu().numpy()
        np.savez(path if path.endswith(".npz") else path + ".npz", **w)

    def load_weights(self, path):
        """Keras HDF5 (weights or whole-model file; detected by signature) or this build's .npz."""
        from ..util import hdf5
        if hdf5.is_hdf5(path):
            from ..util import keras_h5
            res = keras_h5.load_weights(self.engine, path)
            if self.distributed:
                self._check_replicas()
            return res
        path = path if path.endswith(".npz") else path + ".npz"
        with np.load(path, allow_pickle=False) as z:
            w = {k: z[k] for k in z.files}
        self.set_weights({k: v for k, v in w.items() if not k.startswith("__adam__")})
        if self.trainer is not None and "__adam__/m" in w:
            m, v, vh = self.engine.adam_state()
            for store, name in ((m, "m"), (v, "v"), (vh, "vhat")):
                store.copy_(torch.from_numpy(w[f"__adam__/{name}"]))
            self.trainer.step_dev.copy_(torch.from_numpy(w["__adam__/step"]))
        if self.distributed:
            self._check_replicas()

    def save(self, filepath, overwrite=True, include_optimizer=True, **kwargs):
        """keras.Model.save('... .h5') (PLDepth.py:181): model config, weights and the Adam
        slots in Keras' HDF5 model layout; ``load_model`` (models/__init__.py) reads it back.
        The loss is not persisted: a loaded model is given its loss again at ``compile()``,
        lambda weights and reduction included."""
        import os
        from ..util import keras_h5
        if not overwrite and os.path.exists(filepath):
            raise FileExistsError(filepath)
        opt = self.optimizer
        if not include_optimizer:
            self.optimizer = None
        try:
            keras_h5.save_model(self, filepath)
        finally:
            self.optimizer = opt

    def count_params(self):
        return self.engine.count_trainable()


class EffNetFullyFledged(FullyFledgedModel):
    @staticmethod
    def get_model_and_normalization(input_shape, ranking_size, loss_type=DepthLossType.NLL,
                                    batch_size=4, seed=0):
        """pl_hourglass.py:45-100. ``batch_size`` fixes the per-GPU batch the device buffers are
        laid out for (Keras builds for a dynamic batch; the reference always trains with a
        fixed one, PLDepth.py:31,129)."""
        from .effnet_ff import EffNetFF
        if loss_type not in (DepthLossType.NLL, DepthLossType.RANKING):  # the same network
            raise ValueError(f"unsupported loss type {loss_type}")
        eng = EffNetFF(tuple(input_shape), batch_size, seed=seed)
        return EffNetFullyFledged(eng, batch_size=batch_size), preprocess_input_effnet
