"""Minimal training harness standing in for `pl.Trainer` on the hot path (the reference drives
`BaseModel.training_step` through Lightning's automatic-optimisation loop, scripts/train.py:82-120):
zero_grad -> training_step -> backward (gradient buckets all-reduced while it runs) -> fused Adam,
with the per-epoch cosine schedule.  No host synchronisation inside a step: the loss is returned as
a device tensor.

With `use_graph=True` the whole step (several hundred launches, most of them tiny) is captured once
into a HIP graph and replayed: the launch shapes are static by construction (all B*P part slots +
masks, no compaction), the batch is copied into static input tensors, and the optimiser's
per-step scalars live in device memory.  On one GPU the graph holds zero_grad + forward + backward +
Adam.  With data parallelism the step is TWO graphs cut in front of the part encoder's backward
(`DeferredBackward`): graph A = zero_grad + forward + backward of everything but the encoder, then the
all-reduce of the first gradient bucket is launched (asynchronously, on the collective's stream), graph B =
the encoder's backward runs under it, then the second bucket's all-reduce and Adam — the same two-bucket
overlap as the eager path's hooks.

Status: bit-identical to eager launches (tests/test_model_gpu.py) and stable at the full benchmark size.  Two
things make that true: the library issues no hipMemsetAsync / hipMemcpyAsync (as graph NODES they returned stale
data on replay — what an earlier revision of this note blamed on a library GEMM), and everything that must differ
between replays is read from device memory that the host refreshes before each replay: the optimiser's step
scalars (csrc/adam.hip keeps the step count on the device) and the dropout seeds (`advance_seed`).  The step is
GPU-bound, so the replay is only ~2 % faster than eager launches; eager stays the default of bench.py.

With `accumulate=K` > 1 (opt-in) a `train_step` is one micro-batch of a window of K: zero_grad, forward, backward and one
launch that keeps the window's sum beside the flat gradient (csrc/grad_accumulate.hip); the call that closes the window runs
the tail above once, on the mean.  Captured, that micro-step is ONE graph whatever K, and the tail follows it as eager
launches; data parallel, only the closing call issues a collective, one for the whole flat gradient.
"""
from __future__ import annotations

import contextlib
import warnings

import torch
import torch.distributed as dist

from . import _lib
from . import gru as _gru
from .gradsink import DeferredBackward, GradSink
from .dp import BucketedGradReducer, broadcast_from_rank0, bucket_sizes_for, ordered_parameters
from .optim import BufferSlab, FlatBuffers, FusedAdam, GradAccumulator, WeightAverage, cosine_warmup_lr, decay_mask_for


def graph_refusal(model):
    """The first reason why a step of `model` cannot be captured into a HIP graph (it keeps its launches eager), or None."""
    name = type(model).__name__
    table = (
        # identical-part matching draws its point sample on the host every step (base_model._match_parts; reference
        # base_model.py:196-238): a captured step would replay ONE draw for ever, and the capture itself would hit the
        # host copy of the match ids.  With cfg.loss.match_sample = "device" the draw is a kernel reading its counter from
        # device memory (matching.MatchSampler) and the step is captured.
        (getattr(model, "semantic", False) and getattr(model, "match_sample", "host") != "device",
         "models with semantic part matching (the matching's point sample is drawn on the host every step)"),
        # B-LSTM draws its teacher-forcing coin and its decoder noise on the host in every forward (lstm.py; reference
        # b_lstm/seq2seq.py:177-178,212-220): a captured step would replay ONE draw for ever.
        (getattr(model, "host_draws_per_forward", False),
         f"{name} (its teacher-forcing coin and decoder noise are drawn on the host every forward)"),
        # the PointNet++ encoder compacts the valid parts on the host in every forward (pointnet2.py: BatchNorm must
        # see valid parts only): the synchronisation is illegal under capture.
        (any(getattr(mod, "host_sync_per_forward", False) for mod in model.modules()),
         f"{name} (its encoder synchronises with the host in every forward to compact the valid parts)"),
    )
    return next((reason for holds, reason in table if holds), None)


# `Trainer._refuse_swapped`: what each refusal adds behind "the averaged weights are swapped in"
_SWAPPED = {"state_dict": " (inside averaged_weights()); \"model\" would hold the average and \"ema\" the live weights",
            "load_state_dict": " (inside averaged_weights())",
            "train_step": " (inside averaged_weights()); a step would train the average",
            "averaged_weights": " already"}


class Trainer:
    def __init__(self, model, cfg=None, process_group=None, use_graph=False, graph_warmup=3, guard_step=None,
                 guard_buffers=None, ema_decay=None, ema_warmup=None, accumulate=None):
        """`accumulate` (None: `cfg.optimizer.accumulate_grad_batches`, 1 where the key is absent — no preset sets it; an
        integer >= 1): an optimiser step is taken over a WINDOW of that many micro-batches, Lightning's
        `accumulate_grad_batches`.  `train_step` then runs one micro-batch per call — zero_grad, forward, backward, each
        moving BatchNorm statistics, seed positions and draw counters as a step does — and one more launch behind its
        backward (csrc/grad_accumulate.hip mpa_grad_accumulate, optim.GradAccumulator, `self.accumulator`) keeps the
        window's sum in a second flat buffer; the call that closes the window (the K-th, or an earlier one given
        `close_window=True`) leaves the sum in the flat gradient and runs the step's tail once: all-reduce, guard, update,
        commit, average, on the MEAN over the micro-batches actually in the window and over the ranks
        (`grad_scale = 1 / (world * k)`).  `self.window` is the number of micro-batches in the open window.  With 1 every
        launch, collective and result is that of a trainer built without the argument.  The guard judges the window's
        sum: one poisoned micro-batch skips the whole window, and with `guard_buffers` every buffer returns to its bits
        from before the WINDOW (the commit runs at optimiser steps only).  Data parallel: a micro-batch that does not
        close the window issues no collective, the closing one reduces the whole flat gradient in one blocking call (the
        overlap of the bucket all-reduces with backward is given up, there are K times fewer collectives).

        `ema_decay` (None: `cfg.optimizer.ema_decay`, off where the key is absent — no preset sets it) in [0, 1): an
        exponential moving average of the weights is kept on the device (optim.WeightAverage, `self.average`): one more
        launch (csrc/weight_average.hip mpa_ema_update) as the last of every optimiser step — eager, warm-up, captured
        and data-parallel steps alike — averages the flat parameters and every float32 buffer and copies the other
        buffers; `ema_warmup` (None: `cfg.optimizer.ema_warmup`, True where absent) starts with a small decay,
        min(decay, (1 + t) / (10 + t)) over the applied steps t.  A skipped step (`guard_step`) leaves the average's bits
        alone.  The buffers move into one byte slab for it (`self.buffer_slab`, as for `guard_buffers`, which shares
        the slab), so the model must not be moved or cast afterwards.  `averaged_weights()` puts the average in front of
        the model, `evaluate(weights="ema")` evaluates it, `state_dict()` carries it under "ema".

        `guard_step` (None: `cfg.optimizer.skip_nonfinite`, False where the key is absent — no preset sets it): every
        optimiser step is guarded on the device (optim.FusedAdam `guard=True`): a step whose reduced gradient holds a
        NaN or an inf, or behind which the GRU launches' status word is raised, is skipped — parameters, moments and
        the step count keep their bits — and counted.

        `guard_buffers` (None: `cfg.optimizer.skip_rollback_buffers`, False where absent — no preset sets it; needs a
        guarded step): a skipped step also rolls back every module buffer.  The buffers are re-homed here into one
        byte slab (optim.BufferSlab, `self.buffer_slab`) with a shadow beside it, and one more launch behind every
        guarded update (csrc/adam.hip mpa_guard_commit) copies live -> shadow after an applied step and shadow -> live
        after a skipped one, decided on the device by the guard's verdict — eager, warm-up, captured and data-parallel
        steps alike (every rank rolls back its own per-rank statistics on the common verdict).  The run then equals,
        buffers included, one that never saw the skipped batch.  The model must not be moved or cast afterwards
        (`BufferSlab.check()` runs here, at the capture and in `state_dict()`).

        Without `guard_buffers` forward-side state of a skipped step (BatchNorm running statistics,
        `num_batches_tracked`) is NOT rolled back: a NaN born in the forward pass reaches the running statistics.
        Never rolled back, and harmless: the dropout-seed positions (host counters; the skipped step's masks are spent,
        the next step draws fresh ones), the matching and seq2seq draw counters (rewritten from the host counter in
        front of every step) and the producers' counters (the data stream is outside the step).  The remaining hole: a
        step whose gradient is finite while a statistic overflowed to inf is applied and the statistic committed — which
        is why a guarded `state_dict()` still refuses non-finite parameters and buffers."""
        self.model = model
        refusal = graph_refusal(model) if use_graph else None
        if refusal is not None:
            warnings.warn(f"Trainer: use_graph=True is not available for {refusal}; running eager launches")
            use_graph = False
        self.use_graph, self.graph_warmup = use_graph, graph_warmup
        self._fit_pending = None  # what `resume` read for the next `fit` (fit.py)
        self._failed = False    # sticky: a `check_health` reported a launch that gave up (cleared by load_state_dict)
        self._one = None        # d loss / d loss, kept: autograd would fill a fresh ones_like every step
        self._evaluator = None  # built by the first `evaluate`
        self._graph, self._static_batch, self._static_loss, self._eager_steps = None, None, None, 0
        cfg = cfg if cfg is not None else model.cfg
        self.cfg = cfg
        opt = cfg.optimizer
        self.flat = FlatBuffers(ordered_parameters(model))
        every = opt.get("accumulate_grad_batches", 1) if accumulate is None else accumulate
        if isinstance(every, bool) or not isinstance(every, int) or every < 1:
            raise ValueError("Trainer: accumulate (cfg.optimizer.accumulate_grad_batches) must be an integer >= 1, got "
                             f"{every!r}")
        self.accumulate = every
        # the window's sum lives beside the flat gradient from now on: before any capture
        self.accumulator = GradAccumulator(self.flat) if every > 1 else None
        self.micro_batches = 0  # micro-batches this trainer has run (`optimizer.step_count` counts optimiser steps)
        self.guard_step = bool(opt.get("skip_nonfinite", False) if guard_step is None else guard_step)
        self.guard_buffers = bool(opt.get("skip_rollback_buffers", False) if guard_buffers is None else guard_buffers)
        if self.guard_buffers and not self.guard_step:
            raise ValueError("Trainer: guard_buffers=True (cfg.optimizer.skip_rollback_buffers) rolls back the buffers of "
                             "a SKIPPED step and so needs guard_step=True (cfg.optimizer.skip_nonfinite)")
        dev = self.flat.flat_param.device
        ema_decay = opt.get("ema_decay", None) if ema_decay is None else ema_decay
        self.ema_warmup = bool(opt.get("ema_warmup", True) if ema_warmup is None else ema_warmup)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        if self.ema_decay is not None and not 0.0 <= self.ema_decay < 1.0:
            raise ValueError(f"Trainer: ema_decay (cfg.optimizer.ema_decay) must lie in [0, 1), got {ema_decay}")
        # the buffers move into their slab now: the model is on its device and nothing has been captured yet (the weight
        # average needs them as one range too; only `guard_buffers` hands the slab to the optimiser for the rollback)
        self.buffer_slab = BufferSlab(model) if self.guard_buffers or self.ema_decay is not None else None
        # the status word the guard reads is the one the GRU launches raise (allocated here: before any capture)
        status = _gru.prepare(dev)[0] if self.guard_step and dev.type == "cuda" else None
        # weight decay > 0 -> AdamW with biases / normalisation weights exempt (base_model.py:394-404); clip_grad ->
        # global-norm clipping of the averaged gradient (scripts/train.py:90 gradient_clip_val)
        self.optimizer = FusedAdam(self.flat, lr=opt.lr, weight_decay=opt.weight_decay,
                                   decay_mask=decay_mask_for(model, self.flat) if opt.weight_decay > 0 else None,
                                   clip_grad=opt.get("clip_grad", None), guard=self.guard_step, launch_status=status,
                                   guard_state=self.buffer_slab if self.guard_buffers else None)
        self.schedule = None
        if opt.lr_scheduler:
            total = cfg.exp.num_epochs
            self.schedule = cosine_warmup_lr(total, int(total * opt.warmup_ratio), opt.lr,
                                             opt.lr / opt.lr_decay_factor)
        self.epoch = 0
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        broadcast_from_rank0(self.flat, model, process_group)
        if self.buffer_slab is not None:
            self.buffer_slab.refresh()  # (rank 0's buffers arrived in place: they are the state to return to)
        # the average starts as a copy of rank 0's weights, like the weights themselves
        self.average = WeightAverage(self.flat, self.buffer_slab, self.ema_decay, self.ema_warmup) \
            if self.ema_decay is not None else None
        self.optimizer.average = self.average
        self._ema_warned = False
        self.group = process_group
        # eager: bucket hooks fire during backward; graph mode: the same two buckets, reduced between / behind the two
        # graphs (the reducer only provides the bucket slices there: its hooks are switched off)
        self.reducer = BucketedGradReducer(self.flat, bucket_sizes_for(model, self.flat), process_group)
        # accumulate > 1: no bucket hooks either — a micro-batch that does not close its window issues no collective, the
        # closing one reduces the whole flat gradient behind the window's sum (`_reduce_grad`)
        hooks = not use_graph and self.accumulate == 1
        if not hooks:
            self.reducer.enabled = False
        elif self.guard_step and self.world > 1:
            self.reducer.before_reduce = self._mark_before_bucket
        self._graph_b = None
        self.sink = GradSink(on_ready=self.reducer._on_grad if hooks and self.world > 1 else None)
        # buffers the step allocates lazily (the GRU launches' status word + its pinned copy, the loss's side stream)
        # exist BEFORE a capture can see them: a pinned allocation is illegal under capture and a device word born there
        # would live in the graph's private pool
        if dev.type == "cuda":
            _gru.prepare(dev)
            for mod in model.modules():
                if hasattr(mod, "prepare_streams"):
                    mod.prepare_streams(dev)
        self.set_epoch(0)

    def check_health(self, synchronize=False):
        """RuntimeError if a cooperative launch of this step (csrc/gru.hip) gave up: its outputs, and every gradient
        behind them, are undefined.  Without `synchronize` the answer covers every launch whose status copy has already
        arrived (a plain read of pinned memory: this runs after every step and replay); with it — in front of
        checkpoints and evaluation reports — every launch issued so far.

        A guarded trainer with an open window (`accumulate` > 1) does not look unless `synchronize`: the look clears the
        status word as it reports, and the word has to stay raised until the guard gives the window's verdict."""
        if self.guard_step and self.window > 0 and not synchronize:
            return
        try:
            _gru.raise_if_failed(self.flat.flat_param.device, synchronize=synchronize)
        except RuntimeError:
            # sticky: raise_if_failed clears the status word as it reports, so a caller that catches this error and goes
            # on would otherwise get a clean bill of health — and a checkpoint — for parameters behind a failed launch
            self._failed = True
            if self.accumulator is not None:  # the open window's sum holds undefined gradients: no later step applies it
                self.accumulator.drop()
            raise

    @property
    def window(self):
        """The number of micro-batches in the open window (0: the next `train_step` starts one)."""
        return self.accumulator.window if self.accumulator is not None else 0

    # ---- guarded steps -------------------------------------------------------------------------------------------------
    def _health_and_step(self, step):
        """`check_health` and the optimiser step of a path that issues it outside a graph.  Without `guard_buffers` the look comes
        first: a launch that gave up must not reach the parameters (csrc/gru.hip's status word), and a raise leaves the
        step untaken.  With `guard_buffers` the step comes first.  `check_health` raises on the PINNED copy of the status
        word, and only that raise clears the device word, so the guard behind it still reads the word raised: verdict 2,
        the update returns at its first load and the buffers are rolled back — then the look reports the failure.  That
        is what the captured step does (its guard and commit run inside the graph, the report follows the replay), and
        it keeps the rule whole: the buffers are rolled back on every path on which the guard gave a non-zero verdict.
        Raising first would leave that step's statistics folded in with no verdict ever written."""
        if not self.guard_buffers:
            self.check_health()
            step()
        else:
            step()
            self.check_health()

    def _mark_failed_launch(self):
        """Data parallel, in front of the all-reduce of the bucket holding element 0: a status word raised on THIS rank
        becomes a NaN in the reduced gradient of every rank, which then all reach the same verdict (no extra collective)."""
        opt = self.optimizer
        _lib.launch("mpa_guard_mark", self.flat.flat_grad.device, opt.launch_status, self.flat.flat_grad, self.flat.numel)

    def _mark_before_bucket(self, bucket):
        if bucket == 0:  # (FlatBuffers order: the first bucket starts at element 0)
            self._mark_failed_launch()

    def _refuse_swapped(self, what):
        if self.average is not None and self.average.swapped:
            raise RuntimeError(f"Trainer.{what}: the averaged weights are swapped in{_SWAPPED[what]}")

    def _refuse_nonfinite_state(self):
        """Guarded trainers only, at checkpoints: a NaN / inf in a parameter (one mpa_step_guard pass over the flat
        parameters against scratch words) or in a buffer (the forward side is not guarded) must not reach a file."""
        if not self.flat.flat_param.is_cuda:
            return

        def refuse_flat(flat, whose):
            idx = self.optimizer.first_nonfinite(flat)
            if idx is not None:
                k, shape, element = self.flat.owner(idx)
                raise RuntimeError(f"Trainer.state_dict: {whose}parameter {k} (shape {shape}) "
                                   f"holds a non-finite value at element {element}; restore a "
                                   "checkpoint with load_state_dict first")

        refuse_flat(self.flat.flat_param, "")
        for name, buf in self.model.named_buffers():
            if buf.is_floating_point() and not bool(torch.isfinite(buf).all()):
                raise RuntimeError(f"Trainer.state_dict: buffer {name} holds a non-finite value (buffers are rolled back "
                                   "behind a skipped step only with guard_buffers=True, and never behind an applied one); "
                                   "restore a checkpoint with load_state_dict first")
        if self.average is not None:  # the average of an applied step follows the weights, non-finite ones included
            refuse_flat(self.average.ema_param, "the weight average of ")
            state = self.average.ema_state
            for name, (off, size, kind) in zip(self.buffer_slab.names, self.average.segments):
                if kind == 1 and not bool(torch.isfinite(state[off:off + size].view(torch.float32)).all()):
                    raise RuntimeError(f"Trainer.state_dict: the weight average of buffer {name} holds a non-finite "
                                       "value; restore a checkpoint with load_state_dict first")

    def state_dict(self):
        """Model + optimiser state for a checkpoint; refuses (RuntimeError) if a launch behind the current parameters
        gave up — now, or at any `check_health` since the parameters were last loaded.  Besides "model", "optimizer" and
        "epoch" the dictionary carries "dropout_calls": the position of every dropout-seed stream, which
        `load_state_dict` needs to continue a run with the masks the uninterrupted run draws (optional on loading)."""
        if self._failed:
            raise RuntimeError("Trainer.state_dict: an earlier check_health reported a launch that gave up; the parameters "
                               "behind it are undefined — restore a checkpoint with load_state_dict first")
        self._refuse_swapped("state_dict")
        self.check_health(synchronize=True)
        if self.buffer_slab is not None:
            self.buffer_slab.check()
        if self.guard_step:
            self._refuse_nonfinite_state()
        model_state = self.model.state_dict()
        if self.buffer_slab is not None:
            # buffers of several types are views of ONE byte slab, which `torch.save` refuses ("view the same data as
            # different types"): the checkpoint takes copies of them
            slab_views = {id(b) for b in self.model.buffers()}
            for key, b in self.model.named_buffers(remove_duplicate=False):
                if key in model_state and id(b) in slab_views:
                    model_state[key] = model_state[key].clone()
        state = {"model": model_state, "optimizer": self.optimizer.state_dict(), "epoch": self.epoch,
                 # position of every dropout-seed stream (transformer.TransformerEncoder._next_seed), in module order: a
                 # resumed run then draws the masks the uninterrupted one would have drawn
                 "dropout_calls": [m._calls for m in self.model.modules() if hasattr(m, "advance_seed")]}
        if self.average is not None:  # "model" loads into a model as it is (tools/evaluate.py --weights ema)
            state["ema"] = {"decay": self.average.decay, "warmup": self.average.warmup,
                            "model": self.average.averaged_state_dict(self.model)}
        # the open window: a run stopped inside one continues with the sum of the micro-batches it has seen
        state["accumulate"] = self.accumulator.state_dict(self.accumulate) if self.accumulator is not None else \
            {"every": 1, "window": 0, "grad": None}
        return state

    def _load_window(self, entry):
        """Behind a load of the model: the checkpoint's open window (None: an empty one).  An open window saved under
        another `accumulate` is a RuntimeError — its sum cannot be closed by this trainer's rule."""
        if self.accumulator is not None:
            self.accumulator.load_state_dict(entry, self.accumulate)
        elif entry is not None and int(entry["window"]):
            raise RuntimeError(f"Trainer.load_state_dict: the checkpoint holds an open window of {entry['window']} "
                               f"micro-batches taken with accumulate = {entry['every']}, this trainer has accumulate = 1")

    def load_state_dict(self, state):
        """Inverse of `state_dict()`: model weights and buffers (copied in place: the parameters stay views of the flat
        buffer), the optimiser's moments and step count (host and device copy) and the epoch with its learning rate.
        A Lightning-style checkpoint `{"state_dict": ...}` — what the reference's training writes — loads the weights
        only.  A restored trainer is healthy again.

        The dropout-seed positions are host counters; the device word a captured step reads its seed from is not
        restored here because `train_step` rewrites it from the counter (`advance_seed`) in front of every replay, and a
        freshly built `use_graph=True` trainer starts with its eager warm-up steps, whose seeds travel by value."""
        self._refuse_swapped("load_state_dict")
        self._load_window(state.get("accumulate"))  # (first: its refusal leaves the trainer as it was)
        if "state_dict" in state and "model" not in state:
            self.model.load_state_dict(state["state_dict"])
            self._refresh_buffer_shadow()
            self._load_average(None)
            self._failed = False
            return
        self.model.load_state_dict(state["model"])
        self._refresh_buffer_shadow()
        self._load_average(state.get("ema"))
        if state.get("optimizer") is not None:
            self.optimizer.load_state_dict(state["optimizer"])
        if self.schedule is not None:
            self.set_epoch(state["epoch"])  # (the schedule owns the rate)
        else:
            self.epoch = state["epoch"]
        seeded = [m for m in self.model.modules() if hasattr(m, "advance_seed")]
        calls = state.get("dropout_calls")
        if calls is not None:
            if len(calls) != len(seeded):
                raise RuntimeError(f"Trainer.load_state_dict: the checkpoint holds {len(calls)} dropout-seed positions, "
                                   f"the model has {len(seeded)} seeded modules")
            for m, c in zip(seeded, calls):
                m._calls = int(c)
        self._failed = False

    def _refresh_buffer_shadow(self):
        """Behind a load of the model's buffers (copied in place, so they stay views of the slab): the loaded statistics,
        not the ones from before the load, are what a skipped step returns to."""
        if self.buffer_slab is not None:
            self.buffer_slab.check()
            self.buffer_slab.refresh()

    def _load_average(self, ema):
        """Behind a load of the model: the average of before the load never stays.  With the checkpoint's "ema" entry it
        is restored (entries the entry lacks, such as non-persistent buffers, are the loaded weights'); without one it
        becomes the loaded weights, with one warning per trainer.  A trainer without averaging ignores the entry; the
        checkpoint's decay and warm-up are informational, the trainer's own hold."""
        if self.average is None:
            return
        self.average.reset()
        if ema is not None:
            self.average.load_averaged_state_dict(ema["model"], self.model)
        elif not self._ema_warned:
            self._ema_warned = True
            warnings.warn("Trainer.load_state_dict: the checkpoint holds no weight average (\"ema\"); the average restarts "
                          "from the loaded weights")

    @contextlib.contextmanager
    def averaged_weights(self):
        """Inside the block the model computes with the averaged weights and buffers (one bitwise exchange in, one out,
        also when the block raises); `train_step` and `state_dict` refuse meanwhile."""
        if self.average is None:
            raise RuntimeError("Trainer.averaged_weights: weight averaging is off (Trainer(ema_decay=...) / "
                               "cfg.optimizer.ema_decay)")
        self._refuse_swapped("averaged_weights")
        self.average.swap()
        try:
            yield self.model
        finally:
            self.average.swap()

    def evaluate(self, batches, prefix="val", weights="live"):
        """One evaluation pass over `batches` (evaluate.Evaluator on this trainer's model and process group): the
        batch-size-weighted averages as floats.  Touches neither the optimiser nor the dropout seeds of training.
        `weights="ema"`: the pass runs inside `averaged_weights()`."""
        if weights not in ("live", "ema"):
            raise ValueError(f"Trainer.evaluate: weights must be 'live' or 'ema', got {weights!r}")
        if weights == "ema":
            if self.average is None:
                raise RuntimeError("Trainer.evaluate: weights='ema' needs weight averaging (Trainer(ema_decay=...) / "
                                   "cfg.optimizer.ema_decay)")
            with self.averaged_weights():
                return self.evaluate(batches, prefix=prefix)
        from .evaluate import Evaluator
        if self._evaluator is None:
            group = self.group  # (None in a multi-rank job means the default group, as everywhere in this class)
            if group is None and self.world > 1:
                group = dist.group.WORLD
            self._evaluator = Evaluator(self.model, process_group=group, health=lambda: self.check_health(synchronize=True))
        return self._evaluator.run(batches, prefix=prefix)

    def set_epoch(self, epoch):
        self.epoch = epoch
        if self.schedule is not None:
            self.optimizer.lr = self.schedule(epoch)

    @property
    def rank(self):
        return dist.get_rank(self.group) if dist.is_initialized() else 0

    def fit(self, train_producer, sampler, val_batches=None, epochs=None, val_every=None, ckpt_dir=None, keep=5,
            monitor="val/part_acc", log_every=50, on_log=None, max_steps=None, skip_limit=None, val_weights=None):
        """The epoch loop (fit.fit has the contract): order of the epoch from `sampler` (sampler.EpochSampler), batches
        from `train_producer`, the schedule, validation every `val_every` epochs, the best `keep` checkpoints by
        `monitor` plus `last.pt` in `ckpt_dir`.  Continues from the epoch a preceding `resume` returned.  Returns the
        history, one dict per epoch."""
        from . import fit as _fit
        return _fit.fit(self, train_producer, sampler, val_batches=val_batches, epochs=epochs, val_every=val_every,
                        ckpt_dir=ckpt_dir, keep=keep, monitor=monitor, log_every=log_every, on_log=on_log,
                        max_steps=max_steps, skip_limit=skip_limit, val_weights=val_weights)

    def resume(self, ckpt_dir):
        """Load `ckpt_dir/last.pt` if it exists (model, optimiser, schedule, seed positions now; sampler position, producer
        counters and generator states when the next `fit` starts).  Returns the epoch to continue from."""
        from . import fit as _fit
        return _fit.resume(self, ckpt_dir)

    # ---- graph mode -----------------------------------------------------------------------------------
    @property
    def static_batch(self):
        """The static input tensors of the captured step (None before the capture).  A producer that writes a batch
        straight into them (`DevicePartNetProducer.batch(..., out=trainer.static_batch)`) leaves `_graph_step` nothing
        to copy: it skips every tensor whose data pointer already is the static one."""
        return self._static_batch

    def _tensor_items(self, data_dict):
        return {k: v for k, v in data_dict.items() if isinstance(v, torch.Tensor)}

    def _fwd_bwd(self, batch, loss_out=None, batch_idx=0):
        """zero_grad, forward, backward of the eager (the reducer's hooks fire inside), warm-up and one-graph captured steps."""
        # (the two-graph data-parallel capture spells them itself, in `_capture`: it is cut inside backward)
        self.optimizer.zero_grad()
        with self.sink:  # HIP backward kernels write straight into the flat gradient buffer
            loss = self.model.training_step(batch, batch_idx)
            if loss_out is not None:  # graph mode: the loss is copied out before backward recycles memory
                loss_out.copy_(loss.detach())
            # d loss / d loss, kept across steps (with a warm-up step it exists before the capture)
            if self._one is None or self._one.device != loss.device or self._one.dtype != loss.dtype:
                self._one = torch.ones((), dtype=loss.dtype, device=loss.device)
            loss.backward(self._one)
        return loss.detach() if loss_out is None else loss_out

    def _capture(self, data_dict):
        if self.buffer_slab is not None:
            self.buffer_slab.check()  # the graph bakes the buffers' addresses in: they must be the slab's
        self._static_batch = {k: v.clone() for k, v in self._tensor_items(data_dict).items()}
        self._loss_buf = torch.zeros((), dtype=torch.float32, device=self.flat.flat_param.device)
        self._graph = torch.cuda.CUDAGraph()
        if self.world == 1:
            # thread_local: RCCL's watchdog thread may touch the HIP runtime while we capture
            with torch.cuda.graph(self._graph, capture_error_mode="thread_local"):
                self._static_loss = self._fwd_bwd(self._static_batch, self._loss_buf)
                self.optimizer.step_dev()
            return
        # data parallel: graph A stops in front of the encoder's backward, graph B is the encoder's backward
        self.sink.__enter__()  # one sink (one set of use counts) across both graphs
        try:
            with torch.cuda.graph(self._graph, capture_error_mode="thread_local"):
                self.optimizer.zero_grad()
                DeferredBackward.active = []
                loss = self.model.training_step(self._static_batch, 0)
                self._loss_buf.copy_(loss.detach())
                loss.backward()
            self._static_loss = self._loss_buf
            parked = DeferredBackward.active
            if parked:
                self._check_parked_in_last_bucket(parked)
                self._graph_b = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self._graph_b, pool=self._graph.pool(), capture_error_mode="thread_local"):
                    DeferredBackward.run_all()
        finally:
            DeferredBackward.active = None
            self.sink.__exit__(None, None, None)

    def _check_parked_in_last_bucket(self, parked):
        """The two-graph overlap reduces bucket 0 WHILE the parked backward calls run: every gradient they write must
        lie in the last bucket (an encoder module living outside `model.encoder` would race with the all-reduce)."""
        buckets = self.reducer.buckets
        if len(buckets) < 2:
            return
        if len(buckets) > 2:  # (checked here, before the second graph is captured — not at the first replay)
            raise RuntimeError(f"graph-mode data parallelism overlaps exactly two gradient buckets, the reducer made "
                               f"{len(buckets)}; use use_graph=False for this model")
        last = buckets[-1]["slice"]
        base = self.flat.flat_grad.data_ptr()
        lo = (last.data_ptr() - base) // last.element_size()
        hi = lo + last.numel()
        # by the parameters' SLOTS in the flat gradient buffer, not by p.grad: a parameter whose .grad is still None (or
        # that autograd accumulates elsewhere) must not pass unchecked
        slot = {id(p): off for p, off in zip(self.flat.params, self.flat.offsets)}
        for _, _, params in parked:
            for p in params:
                if not isinstance(p, torch.Tensor):
                    continue
                off = slot.get(id(p))
                if off is None or not (lo <= off < hi):
                    raise RuntimeError("graph-mode data parallelism: a deferred encoder backward owns a parameter "
                                       "outside the last gradient bucket (an encoder module outside model.encoder?); "
                                       "use use_graph=False for this model")

    def _reduce_grad(self, second_half=None):
        """The gradient's sum over the ranks on the paths without the reducer's hooks.  No `second_half` (the warm-up step;
        a replay with nothing deferred): the whole flat gradient in one blocking call.  With it (the second graph, the
        encoder's backward): bucket 0 is reduced WHILE it runs, the encoder's bucket behind it."""
        # (never per bucket without it: a ring's summation order may depend on the slice.  A guarded step marks in front of
        # the first collective of either form: the one whose slice holds element 0)
        if self.world == 1:
            return
        buckets = self.reducer.buckets
        overlap = second_half is not None and len(buckets) > 1
        if second_half is not None:
            assert len(buckets) <= 2, "the two-graph overlap reduces only the first and the last bucket"
            if not overlap:  # one bucket: nothing to run it under
                second_half()
        if self.guard_step:
            self._mark_failed_launch()
        if second_half is None:
            dist.all_reduce(self.flat.flat_grad, group=self.group)
            return
        pending = [dist.all_reduce(buckets[0]["slice"], group=self.group, async_op=True)]
        if overlap:
            second_half()
            pending.append(dist.all_reduce(buckets[-1]["slice"], group=self.group, async_op=True))
        for work in pending:
            work.wait()

    def _graph_step(self, data_dict):
        self.model.train()
        self.optimizer.grad_scale = 1.0 / self.world
        if self._graph is None:
            if self._eager_steps < self.graph_warmup:  # let allocator / library state settle first
                self._eager_steps += 1
                loss = self._fwd_bwd(self._tensor_items(data_dict))
                self._reduce_grad()
                self._health_and_step(self.optimizer.step)
                return loss
            torch.cuda.synchronize()
            self._capture(data_dict)
        for k, v in self._tensor_items(data_dict).items():
            if v.data_ptr() != self._static_batch[k].data_ptr():
                self._static_batch[k].copy_(v, non_blocking=True)
        self.optimizer.prepare_hyper()
        for mod in self.model.modules():  # fresh dropout masks: the captured kernels read their seed from memory
            if hasattr(mod, "advance_seed"):
                mod.advance_seed()
        self._graph.replay()
        if self.world > 1:
            # (no second graph: nothing was deferred — an encoder outside the fused kernels — and one all-reduce follows)
            self._reduce_grad(self._graph_b.replay if self._graph_b is not None else None)
            self._health_and_step(self.optimizer.step_dev)  # (the optimiser step is not captured here)
        # the captured status copy refreshes the pinned word on every replay: a replay that gave up is reported here, at
        # the latest one replay later (the copy is asynchronous), and the word is cleared so that later replays run
        self.check_health()
        return self._static_loss

    # ---- gradient accumulation ------------------------------------------------------------------------------------------
    def _capture_micro(self, data_dict):
        """The ONE graph of a captured trainer with `accumulate` > 1, whatever the window's length and position: zero_grad,
        forward, backward and the accumulate launch reading its mode from the device word.  The tail stays outside, as the
        data-parallel path keeps its optimiser step outside its graphs."""
        if self.buffer_slab is not None:
            self.buffer_slab.check()
        acc = self.accumulator
        acc.mode_word.fill_(acc.IDLE)
        acc.launch()  # (writes nothing; the kernel's code object is loaded outside the capture whatever the warm-up ran)
        self._static_batch = {k: v.clone() for k, v in self._tensor_items(data_dict).items()}
        self._loss_buf = torch.zeros((), dtype=torch.float32, device=self.flat.flat_param.device)
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph, capture_error_mode="thread_local"):
            self._static_loss = self._fwd_bwd(self._static_batch, self._loss_buf)
            acc.launch()

    def _replay_micro(self, data_dict, closing):
        if self._graph is None:
            torch.cuda.synchronize()
            self._capture_micro(data_dict)
        for k, v in self._tensor_items(data_dict).items():
            if v.data_ptr() != self._static_batch[k].data_ptr():
                self._static_batch[k].copy_(v, non_blocking=True)
        # the host writes the mode in front of the replay; a window of one micro-batch replays the launch idle (mode 3
        # returns at its first load) rather than keeping a second graph without it
        size = self.accumulator.write_mode(closing)
        for mod in self.model.modules():
            if hasattr(mod, "advance_seed"):
                mod.advance_seed()
        self._graph.replay()
        return self._static_loss, size

    def _micro_step(self, data_dict, batch_idx, close_window):
        """One micro-batch of a trainer with `accumulate` > 1; the tail behind the one that closes the window."""
        acc = self.accumulator
        closing = bool(close_window) or acc.window + 1 >= self.accumulate
        self.model.train()
        try:
            replay = self.use_graph and (self._graph is not None or self._eager_steps >= self.graph_warmup)
            if replay:
                loss, size = self._replay_micro(data_dict, closing)
            else:
                if self.use_graph:
                    self._eager_steps += 1
                    loss = self._fwd_bwd(self._tensor_items(data_dict))
                else:
                    loss = self._fwd_bwd(data_dict, batch_idx=batch_idx)
                size = acc.launch_add(closing)
            if not closing:
                # unguarded: a launch that gave up is reported at its micro-batch, and `check_health` drops the window;
                # guarded: the word stays raised for the window's verdict (`check_health` does not look meanwhile)
                self.check_health()
                return loss
            # the flat gradient holds the window's sum: the tail of a step, on the mean over its micro-batches and the ranks
            self.optimizer.grad_scale = 1.0 / (self.world * size)
            self._reduce_grad()
            self._health_and_step(self.optimizer.step)
            if replay:
                self.check_health()
            return loss
        except BaseException:
            acc.drop()
            raise

    def train_step(self, data_dict, batch_idx=0, close_window=None):
        """One optimiser step on this rank's shard; returns the (detached) scalar loss tensor.

        With `accumulate` > 1: one MICRO-BATCH, whose loss is returned; the window closes, and the optimiser step is
        taken, when it holds `accumulate` micro-batches or earlier with `close_window=True` (the epoch's last batch in
        `fit`).  `close_window` means nothing to a trainer with `accumulate` = 1, whose every call is a step."""
        self._refuse_swapped("train_step")
        self.micro_batches += 1
        if self.accumulate > 1:
            return self._micro_step(data_dict, batch_idx, close_window)
        if self.use_graph:
            return self._graph_step(data_dict)
        self.model.train()
        loss = self._fwd_bwd(data_dict, batch_idx=batch_idx)  # (the reducer's hooks fire inside)
        self.optimizer.grad_scale = self.reducer.finish()
        self._health_and_step(self.optimizer.step)
        return loss
