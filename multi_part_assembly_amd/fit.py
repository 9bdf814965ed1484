"""The epoch loop around `Trainer.train_step` — what Lightning's `Trainer.fit`, its `ModelCheckpoint(save_top_k=5)` and
its loaders do for the reference (scripts/train.py:57-120): order of the epoch, schedule, validation, checkpoints, resume.

The host stays out of the steps: the index batches are device views of `sampler.EpochSampler`, the producers take them as
they are, the running loss is a device scalar added to per step and read once per `log_every` steps and once per epoch.
`fit` and `resume` take the trainer as their first argument (`Trainer.fit` / `Trainer.resume` forward to them), and use
only its public methods, so the bookkeeping can be exercised with a stub and no device."""
from __future__ import annotations

import inspect
import os
import random
import shutil

import numpy as np
import torch

LAST = "last.pt"


def epoch_path(ckpt_dir, epoch):
    return os.path.join(ckpt_dir, f"model-epoch={epoch:03d}.pt")


def higher_is_better(monitor):
    return monitor.endswith("acc")


def save_atomic(state, path):
    """`torch.save` under a temporary name in the same directory, then `os.replace`: a reader (or a preempted writer)
    never leaves or sees half a file."""
    tmp = path + ".tmp"
    torch.save(state, tmp)
    os.replace(tmp, path)


def rng_state(device=None):
    """The host generators B-LSTM's draws and the host matching consume, and the device's torch generator."""
    state = {"torch": torch.get_rng_state(), "numpy": np.random.get_state(), "python": random.getstate()}
    if device is not None and torch.device(device).type == "cuda":
        state["cuda"] = torch.cuda.get_rng_state(device)
    return state


def set_rng_state(state, device=None):
    torch.set_rng_state(state["torch"].cpu())
    np.random.set_state(state["numpy"])
    random.setstate(state["python"])
    if "cuda" in state and device is not None and torch.device(device).type == "cuda":
        torch.cuda.set_rng_state(state["cuda"].cpu(), device)


def rank_checkpoints(kept, monitor, keep):
    """`kept`: [(epoch, score or None)] -> (the `keep` best, the rest).  Higher is better for `*acc`, lower otherwise; an
    epoch without the monitored value (no validation ran) ranks behind every epoch with one, newer before older."""
    sign = -1.0 if higher_is_better(monitor) else 1.0
    order = sorted(kept, key=lambda es: (es[1] is None, sign * es[1] if es[1] is not None else 0.0, -es[0]))
    return order[:keep], order[keep:]


def _device_of(trainer):
    flat = getattr(trainer, "flat", None)
    return flat.flat_param.device if flat is not None else None


def _eval_counters(trainer):
    model = getattr(trainer, "model", None)
    return [m._eval_calls for m in model.modules() if hasattr(m, "_eval_calls")] if model is not None else []


def checkpoint_state(trainer, sampler, producers, next_epoch, history, kept, loss_sum=0.0, loss_steps=0):
    """`Trainer.state_dict()` (so `Trainer.load_state_dict` and the evaluation tools read the file as before) plus "fit":
    what continues the RUN — the sampler's position, every producer's batch counter, the generator states, the epoch to
    continue from, the history and the checkpoints kept so far."""
    state = dict(trainer.state_dict())
    state["fit"] = {
        "next_epoch": int(next_epoch),
        "sampler": sampler.state_dict(),
        "batch_counters": [int(getattr(p, "batch_counter", 0)) for p in producers],
        "eval_calls": _eval_counters(trainer),
        "rng": rng_state(_device_of(trainer)),
        "history": list(history),
        "kept": [tuple(k) for k in kept],
        "loss_sum": float(loss_sum),
        "loss_steps": int(loss_steps),
    }
    return state


def resume(trainer, ckpt_dir):
    """Load `ckpt_dir/last.pt` if present: the trainer's state now, the rest (sampler, producer counters, generator
    states) is handed to the next `fit`, which knows the sampler and the producer.  Returns the epoch to continue from (0
    without a checkpoint)."""
    path = os.path.join(ckpt_dir, LAST) if ckpt_dir else None
    if path is None or not os.path.exists(path):
        trainer._fit_pending = None
        return 0
    state = torch.load(path, map_location=_device_of(trainer) or "cpu", weights_only=False)
    trainer.load_state_dict(state)
    trainer._fit_pending = state["fit"]
    return state["fit"]["next_epoch"]


def fit(trainer, train_producer, sampler, val_batches=None, epochs=None, val_every=None, ckpt_dir=None, keep=5,
        monitor="val/part_acc", log_every=50, on_log=None, max_steps=None, skip_limit=None, val_weights=None):
    """Train from the epoch a preceding `resume` returned (0 otherwise) up to `epochs` (default `cfg.exp.num_epochs`).

    Per epoch e: `set_epoch(e)` on trainer and sampler; `train_step(train_producer.batch(idx))` for every index batch of
    the sampler, the producer writing into `trainer.static_batch` once the step is captured and its `batch` takes `out=`;
    `check_health()` after every step; every `val_every` epochs (default `cfg.exp.val_every`; epochs e with (e + 1) %
    val_every == 0) `trainer.evaluate(val_batches)` — `val_batches` an iterable that can be walked again, or a callable
    returning one; then `model-epoch={e:03d}.pt` and `last.pt` go to `ckpt_dir`, written atomically by rank 0, and all but
    the best `keep` epoch files by `monitor` are removed.  `on_log(record)` receives a dict per `log_every` steps
    (`epoch`, `step`, `lr`, `train/loss` = the epoch's running mean) and the epoch's dict at its end.

    `max_steps`: stop after that many steps of this call as a preemption would — `last.pt` then holds the position
    inside the epoch, and a resumed run continues with the batches this one would have seen.  Returns the history: one
    dict per finished epoch (`epoch`, `lr`, `train/loss`, the validation metrics where they ran).

    With a guarded trainer (`Trainer(guard_step=True)`: non-finite or failed steps are skipped on the device) every
    `log_every` record also carries `grad_norm` (the last step's; inf for a skipped non-finite one), `skipped` and
    `skipped_in_a_row`, read in the SAME device read as the running loss; `skip_limit`: RuntimeError with the
    optimiser's `guard_report` text at a log read that finds `skipped_in_a_row >= skip_limit`.

    With a trainer that accumulates (`Trainer(accumulate=K)`, K > 1) every `train_step` is a micro-batch: `log_every`,
    `max_steps`, `step` and the sampler's position count micro-batches, `train/loss` stays the mean of the micro-batch
    losses, and `skip_limit` counts optimiser steps in a row (the guard's own word).  The epoch's last batch is passed with
    `close_window=True`, so no window spans two epochs and the learning rate of a step is one epoch's.  A run stopped by
    `max_steps` inside a window writes the open window (`Trainer.state_dict` carries its sum) and the resumed run
    continues it.

    `val_weights`: "live" or "ema" — which weights the validation passes (and so the `monitor` ranking) see; None means
    "ema" for a trainer that keeps a weight average (`Trainer(ema_decay=...)`) and "live" otherwise.  The record of an
    epoch that validated says which under "val/weights".  The checkpoints carry the average (`Trainer.state_dict`)."""
    guarded = bool(getattr(trainer, "guard_step", False))
    averaging = getattr(trainer, "average", None) is not None
    windows = getattr(trainer, "accumulate", 1) > 1  # (a trainer that knows nothing of windows is called as before)
    if val_weights is None:
        val_weights = "ema" if averaging else "live"
    if val_weights not in ("live", "ema"):
        raise ValueError(f"fit: val_weights must be 'live' or 'ema', got {val_weights!r}")
    if val_weights == "ema" and not averaging:
        raise ValueError("fit: val_weights='ema' needs a trainer that averages (Trainer(ema_decay=...) / cfg.optimizer.ema_decay)")
    if skip_limit is not None and not guarded:
        raise ValueError("fit: skip_limit needs a guarded trainer (Trainer(guard_step=True) / cfg.optimizer.skip_nonfinite)")

    def read(acc):
        """The one device read of a log interval: (running loss, the guard's figures or {})."""
        if not guarded:
            return float(acc.item()), {}
        opt = trainer.optimizer
        v = torch.cat([acc.detach().reshape(1).double(), opt.grad_norm().double(),
                       opt.guard_words()[2:4].double()]).tolist()
        return v[0], {"grad_norm": v[1], "skipped": int(v[2]), "skipped_in_a_row": int(v[3])}
    cfg = getattr(trainer, "cfg", None) or getattr(getattr(trainer, "model", None), "cfg", None)
    if epochs is None:
        epochs = cfg.exp.num_epochs
    if val_every is None:
        # configs/_base_/default_exp.py:13 of the reference: every 10 epochs unless the preset says otherwise
        val_every = cfg.exp.get("val_every", 10) if val_batches is not None else 0
    producers = [train_producer]
    takes_out = "out" in inspect.signature(train_producer.batch).parameters
    writes = getattr(trainer, "rank", 0) == 0 and ckpt_dir is not None
    if writes:
        os.makedirs(ckpt_dir, exist_ok=True)

    pending, trainer._fit_pending = getattr(trainer, "_fit_pending", None), None
    start, history, kept, loss_sum, loss_steps = 0, [], [], 0.0, 0
    if pending is not None:
        start, history, kept = pending["next_epoch"], list(pending["history"]), [tuple(k) for k in pending["kept"]]
        sampler.load_state_dict(pending["sampler"])
        for p, c in zip(producers, pending["batch_counters"]):
            if hasattr(p, "batch_counter"):
                p.batch_counter = c
        model = getattr(trainer, "model", None)
        if model is not None:
            for m, c in zip([m for m in model.modules() if hasattr(m, "_eval_calls")], pending.get("eval_calls", [])):
                m._eval_calls = c
        loss_sum, loss_steps = pending["loss_sum"], pending["loss_steps"]
        set_rng_state(pending["rng"], _device_of(trainer))  # last: nothing above draws

    def save(state, epoch_file):
        if epoch_file is not None:
            save_atomic(state, epoch_file)
            tmp = os.path.join(ckpt_dir, LAST + ".tmp")
            shutil.copyfile(epoch_file, tmp)
            os.replace(tmp, os.path.join(ckpt_dir, LAST))
        else:
            save_atomic(state, os.path.join(ckpt_dir, LAST))

    steps_run = 0
    for epoch in range(start, epochs):
        trainer.set_epoch(epoch)
        # only a position `resume` restored continues inside an epoch; a sampler left at the end of an earlier run starts anew
        resumed_inside = pending is not None and epoch == start and sampler.epoch == epoch \
            and 0 < sampler.next_step < len(sampler)
        if not resumed_inside:
            sampler.set_epoch(epoch)
            loss_sum, loss_steps = 0.0, 0
        lr = float(trainer.optimizer.lr)
        acc, acc_steps = None, 0  # the device accumulator since the last read, and the steps behind it
        for idx in sampler:
            static = trainer.static_batch if takes_out else None
            batch = train_producer.batch(idx, out=static) if static is not None else train_producer.batch(idx)
            if windows:  # no window spans two epochs: the epoch's last batch closes the one it is in
                loss = trainer.train_step(batch, close_window=sampler.next_step >= len(sampler))
            else:
                loss = trainer.train_step(batch)
            trainer.check_health()
            if acc is None:
                acc = loss.detach().clone()
            else:
                acc.add_(loss.detach())
            acc_steps += 1
            steps_run += 1
            if log_every and sampler.next_step % log_every == 0:
                value, guard_figures = read(acc)
                loss_sum, loss_steps, acc, acc_steps = loss_sum + value, loss_steps + acc_steps, None, 0
                if on_log is not None:
                    on_log({"epoch": epoch, "step": sampler.next_step, "lr": lr, "train/loss": loss_sum / loss_steps,
                            **guard_figures})
                if skip_limit is not None and guard_figures["skipped_in_a_row"] >= skip_limit:
                    report = trainer.optimizer.guard_report(getattr(trainer, "flat", None))
                    raise RuntimeError(f"fit: {guard_figures['skipped_in_a_row']} optimiser steps skipped in a row "
                                       f"(skip_limit {skip_limit}) at epoch {epoch}, step {sampler.next_step}: "
                                       + report["text"])
            if max_steps is not None and steps_run >= max_steps:
                break
        if acc is not None:  # the epoch's (or the interrupted epoch's) one read
            loss_sum, loss_steps = loss_sum + float(acc.item()), loss_steps + acc_steps
        if sampler.next_step < len(sampler):  # stopped inside the epoch: only the position is saved
            if writes:
                _check_producers(producers)
                save(checkpoint_state(trainer, sampler, producers, epoch, history, kept, loss_sum, loss_steps), None)
            return history
        record = {"epoch": epoch, "lr": lr, "train/loss": loss_sum / max(loss_steps, 1)}
        if val_every and val_batches is not None and (epoch + 1) % val_every == 0:
            batches = val_batches() if callable(val_batches) else val_batches
            # (a trainer that knows nothing of `weights` is only ever asked for its live weights, positionally as before)
            record.update(trainer.evaluate(batches) if val_weights == "live" else
                          trainer.evaluate(batches, weights=val_weights))
            record["val/weights"] = val_weights
        history.append(record)
        if on_log is not None:
            on_log(record)
        if writes:
            _check_producers(producers)
            kept.append((epoch, record.get(monitor)))
            kept, dropped = rank_checkpoints(kept, monitor, keep)
            save(checkpoint_state(trainer, sampler, producers, epoch + 1, history, kept), epoch_path(ckpt_dir, epoch))
            for old, _ in dropped:
                if os.path.exists(epoch_path(ckpt_dir, old)):
                    os.remove(epoch_path(ckpt_dir, old))
        if max_steps is not None and steps_run >= max_steps:
            break
    return history


def _check_producers(producers):
    """A batch built from a bad device index must not reach a checkpoint (the producers report it here, synchronising)."""
    for p in producers:
        if hasattr(p, "check"):
            p.check()
