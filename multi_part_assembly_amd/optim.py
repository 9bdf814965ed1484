"""Optimiser and LR schedule of the training step.

`FusedAdam` keeps every parameter, gradient and Adam moment of the model in four flat fp32 buffers
and performs the step with one HIP kernel (csrc/adam.hip); the flat gradient buffer is also what the
data-parallel all-reduce operates on (multi_part_assembly_amd/dp.py) — one collective, no per-tensor
bookkeeping.  Replaces torch.optim.Adam/AdamW as configured by the reference
(models/modules/base_model.py:389-406).

`cosine_warmup_lr` restates the per-epoch schedule of the reference's CosineAnnealingWarmupRestarts
(utils/lr.py:26-125) for cycle_mult = gamma = 1, the only way the reference uses it
(base_model.py:411-417).
"""
from __future__ import annotations

import math

import torch

from . import _lib


class FlatBuffers:
    """Re-homes the parameters of a model (and their .grad) as views of two flat fp32 buffers.

    Device-agnostic (the gloo/CPU tests of the data-parallel path use it too).  `order` lets the
    caller group parameters into contiguous regions — the gradient buckets of dp.py."""

    def __init__(self, params):
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("FlatBuffers: no trainable parameters")
        dev = self.params[0].device
        offsets, total = [], 0
        for p in self.params:
            if p.dtype != torch.float32 or p.device != dev:
                raise RuntimeError("FlatBuffers: all parameters must be fp32 on one device")
            offsets.append(total)
            total += (p.numel() + 3) // 4 * 4  # keep every tensor 16-byte aligned
        self.numel, self.offsets = total, offsets
        self.flat_param = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros_like(self.flat_param)
        with torch.no_grad():
            for p, off in zip(self.params, offsets):
                view = self.flat_param[off:off + p.numel()].view_as(p)
                view.copy_(p)
                p.data = view
                p.grad = self.flat_grad[off:off + p.numel()].view_as(p)

    def span(self, first, last):
        """[start, end) element range covering parameters first..last (inclusive indices)."""
        return self.offsets[first], self.offsets[last] + (self.params[last].numel() + 3) // 4 * 4

    def owner(self, index):
        """(k, shape, element) of the last parameter whose offset is <= `index` (in the padding: element >= its numel)."""
        k = max(i for i, off in enumerate(self.offsets) if off <= index)
        return k, tuple(self.params[k].shape), index - self.offsets[k]

    def zero_grad(self):
        """One memset; gradients stay views of the flat buffer (never set to None)."""
        self.flat_grad.zero_()


class BufferSlab:
    """Re-homes every module buffer of a model (`model.buffers()`: BatchNorm running statistics, the int64
    `num_batches_tracked` scalars, whatever else a module registers, non-persistent ones included; a buffer shared by
    several modules once) as a view of ONE byte slab `live`, each buffer on a 16-byte boundary with zero padding, beside
    a `shadow` slab of the same size that starts as a copy.  What csrc/adam.hip mpa_guard_commit works on: behind an
    applied step shadow <- live, behind a skipped one live <- shadow, so a skipped step leaves every buffer with the bits
    it had before the step.  Kernels that write running statistics take the buffers as tensors and so write into the
    slab; a captured step bakes the slab's addresses in, which is why the slab has to exist before the first capture.

    `names`, `offsets`, `sizes` (bytes) describe the layout.  Device-agnostic like FlatBuffers: on host tensors
    `commit` is `guard_ref.commit` on the slab.  A model without buffers gives a slab of zero bytes."""

    ALIGN = 16

    def __init__(self, model):
        self.model = model
        named = list(model.named_buffers())  # (remove_duplicate: a shared buffer appears once, under its first name)
        dev = named[0][1].device if named else next((p.device for p in model.parameters()), torch.device("cpu"))
        self.names, self.offsets, self.sizes, total = [], [], [], 0
        for name, b in named:
            if b.device != dev:
                raise RuntimeError(f"BufferSlab: buffer {name} lives on {b.device}, the slab on {dev}")
            self.names.append(name)
            self.offsets.append(total)
            self.sizes.append(b.numel() * b.element_size())
            total += (self.sizes[-1] + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.nbytes = total
        self.live = torch.zeros(total, dtype=torch.uint8, device=dev)
        self._layout = []  # (name, dtype, shape) per slot, for check()
        with torch.no_grad():
            for (name, b), off, size in zip(named, self.offsets, self.sizes):
                view = self.live[off:off + size].view(b.dtype).view(b.shape)
                view.copy_(b)
                b.data = view
                self._layout.append((name, b.dtype, tuple(b.shape)))
        self.shadow = self.live.clone()
        self.check()

    def refresh(self):
        """shadow <- live: the current buffers become what a skipped step rolls back to (after a checkpoint was loaded)."""
        self.shadow.copy_(self.live)

    def launch_commit(self, guard):
        """mpa_guard_commit behind the verdict `guard[0]`, always launched (`FusedAdam.step_dev`) unless the slab is empty."""
        if self.nbytes:
            _lib.launch("mpa_guard_commit", self.live.device, guard, self.live, self.shadow, self.nbytes)

    def commit(self, guard):
        """`launch_commit` (`guard`: the optimiser's guard words on the slab's device); on host tensors its restatement."""
        if self.live.is_cuda or not self.nbytes:
            return self.launch_commit(guard)
        from .guard_ref import commit
        live, shadow = commit(int(guard[0]), self.live.numpy(), self.shadow.numpy())
        self.live.copy_(torch.from_numpy(live))
        self.shadow.copy_(torch.from_numpy(shadow))

    def check(self):
        """RuntimeError naming the buffer if a buffer of the model no longer is its view of the slab (after
        `model.to(...)`, `.float()` / `.double()`, or a module that registered a buffer anew): a rollback would then
        restore memory nobody reads."""
        slots = {name: (off, dtype, shape) for (name, dtype, shape), off in zip(self._layout, self.offsets)}
        base = self.live.data_ptr()
        now = dict(self.model.named_buffers())
        for name in slots:
            if name not in now:
                raise RuntimeError(f"BufferSlab: buffer {name} left the model after the slab was built")
        for name, b in now.items():
            if name not in slots:
                raise RuntimeError(f"BufferSlab: buffer {name} was registered after the slab was built; build the trainer "
                                   "after the model is complete")
            off, dtype, shape = slots[name]
            moved = b.numel() > 0 and b.data_ptr() != base + off
            if moved or b.dtype != dtype or tuple(b.shape) != shape or b.device != self.live.device:
                raise RuntimeError(f"BufferSlab: buffer {name} no longer lives in the slab (model.to(...), .float() or a "
                                   "re-registered buffer after the trainer was built?); a skipped step could not roll it back")


class WeightAverage:
    """An exponential moving average of a model's weights beside the live ones (csrc/weight_average.hip; timm's
    ModelEmaV2 / torch.optim.swa_utils.AveragedModel): `ema_param`, a second flat buffer, and `ema_state`, a second byte
    slab, both starting as copies of the current state.  `update` averages behind an optimiser step — one launch,
    coefficient from the device step count `hyper[4]`, nothing written behind a non-zero guard verdict; `decay` in
    [0, 1), `warmup`: d = min(decay, (1 + t) / (10 + t)).  float32 buffers are averaged, every other buffer (the int64
    `num_batches_tracked`) is copied.  `swap` exchanges live and averaged bits in place (`swapped` says which are in
    front): parameters and buffers stay views of the same memory, so kernels, GradSink and captured graphs see the
    averaged values with no re-homing.  Device-agnostic like FlatBuffers and BufferSlab: on host tensors the methods
    run the restatement `ema_ref`."""

    def __init__(self, flat, slab, decay, warmup=True):
        import ctypes
        from .ema_ref import KIND_COPY, KIND_F32, check_segments
        decay = float(decay)
        if not 0.0 <= decay < 1.0:  # (false for a NaN)
            raise ValueError(f"WeightAverage: decay must lie in [0, 1), got {decay}")
        if slab.live.device != flat.flat_param.device:
            raise RuntimeError("WeightAverage: the flat parameters and the buffer slab live on different devices")
        self.flat, self.slab, self.decay, self.warmup = flat, slab, decay, bool(warmup)
        self.ema_param = flat.flat_param.clone()
        self.ema_state = slab.live.clone()
        self.segments = [(off, size, KIND_F32 if dtype == torch.float32 else KIND_COPY)
                         for (_, dtype, _), off, size in zip(slab._layout, slab.offsets, slab.sizes)]
        check_segments(self.segments, slab.nbytes)
        words = [w for seg in self.segments for w in seg]
        self._table_host = (ctypes.c_int64 * len(words))(*words) if words else None
        self._table_dev = torch.tensor(words, dtype=torch.int64, device=flat.flat_param.device) if words else None
        self.swapped = False

    def _refuse_swapped(self, what):
        if self.swapped:
            raise RuntimeError(f"WeightAverage.{what}: the averaged weights are swapped in (swap() back first)")

    def launch_update(self, hyper, guard):
        """mpa_ema_update, wherever the tensors live (what `FusedAdam.step_dev` issues; the package's one launch of it)."""
        _lib.launch("mpa_ema_update", self.ema_param.device, self.flat.flat_param, self.ema_param, self.flat.numel,
                    self.slab.live, self.ema_state, self.slab.nbytes, self._table_host, self._table_dev, len(self.segments),
                    hyper, self.decay, int(self.warmup), guard)

    def update(self, hyper, guard=None):
        """ema <- ema + c (current - ema) behind the step whose count `hyper[4]` holds (`hyper`: the optimiser's eight
        words; `guard`: its guard words or None)."""
        self._refuse_swapped("update")
        if self.ema_param.is_cuda:
            return self.launch_update(hyper, guard)
        from .ema_ref import update
        t = int(hyper[4:5].view(torch.int32)[0])
        ema, state = update(0 if guard is None else int(guard[0]), t, self.decay, self.warmup,
                            self.flat.flat_param.detach().numpy(), self.ema_param.numpy(), self.slab.live.numpy(),
                            self.ema_state.numpy(), self.segments)
        self.ema_param.copy_(torch.from_numpy(ema))
        self.ema_state.copy_(torch.from_numpy(state))

    def swap(self):
        """Exchange live and averaged weights, bit for bit, in one launch."""
        param, live = self.flat.flat_param, self.slab.live
        if param.is_cuda:
            _lib.launch("mpa_ema_swap", param.device, param, self.ema_param, self.flat.numel * 4, live, self.ema_state,
                        self.slab.nbytes)
        else:
            with torch.no_grad():
                for a, b in ((param, self.ema_param), (live, self.ema_state)):
                    keep = a.clone()
                    a.copy_(b)
                    b.copy_(keep)
        self.swapped = not self.swapped

    def reset(self):
        """average <- current weights (after a checkpoint without an average was loaded)."""
        self._refuse_swapped("reset")
        with torch.no_grad():
            self.ema_param.copy_(self.flat.flat_param)
            self.ema_state.copy_(self.slab.live)

    def _slots(self, model):
        """state_dict key -> ("param", offset, tensor) | ("buffer", offset, tensor) for what the average holds."""
        flat_off = {id(p): off for p, off in zip(self.flat.params, self.flat.offsets)}
        first = dict(model.named_buffers())
        slab_off = {id(first[name]): off for name, off in zip(self.slab.names, self.slab.offsets) if name in first}
        slots = {}
        for key, p in model.named_parameters(remove_duplicate=False):
            if id(p) in flat_off:
                slots[key] = ("param", flat_off[id(p)], p)
        for key, b in model.named_buffers(remove_duplicate=False):
            if id(b) in slab_off:
                slots[key] = ("buffer", slab_off[id(b)], b)
        return slots

    def _view(self, kind, off, like):
        if kind == "param":
            return self.ema_param[off:off + like.numel()].view_as(like)
        return self.ema_state[off:off + like.numel() * like.element_size()].view(like.dtype).view(like.shape)

    def averaged_state_dict(self, model):
        """A dict shaped like `model.state_dict()` (same keys, same order) of CLONES, built without swapping: trainable
        parameters from the averaged flat buffer, buffers from the averaged slab, everything else (parameters with
        requires_grad=False) from the model."""
        self._refuse_swapped("averaged_state_dict")
        slots = self._slots(model)
        out = type(model.state_dict())()
        for key, value in model.state_dict().items():
            slot = slots.get(key)
            out[key] = (self._view(*slot) if slot is not None else value).detach().clone()
        return out

    def load_averaged_state_dict(self, state, model):
        """Inverse of `averaged_state_dict`: every key the average holds is copied in; a missing one is a KeyError.
        Entries the average does not hold (frozen parameters) are ignored."""
        self._refuse_swapped("load_averaged_state_dict")
        slots = self._slots(model)
        wanted = [k for k in model.state_dict() if k in slots]
        missing = [k for k in wanted if k not in state]
        if missing:
            raise KeyError(f"WeightAverage.load_averaged_state_dict: missing {missing[:3]}{'...' if len(missing) > 3 else ''}")
        with torch.no_grad():
            for key in wanted:
                self._view(*slots[key]).copy_(state[key])


class GradAccumulator:
    """The sum of a window of micro-batch gradients beside the flat gradient (csrc/grad_accumulate.hip; Lightning's
    `accumulate_grad_batches`): `acc`, a second flat buffer allocated here (before any capture), `mode_word`, the int32
    device word a captured launch reads its mode from (written with `fill_`, as the learning rate is; `IDLE` = 3 writes
    nothing), and `window`, the number of micro-batches the open window holds.  Behind the backward of every micro-batch
    `launch_add(closing)` issues the package's one launch of mpa_grad_accumulate — FIRST, ADD, ..., LAST (`accum_ref.mode_at`),
    none for a window that closes at its first micro-batch — and returns the window's size when it closed it, so the
    flat gradient then holds the window's sum and the caller takes the step with `grad_scale = 1 / (world * size)`.
    Device-agnostic like FlatBuffers: on host tensors `add` runs the restatement `accum_ref`."""

    IDLE = 3

    def __init__(self, flat):
        self.flat = flat
        self.acc = torch.zeros_like(flat.flat_grad)
        self.mode_word = torch.full((1,), self.IDLE, dtype=torch.int32, device=flat.flat_grad.device)
        self.window = 0

    def _advance(self, closing):
        from .accum_ref import mode_at
        mode = mode_at(self.window, closing)
        self.window += 1
        size = self.window
        if closing:
            self.window = 0
        return mode, (size if closing else None)

    def launch(self, mode=None):
        """mpa_grad_accumulate, wherever the tensors live: `mode` by value, or (None) from `mode_word`."""
        _lib.launch("mpa_grad_accumulate", self.acc.device, self.flat.flat_grad, self.acc, self.flat.numel,
                    0 if mode is None else int(mode), self.mode_word if mode is None else None)

    def launch_add(self, closing):
        """The micro-batch whose gradient the flat buffer holds joins the window (one launch, by value; none for a window
        of one).  Returns the window's size if `closing`, else None."""
        mode, size = self._advance(closing)
        if mode is not None:
            self.launch(mode)
        return size

    def write_mode(self, closing):
        """`launch_add` for a captured launch: only the mode word is written (IDLE for a window of one); the replay of
        the graph that holds `launch()` does the rest."""
        mode, size = self._advance(closing)
        self.mode_word.fill_(self.IDLE if mode is None else mode)
        return size

    def add(self, closing):
        """`launch_add`; on host tensors its restatement."""
        if self.acc.is_cuda:
            return self.launch_add(closing)
        from .accum_ref import accumulate
        mode, size = self._advance(closing)
        if mode is not None:
            grad, acc = accumulate(mode, self.flat.flat_grad.detach().numpy(), self.acc.numpy())
            self.flat.flat_grad.copy_(torch.from_numpy(grad))
            self.acc.copy_(torch.from_numpy(acc))
        return size

    def drop(self):
        """Forget the open window (its sum holds undefined gradients): the next micro-batch starts one with FIRST."""
        self.window = 0

    def state_dict(self, every):
        return {"every": int(every), "window": self.window, "grad": self.acc.clone() if self.window else None}

    def load_state_dict(self, state, every):
        """A missing entry (None) means an empty window; an open window saved under another `every` is refused."""
        window = int(state["window"]) if state is not None else 0
        if window and int(state["every"]) != int(every):
            raise RuntimeError(f"GradAccumulator.load_state_dict: the checkpoint holds an open window of {window} "
                               f"micro-batches taken with accumulate = {state['every']}, this trainer has accumulate = "
                               f"{every}; finish the window first or build the trainer with the checkpoint's value")
        if window:
            if window >= int(every) or state.get("grad") is None:
                raise RuntimeError(f"GradAccumulator.load_state_dict: an open window of {window} micro-batches needs its "
                                   f"sum and accumulate > {window}")
            self.acc.copy_(state["grad"])
        self.window = window


def decay_mask_for(model, flat: "FlatBuffers"):
    """1/0 per element of the flat parameter buffer: the reference's AdamW parameter groups (utils/utils.py:90-125
    `filter_wd_parameters`) exempt every bias and the weights of normalisation layers from weight decay."""
    import torch.nn as nn
    norm_types = (nn.LayerNorm, nn.GroupNorm, nn.modules.batchnorm._BatchNorm, nn.modules.instancenorm._InstanceNorm)
    no_decay = set()
    for m in model.modules():
        if isinstance(m, norm_types) and getattr(m, "weight", None) is not None:
            no_decay.add(id(m.weight))
        if getattr(m, "bias", None) is not None and isinstance(m.bias, torch.Tensor):
            no_decay.add(id(m.bias))
    mask = torch.zeros_like(flat.flat_param)
    for p, off in zip(flat.params, flat.offsets):
        if id(p) not in no_decay:
            mask[off:off + p.numel()] = 1.0
    return mask


class FusedAdam:
    """One-kernel Adam / AdamW over FlatBuffers.  `step()` = `prepare_hyper()` + `step_dev()`: the step count and
    the bias corrections live in DEVICE memory and are advanced by the library on the stream (csrc/adam.hip), so
    neither eager steps nor HIP-graph replays upload per-step scalars from the host — a host that runs steps ahead
    of the GPU cannot corrupt a queued update.  Learning rate and grad_scale are written with `fill_` (the value
    travels as a kernel argument) only when they change.

    `grad_scale`: what the flat gradient, a SUM, is multiplied by inside the update: 1 / world for the mean over the ranks,
    1 / (world * k) behind a window of k accumulated micro-batches (`GradAccumulator`); it travels through `hyper[3]`.

    `decay_mask`: optional flat 1/0 tensor (see `decay_mask_for`).  `clip_grad`: global-norm clipping of the
    (mean) gradient, the reference's `gradient_clip_val` (scripts/train.py:90).

    `guard=True`: `step_dev()` looks at the gradient first (csrc/adam.hip mpa_step_guard: one pass that is also the
    clipping's norm) and SKIPS the step on the device — parameters, moments, step count and bias corrections keep their
    bits — when the gradient holds a NaN or an inf, or when `launch_status` (an int32 device word, e.g. the GRU launches'
    status word) is raised.  What the reference gets from Lightning's GradScaler in its `--fp16` runs.  Eight device
    words count what happened (`guard_words()`, `guard_report()`).

    `guard_state` (a `BufferSlab`, needs `guard=True`): `step_dev()` issues mpa_guard_commit on the slab directly behind
    the guarded update, so a skipped step also leaves every module buffer (BatchNorm running statistics,
    `num_batches_tracked`, ...) with the bits it had before the step, and an applied step makes the current ones the
    state to return to.  Without it the buffers keep what the skipped step's forward wrote.  Host-side counters
    (dropout-seed positions, draw counters, the producers') are never rolled back: the skipped step's draws are spent
    and the next step draws fresh ones.

    `average` (a `WeightAverage` over the same flat buffer; may be assigned after construction): `step_dev()` issues
    mpa_ema_update as its LAST launch — behind the update, and behind mpa_guard_commit where that runs — with the guard words
    when `guard=True`, so the average of a skipped step keeps its bits.  One launch more per step, none without it."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 decoupled_weight_decay=None, decay_mask=None, clip_grad=None, guard=False, launch_status=None,
                 guard_state=None, average=None):
        if guard_state is not None and not guard:
            raise ValueError("FusedAdam: guard_state (the buffer slab a skipped step rolls back) needs guard=True")
        self.flat = params if isinstance(params, FlatBuffers) else FlatBuffers(params)
        self.params = self.flat.params
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        # the reference switches to AdamW as soon as weight_decay > 0 (base_model.py:394-404)
        self.decoupled = (weight_decay > 0) if decoupled_weight_decay is None else decoupled_weight_decay
        self.decay_mask = decay_mask
        self.clip_grad = clip_grad if clip_grad else None
        self._clip_ws = None
        self._clip_written = False  # the device-side clip coefficient holds a value other than 1
        self._step_count = 0
        self.grad_scale = 1.0
        self.numel = self.flat.numel
        self.flat_param, self.flat_grad = self.flat.flat_param, self.flat.flat_grad
        self.exp_avg = torch.zeros_like(self.flat_param)
        self.exp_avg_sq = torch.zeros_like(self.flat_param)
        self._hyper_dev, self._uploaded = None, (None, None)
        self.guard, self.launch_status, self.guard_state = bool(guard), launch_status, guard_state
        self.average = average
        # the eight guard words live from construction on (a checkpoint may be loaded before the first step)
        self._guard_dev = torch.zeros(8, dtype=torch.int32, device=self.flat_param.device) if self.guard else None
        self._guard_ws = None

    def zero_grad(self):
        self.flat.zero_grad()

    # ---- device-resident hyper-parameters -----------------------------------------------------------------
    def _ensure_hyper(self):
        if self._hyper_dev is None:
            dev = self.flat_param.device
            if dev.type != "cuda":
                raise RuntimeError("FusedAdam.step: parameters must live on the GPU (HIP kernel only)")
            self._hyper_dev = torch.zeros(8, dtype=torch.float32, device=dev)
            self._hyper_dev[5] = 1.0  # clip coefficient: no clipping
            self._set_device_step(self._step_count)
        if self.guard:
            self.guard_workspace()

    def guard_workspace(self):  # (mpa_step_guard's partial sums and first-bad indices, allocated on first use)
        if self._guard_ws is None:
            self._guard_ws = torch.empty(_lib.query("mpa_step_guard_workspace") // 4, dtype=torch.int32,
                                         device=self.flat_param.device)
        return self._guard_ws

    @property
    def step_count(self):
        return self._step_count

    @step_count.setter
    def step_count(self, value):
        """The device keeps its own copy (bias corrections are computed there): assigning re-synchronises it."""
        self._step_count = int(value)
        if self._hyper_dev is not None:
            self._set_device_step(self._step_count)

    def _ensure_clip_ws(self):
        """Allocated on first use, so `clip_grad` may be assigned after construction or after the first step."""
        if self._clip_ws is None:
            self._clip_ws = torch.empty(_lib.query("mpa_grad_clip_workspace") // 8, dtype=torch.float64,
                                        device=self.flat_param.device)

    def _set_device_step(self, step):
        self._hyper_dev[4:5].view(torch.int32).fill_(int(step))

    def prepare_hyper(self):
        """Host-side bookkeeping in front of `step_dev`: advances the host mirror of the step count and rewrites
        lr / grad_scale on the device when they changed (fill_: no host staging buffer involved)."""
        self._ensure_hyper()
        self._step_count += 1  # (the device advances its own counter inside step_dev)
        if self._uploaded != (float(self.lr), float(self.grad_scale)):
            self._hyper_dev[0:1].fill_(float(self.lr))
            self._hyper_dev[3:4].fill_(float(self.grad_scale))
            self._uploaded = (float(self.lr), float(self.grad_scale))

    def step_dev(self):
        """[clip coefficient +] step-count advance + Adam update [+ weight average], all on the stream (safe to capture
        in a HIP graph: every launch argument is constant across replays)."""
        self._update_dev()
        if self.average is not None:  # last: behind the advance of the step count and the commit of the buffers
            self.average.launch_update(self._hyper_dev, self._guard_dev)

    def _update_dev(self):
        dev = self.flat_param.device
        if self.guard:
            # pass + verdict / coefficient / advance, then the update that returns at once behind a non-zero verdict
            # (clipping off: one launch more than advance + update; clipping on: one fewer than its four)
            self._clip_written = bool(self.clip_grad)  # (the verdict kernel rewrites the coefficient in every step)
            _lib.launch("mpa_step_guard", dev, self.flat_grad, self.numel, float(self.clip_grad or 0.0),
                        self._hyper_dev.data_ptr() + 12, 1.0, self.launch_status, self.guard_workspace(), self._hyper_dev,
                        self._guard_dev, float(self.betas[0]), float(self.betas[1]))
            _lib.launch("mpa_adam_step_guarded", dev, self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq,
                        self.numel, self._hyper_dev, float(self.betas[0]), float(self.betas[1]), float(self.eps),
                        float(self.weight_decay), int(self.decoupled), self.decay_mask, self._guard_dev)
            if self.guard_state is not None:  # applied: shadow <- live; skipped: live <- shadow (same verdict word)
                self.guard_state.launch_commit(self._guard_dev)
            return
        if not self.clip_grad and self._clip_written:  # clipping was switched off: back to "no clipping"
            self._hyper_dev[5:6].fill_(1.0)
            self._clip_written = False
        if self.clip_grad:
            self._ensure_clip_ws()
            self._clip_written = True
            _lib.launch("mpa_grad_clip_coef", dev, self.flat_grad, self.numel, float(self.clip_grad),
                        self._hyper_dev.data_ptr() + 12, 1.0, self._clip_ws, self._hyper_dev.data_ptr() + 20)
        _lib.launch("mpa_adam_step_dev", dev, self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, self.numel,
                    self._hyper_dev, float(self.betas[0]), float(self.betas[1]), float(self.eps),
                    float(self.weight_decay), int(self.decoupled), self.decay_mask)

    def step(self, lr=None):
        if lr is not None:
            self.lr = lr
        self.prepare_hyper()
        self.step_dev()

    # ---- the guard's eight words ----------------------------------------------------------------------------------------
    def guard_words(self):
        """The eight int32 guard words (include/mpa_hip.h, guard_ref.WORDS) as a DEVICE tensor: no synchronisation."""
        if not self.guard:
            raise RuntimeError("FusedAdam.guard_words: the optimiser was built with guard=False")
        return self._guard_dev

    def grad_norm(self):
        """hyper[6] as a one-element DEVICE view: the norm of the last step's (scaled) gradient, +inf for a non-finite
        one.  Written by every guarded step (by the clipping alone without the guard)."""
        self._ensure_hyper()
        return self._hyper_dev[6:7]

    def first_nonfinite(self, flat_tensor):
        """The smallest index of a NaN / inf in `flat_tensor` (on the device, of the flat buffers' length) or None: one
        mpa_step_guard pass against scratch words — the optimiser's own count and words stay — and one device read."""
        dev = flat_tensor.device
        hyper, words = torch.zeros(8, dtype=torch.float32, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)
        _lib.launch("mpa_step_guard", dev, flat_tensor, self.numel, 0.0, None, 1.0, None, self.guard_workspace(), hyper,
                    words, float(self.betas[0]), float(self.betas[1]))
        verdict, _, _, _, idx = words[:5].tolist()
        return idx if verdict else None

    def guard_report(self, flat=None):
        """One device read: the words by name, plus `parameter` (index into `flat.params`), `shape` and `element` of the
        tensor owning `first_bad_index` (resolved through `FlatBuffers.owner`; None when the last skip was the status
        word's alone, or nothing was skipped) and a one-line `text`."""
        from .guard_ref import LAUNCH_FAILED, NONFINITE, describe
        flat = flat if flat is not None else self.flat
        rep = describe(self.guard_words().tolist())
        rep.update(parameter=None, shape=None, element=None)
        idx = rep["first_bad_index"]
        if rep["skipped"] and idx >= 0:
            rep.update(zip(("parameter", "shape", "element"), flat.owner(idx)))
        if not rep["skipped"]:
            rep["text"] = f"{rep['applied']} steps applied, none skipped"
        else:
            why = []
            if rep["verdicts_or"] & NONFINITE:
                why.append("non-finite gradient")
            if rep["verdicts_or"] & LAUNCH_FAILED:
                why.append("raised launch status word")
            where = (f"first non-finite gradient element: flat index {idx} = element {rep['element']} of parameter "
                     f"{rep['parameter']} (shape {rep['shape']})") if rep["parameter"] is not None else \
                "the launch status word alone"
            rep["text"] = (f"{rep['applied']} steps applied, {rep['skipped']} skipped ({' / '.join(why)} seen), "
                           f"{rep['skipped_in_a_row']} in a row; last skipped attempt {rep['last_skipped_attempt']}: {where}")
        return rep

    def state_dict(self):
        state = {"step": self.step_count, "lr": self.lr, "exp_avg": self.exp_avg.clone(),
                 "exp_avg_sq": self.exp_avg_sq.clone()}
        if self.guard:
            # the host mirror counts ATTEMPTS once steps can be skipped: the applied count is the device's (one read, at
            # a checkpoint, which synchronises anyway)
            if self._hyper_dev is not None:
                state["step"] = int(self._hyper_dev[4:5].view(torch.int32).item())
            state["guard"] = self._guard_dev.clone()
        return state

    def load_state_dict(self, state):
        self.step_count, self.lr = state["step"], state["lr"]  # (the setter re-synchronises the device counter)
        self.exp_avg.copy_(state["exp_avg"])
        self.exp_avg_sq.copy_(state["exp_avg_sq"])
        if self.guard:  # (a checkpoint without the words: counting starts at zero)
            if state.get("guard") is not None:
                self._guard_dev.copy_(state["guard"])
            else:
                self._guard_dev.zero_()


def cosine_warmup_lr(total_epochs, warmup_epochs, max_lr, min_lr):
    """epoch -> learning rate.  Epoch 0 runs at `min_lr` (the reference scheduler resets the rate
    to min_lr at the end of its constructor, utils/lr.py:68-75), later epochs follow the linear
    warm-up / half-cosine of utils/lr.py:77-91 and restart every `total_epochs`."""
    assert warmup_epochs < total_epochs

    def lr_at(epoch):
        if epoch <= 0:
            return min_lr
        s = epoch % total_epochs
        if s < warmup_epochs:
            return (max_lr - min_lr) * s / warmup_epochs + min_lr
        phase = (s - warmup_epochs) / (total_epochs - warmup_epochs)
        return min_lr + (max_lr - min_lr) * (1 + math.cos(math.pi * phase)) / 2

    return lr_at
