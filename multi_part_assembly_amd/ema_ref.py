"""numpy restatement of the weight average (csrc/weight_average.hip: mpa_ema_update, mpa_ema_swap) — the specification
the kernels are tested against, bit for bit.

An exponential moving average of the weights, as timm's ModelEmaV2 and torch.optim.swa_utils.AveragedModel keep it, updated
behind every APPLIED optimiser step: e <- e + (1 - d) (p - e).  The step count t is the optimiser's applied-step count AFTER
this step's advance (t >= 1); with `warmup` the decay starts small, d = min(decay, (1 + t) / (10 + t)), so the first
steps are not dominated by the initial weights.  Every operation is one rounded float32 operation, no fused multiply-add.

The state of a model is two ranges: the flat float32 parameter buffer (optim.FlatBuffers) and the byte slab of the module
buffers (optim.BufferSlab), described by `segments` = [(byte offset, byte size, kind)]: kind `KIND_F32` is averaged like
the parameters, kind `KIND_COPY` (int64 counters, flags, anything else) is copied bit for bit.  A segment's slot reaches
from its offset to its end rounded up to 16 bytes; the bytes behind `size` (the slab's zero padding) are copied.  A
non-zero guard verdict (guard_ref: the step was skipped) leaves every bit of the average alone.
"""
from __future__ import annotations

import numpy as np

KIND_COPY, KIND_F32 = 0, 1
UNIT = 16                      # bytes per lane and access, the granularity of both kernels
THREADS, BLOCKS = 256, 2048    # kThreads, kEmaBlocks of csrc/weight_average.hip


def coefficient(t, decay, warmup):
    """c = 1 - d as float32 for the applied-step count `t` (an int32)."""
    f = np.float32
    a = f(np.int32(t))
    with np.errstate(all="ignore"):
        q = (f(1.0) + a) / (f(10.0) + a)
        d = np.fmin(f(decay), q) if warmup else f(decay)
        return f(f(1.0) - d)


def _average(p, e, c):
    with np.errstate(all="ignore"):
        diff = p - e
        return e + c * diff


def check_segments(segments, state_bytes):
    """ValueError unless the slots start on 16-byte boundaries, ascend without overlap and lie inside the slab."""
    end = 0
    for k, (off, size, kind) in enumerate(segments):
        slot = (size + UNIT - 1) // UNIT * UNIT
        if off < 0 or off % UNIT:
            raise ValueError(f"ema_ref: segment {k} does not start on a 16-byte boundary")
        if size < 0 or off + slot > state_bytes:
            raise ValueError(f"ema_ref: segment {k} leaves the slab")
        if off < end:
            raise ValueError(f"ema_ref: segment {k} overlaps the one before it")
        if kind not in (KIND_COPY, KIND_F32) or (kind == KIND_F32 and size % 4):
            raise ValueError(f"ema_ref: segment {k}: kind must be 0 (copied) or 1 (float32, a multiple of 4 bytes)")
        end = off + slot


def update(verdict, t, decay, warmup, param, ema, live, ema_state, segments):
    """mpa_ema_update: returns (ema, ema_state) after the call as new arrays.  `param`, `ema`: float32 vectors of equal
    size; `live`, `ema_state`: uint8 vectors of equal size, a multiple of 16 (empty for a model without buffers)."""
    param, live = np.asarray(param), np.asarray(live)
    ema, ema_state = np.array(ema, copy=True), np.array(ema_state, copy=True)
    if param.dtype != np.float32 or ema.dtype != np.float32 or param.shape != ema.shape or param.ndim != 1:
        raise ValueError("ema_ref.update: two one-dimensional float32 arrays of equal size")
    if live.dtype != np.uint8 or ema_state.dtype != np.uint8 or live.shape != ema_state.shape or live.ndim != 1:
        raise ValueError("ema_ref.update: two one-dimensional uint8 arrays of equal size")
    if live.size % UNIT or param.size % 4:
        raise ValueError("ema_ref.update: the slab must be a multiple of 16 bytes, the parameters a multiple of 4 elements")
    if not 0.0 <= float(decay) < 1.0:
        raise ValueError("ema_ref.update: decay must lie in [0, 1)")
    check_segments(segments, live.size)
    if int(verdict) != 0:
        return ema, ema_state
    c = coefficient(t, decay, warmup)
    ema = _average(param, ema, c)
    for off, size, kind in segments:
        end = off + (size + UNIT - 1) // UNIT * UNIT
        old = ema_state[off:off + size].copy()
        ema_state[off:end] = live[off:end]
        if kind == KIND_F32:
            p = live[off:off + size].copy().view(np.float32)
            ema_state[off:off + size] = _average(p, old.view(np.float32), c).view(np.uint8)
    return ema, ema_state


def swap(a, b):
    """One pair of mpa_ema_swap: returns (a, b) after the call as new arrays — each with the other's bits."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or a.ndim != 1:
        raise ValueError("ema_ref.swap: two one-dimensional arrays of equal size and type")
    if a.nbytes % UNIT:
        raise ValueError("ema_ref.swap: the size must be a multiple of 16 bytes")
    return b.copy(), a.copy()
