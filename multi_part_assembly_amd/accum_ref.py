"""numpy restatement of the gradient accumulation (csrc/grad_accumulate.hip: mpa_grad_accumulate) — the specification the
kernel is tested against, bit for bit.

One optimiser step over a window of k micro-batches (Lightning's `accumulate_grad_batches`): behind every micro-batch's
backward one pass over the flat gradient `grad` and an equally long accumulator `acc`,

    FIRST (0)  acc  <- grad            the accumulator's old content is never read
    ADD   (1)  acc  <- acc + grad
    LAST  (2)  grad <- acc + grad      the sum lands in the flat gradient, where the step's tail looks

so a window of k >= 2 is FIRST, ADD x (k - 2), LAST and leaves `window_sum` = ((g0 + g1) + g2) + ... in the gradient; a
window of one micro-batch needs no pass.  Every addition is one rounded float32 operation, denormals are kept, and a mode
outside 0..2 (which only a device word can hold) writes nothing.  The mean is not taken here: 1 / k travels as the
optimiser's `grad_scale`.
"""
from __future__ import annotations

import numpy as np

FIRST, ADD, LAST = 0, 1, 2
UNIT = 16                      # bytes per lane and access
THREADS, BLOCKS = 256, 2048    # kThreads, kAccBlocks of csrc/grad_accumulate.hip


def modes(k):
    """The modes of a window of `k` micro-batches, one per micro-batch: None where no pass is issued (k == 1)."""
    if k < 1:
        raise ValueError("accum_ref.modes: a window holds at least one micro-batch")
    return [None] if k == 1 else [FIRST] + [ADD] * (k - 2) + [LAST]


def mode_at(position, closing):
    """The mode behind micro-batch `position` (0-based) of a window that this micro-batch closes or not; None: no pass."""
    if position == 0:
        return None if closing else FIRST
    return LAST if closing else ADD


def accumulate(mode, grad, acc):
    """mpa_grad_accumulate: returns (grad, acc) after the call as new arrays."""
    grad, acc = np.array(grad, copy=True), np.array(acc, copy=True)
    if grad.dtype != np.float32 or acc.dtype != np.float32 or grad.shape != acc.shape or grad.ndim != 1:
        raise ValueError("accum_ref.accumulate: two one-dimensional float32 arrays of equal size")
    if grad.size % 4:
        raise ValueError("accum_ref.accumulate: the size must be a multiple of 4 elements")
    mode = int(mode)
    with np.errstate(all="ignore"):
        if mode == FIRST:
            acc = grad.copy()
        elif mode == ADD:
            acc = acc + grad
        elif mode == LAST:
            grad = acc + grad
    return grad, acc


def window_sum(grads):
    """((g0 + g1) + g2) + ... in float32: what a window of these micro-batch gradients leaves in the flat gradient."""
    grads = [np.asarray(g) for g in grads]
    if not grads or any(g.dtype != np.float32 or g.shape != grads[0].shape for g in grads):
        raise ValueError("accum_ref.window_sum: at least one float32 array, all of one shape")
    total = grads[0].copy()
    with np.errstate(all="ignore"):
        for g in grads[1:]:
            total = total + g
    return total
