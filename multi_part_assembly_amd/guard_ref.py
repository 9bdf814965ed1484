"""numpy restatement of the guarded optimiser step (csrc/adam.hip: mpa_step_guard, mpa_adam_step_guarded,
mpa_guard_mark) — the specification the kernels are tested against, word for word and bit for bit.

A step is SKIPPED when its flat gradient holds a NaN or an inf (verdict bit 0) or when the launches' status word is
raised (bit 1): parameters, both Adam moments, the step count and the bias corrections keep their bits.  The reference
gets the first half from Lightning's GradScaler in its documented `--fp16` runs (docs/model.md:76,95,123).

`sum_of_squares` walks the gradient in the kernel's order (512 blocks of 256 threads, a float4 per thread and grid
stride, a three-element tail, a binary tree per block, the blocks added in index order), so the coefficient and the norm
come out with the device's bits: every operation is one IEEE double operation (a float's square is exact in double).

`commit` restates mpa_guard_commit, the buffer rollback behind the verdict (optim.BufferSlab): an applied step makes the
live bytes the shadow, a skipped one makes the shadow the live bytes; `run_steps` carries a slab through a sequence of steps.
"""
from __future__ import annotations

import numpy as np

BLOCKS, THREADS = 512, 256          # kNormBlocks, kThreads of csrc/adam.hip
NONFINITE, LAUNCH_FAILED = 1, 2     # the verdict's bits
WORDS = ("verdict", "applied", "skipped", "skipped_in_a_row", "first_bad_index", "last_skipped_attempt", "verdicts_or",
         "reserved")


def sum_of_squares(grad):
    """Double sum of squares of the float32 vector `grad`, in the order of the device's two-stage sum."""
    g = np.ascontiguousarray(grad, dtype=np.float32).astype(np.float64)
    n = g.size
    n4, stride = n // 4, BLOCKS * THREADS
    with np.errstate(over="ignore", invalid="ignore"):
        sq = g * g
        q = sq[:4 * n4].reshape(n4, 4)
        q = ((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]                # one term per float4, left to right
        rounds = -(-n4 // stride)
        q = np.concatenate([q, np.zeros(rounds * stride - n4)]).reshape(rounds, stride)
        acc = np.zeros(stride)
        for r in range(rounds):                                        # a thread's grid-stride loop (+0.0 changes nothing)
            acc = acc + q[r]
        tail = sq[4 * n4:]
        acc[:tail.size] = acc[:tail.size] + tail                       # threads 0..2 of block 0
        red = acc.reshape(BLOCKS, THREADS).copy()
        o = THREADS // 2
        while o > 0:
            red[:, :o] = red[:, :o] + red[:, o:2 * o]
            o //= 2
        s = np.float64(0.0)
        for b in range(BLOCKS):
            s = s + red[b, 0]
    return s


def first_nonfinite(grad):
    """Smallest flat index of a NaN / +-inf element, or -1."""
    bad = np.flatnonzero(~np.isfinite(np.asarray(grad, dtype=np.float32)))
    return int(bad[0]) if bad.size else -1


def clip_coefficient(s, max_norm, scale):
    """(hyper[5], hyper[6]) as float32 for the FINITE double sum of squares `s`: torch.nn.utils.clip_grad_norm_'s
    coefficient on the norm of the scaled gradient; max_norm <= 0 means no clipping."""
    norm = np.sqrt(np.float64(s)) * np.float64(np.float32(scale))
    c = np.float64(np.float32(max_norm)) / (norm + np.float64(1e-6))
    with np.errstate(over="ignore"):  # (the norm of a few elements near the largest float exceeds a float: inf, as on the device)
        coef = np.float32(c) if (max_norm > 0 and c < 1.0) else np.float32(1.0)
        return coef, np.float32(norm)


def new_hyper(lr=1e-3, grad_scale=1.0, step=0, beta1=0.9, beta2=0.999):
    """The 8-float hyper buffer of mpa_adam_step_dev as a float32 array ([4] carries the step count's int32 bits)."""
    h = np.zeros(8, dtype=np.float32)
    h[0], h[3], h[5] = lr, grad_scale, 1.0
    h[4:5].view(np.int32)[0] = step
    if step > 0:
        h[1] = np.float32(1.0 - np.float64(np.float32(beta1)) ** step)
        h[2] = np.float32(np.sqrt(1.0 - np.float64(np.float32(beta2)) ** step))
    return h


def step_guard(grad, max_norm, scale, launch_status, hyper, guard, beta1=0.9, beta2=0.999):
    """mpa_step_guard: updates `hyper` (float32[8]) and `guard` (int32[8]) in place and returns the verdict.
    `launch_status`: None (NULL) or the value of the status word."""
    s = sum_of_squares(grad)
    nonfinite = not np.isfinite(s)
    verdict = (NONFINITE if nonfinite else 0) | (LAUNCH_FAILED if launch_status is not None and launch_status != 0 else 0)
    if nonfinite:
        hyper[5], hyper[6] = np.float32(1.0), np.float32(np.inf)
    else:
        hyper[5], hyper[6] = clip_coefficient(s, max_norm, scale)
    guard[0] = verdict
    if verdict == 0:
        guard[1] += 1
        guard[3] = 0
        step = int(hyper[4:5].view(np.int32)[0]) + 1                   # adam_advance_kernel
        hyper[4:5].view(np.int32)[0] = step
        hyper[1] = np.float32(1.0 - np.float64(np.float32(beta1)) ** step)
        hyper[2] = np.float32(np.sqrt(1.0 - np.float64(np.float32(beta2)) ** step))
    else:
        guard[2] += 1
        guard[3] += 1
        guard[4] = first_nonfinite(grad) if nonfinite else -1
        guard[5] = guard[1] + guard[2]
    guard[6] |= verdict
    guard[7] = 0
    return verdict


def adam_step_guarded(param, grad, exp_avg, exp_avg_sq, hyper, guard, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
                      decoupled=False, decay_mask=None):
    """mpa_adam_step_guarded on float32 arrays, in place: the identity when guard[0] != 0, else torch.optim.Adam's
    single-tensor update term by term in float32 (csrc/adam.hip `adam_one`)."""
    if guard[0] != 0:
        return
    f = np.float32
    lr, bc1, bc2_sqrt = f(hyper[0]), f(hyper[1]), f(hyper[2])
    b1, b2 = f(beta1), f(beta2)
    g = grad.astype(np.float32) * (f(hyper[3]) * f(hyper[5]))
    wd = np.full_like(param, f(weight_decay)) * (decay_mask.astype(np.float32) if decay_mask is not None and weight_decay
                                                 else f(1.0))
    if decoupled:
        param[...] = np.where(wd != 0, param * (f(1.0) - lr * wd), param)
    else:
        g = np.where(wd != 0, g + wd * param, g)
    exp_avg[...] = exp_avg + (g - exp_avg) * (f(1.0) - b1)
    exp_avg_sq[...] = exp_avg_sq * b2 + (g * g) * (f(1.0) - b2)
    denom = np.sqrt(exp_avg_sq) / bc2_sqrt + f(eps)
    param[...] = param - (lr / bc1) * (exp_avg / denom)


def guard_mark(launch_status, grad):
    """mpa_guard_mark: a raised status word becomes a quiet NaN in element 0 of the gradient."""
    if launch_status != 0:
        grad[0] = np.float32(np.nan)


COMMIT_BLOCKS, COMMIT_UNIT = 512, 16  # kCommitBlocks of csrc/adam.hip (blocks of THREADS threads), bytes per unit


def commit(verdict, live, shadow):
    """mpa_guard_commit on two numpy byte arrays of equal size: returns (live, shadow) after the call, as new arrays.
    verdict == 0 (the step was applied): shadow <- live; anything else (skipped): live <- shadow.  Bit for bit."""
    live, shadow = np.asarray(live), np.asarray(shadow)
    if live.dtype != np.uint8 or shadow.dtype != np.uint8 or live.ndim != 1 or live.shape != shadow.shape:
        raise ValueError("guard_ref.commit: two one-dimensional uint8 arrays of equal size")
    if live.size % COMMIT_UNIT:
        raise ValueError("guard_ref.commit: the size must be a multiple of 16 bytes")
    keep = shadow if int(verdict) != 0 else live
    return keep.copy(), keep.copy()


def run_steps(steps, state, live, shadow, hyper=None, guard=None, max_norm=0.0, scale=1.0):
    """A sequence of guarded steps that carries a buffer slab: `steps` = [(grad, launch_status, forward_bytes)], where
    `forward_bytes` is what the step's forward leaves in the live slab before the verdict is known.  `state` = (param,
    exp_avg, exp_avg_sq), updated in place.  Returns (live, shadow, verdicts)."""
    hyper = new_hyper() if hyper is None else hyper
    guard = np.zeros(8, dtype=np.int32) if guard is None else guard
    verdicts = []
    for grad, status, forward_bytes in steps:
        live = np.asarray(forward_bytes, dtype=np.uint8).copy()
        verdicts.append(step_guard(grad, max_norm, scale, status, hyper, guard))
        adam_step_guarded(state[0], grad, state[1], state[2], hyper, guard)
        live, shadow = commit(guard[0], live, shadow)
    return live, shadow, verdicts


def describe(words):
    """The eight words as a dict keyed by `WORDS`."""
    return {k: int(w) for k, w in zip(WORDS, words)}
