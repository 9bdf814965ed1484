"""numpy restatement of `mpa_repulsion_cd_forward` / `mpa_repulsion_cd_backward` (include/mpa_hip.h): the repulsion loss
of the reference (multi_part_assembly/utils/loss.py:205-225) over the unordered pairs of valid parts, operation by
operation, in float32 (the order the kernel follows, bit for bit) or in float64 (the anchor of the tests).  It is the
specification csrc/repulsion.hip is held to, and what `loss.repulsion_cd_loss(fused=True)` is compared with.  Imports
nothing but numpy.

    loss_b = [nv thre + 2 sum_{i<j, both valid} max(0, thre - cd_ij)] / nv^2        nv = number of valid parts
    cd_ij  = mean_n d1[n] + mean_m d2[m],  d1[n] = min_m d(a_n, b_m),  d2[m] = min_n d(a_n, b_m)
    d      = (dx*dx + dy*dy) + dz*dz, every operation rounded; the lowest index wins a tie; a point that never sees
             d < 1e32 keeps (1e32, -1)                                               (the Chamfer contract)

The diagonal of the reference's P x P sum is `thre` per valid part (cd_ii = 0) and every unordered pair appears twice.
"""
from __future__ import annotations

import numpy as np

MAX_POINTS = 2048  # the kernel's envelope (csrc/repulsion.hip)
MAX_PARTS = 64
LANES = 256        # partial sums of `ordered_sum`
FAR = 1e32

NOT_SEARCHED, SEARCHED, HINGED = 0, 1, 2  # the flag of a pair slot


def pair_slots(P):
    """The unordered pairs (i, j), i < j, in slot order: i ascending, then j ascending.  P (P - 1) / 2 of them."""
    return [(i, j) for i in range(P) for j in range(i + 1, P)]


def pair_distances(a, b):
    """d [Na, Nb] between two clouds in their dtype: (dx*dx + dy*dy) + dz*dz, each operation rounded."""
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def nearest(d, axis):
    """(min, arg-min) along `axis` under the Chamfer contract: the first index attaining the minimum; (1e32, -1) where no
    distance is below 1e32."""
    idx = np.argmin(d, axis=axis)
    best = np.take_along_axis(d, np.expand_dims(idx, axis), axis).squeeze(axis)
    seen = best < d.dtype.type(FAR)
    return np.where(seen, best, d.dtype.type(FAR)), np.where(seen, idx, -1).astype(np.int32)


def pair_search(a, b):
    """(d1 [Na], idx1 [Na], d2 [Nb], idx2 [Nb]) of one pair: what `chamfer_distance(a[None], b[None])` returns."""
    d = pair_distances(a, b)
    d1, i1 = nearest(d, 1)
    d2, i2 = nearest(d, 0)
    return d1, i1, d2, i2


def ordered_sum(v):
    """Sum of a vector in the kernel's order: LANES partial sums p[t] = ((v[t] + v[t + 256]) + v[t + 512]) + ... started
    at 0; in each group of 64 partials six butterfly steps p[t] += p[t ^ off], off = 32, 16, 8, 4, 2, 1; the four group
    sums added left to right."""
    v = np.asarray(v)
    p = np.zeros(LANES, dtype=v.dtype)
    for k0 in range(0, len(v), LANES):
        chunk = v[k0:k0 + LANES]
        p[:len(chunk)] = p[:len(chunk)] + chunk
    p = p.reshape(LANES // 64, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        p = p + p[:, lane ^ off]
    s = p[0, 0]
    for w in range(1, LANES // 64):
        s = s + p[w, 0]
    return s


def mean(v):
    v = np.asarray(v)
    return ordered_sum(v) / v.dtype.type(len(v))


def box_gap(a, b):
    """The squared gap between the bounding boxes of two clouds, in their dtype with the rounded formula of
    csrc/contact_points.hip: per axis max(lo_b - hi_a, lo_a - hi_b, 0), then (gx*gx + gy*gy) + gz*gz.  Subtraction,
    multiplication of non-negative values and addition are monotone under rounding, so it is a lower bound of every
    COMPUTED d of the pair."""
    zero = a.dtype.type(0)
    g = [max(b[:, k].min() - a[:, k].max(), a[:, k].min() - b[:, k].max(), zero) for k in range(3)]
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]


def pruned(a, b, thre):
    """The prune of the kernel: the pair is not searched when box_gap >= thre.  Every d >= g, so both means are at least
    g (1 - N 2^-24) and cd >= 2 g (1 - N 2^-24) >= g >= thre for N <= 2048: the hinge of a pruned pair is exactly zero."""
    return bool(box_gap(a, b) >= a.dtype.type(thre))


def repulsion_cd(part_pcs, valids, thre, dtype=np.float32, prune=True, details=False):
    """loss [B], cd [B, P, P], flag [B, P (P - 1) / 2] uint8 of `mpa_repulsion_cd_forward` in `dtype`.

    part_pcs [B, P, N, 3] posed clouds (cast to `dtype`); valids [B, P] (a part is valid iff == 1; padded slots are never
    read); `thre` is rounded to `dtype`.  flag: NOT_SEARCHED (a padded member, or pruned), SEARCHED (cd known, hinge
    below zero), HINGED (thre - cd >= 0: the pair carries gradient, the rule of torch's clamp_min).  cd is symmetric,
    0 on the diagonal and 0 wherever the pair was not searched; with prune=False every valid pair is searched.  A sample
    without a valid part has loss NaN (0 / 0, as the reference).  `details`: also {(b, i, j): (d1, idx1, d2, idx2)}."""
    pcs = np.asarray(part_pcs, dtype=dtype)
    valids = np.asarray(valids)
    if pcs.ndim != 4 or pcs.shape[3] != 3 or valids.shape != pcs.shape[:2]:
        raise ValueError(f"repulsion_cd: part_pcs {pcs.shape} must be [B, P, N, 3] and valids {valids.shape} [B, P]")
    B, P, N, _ = pcs.shape
    T = pcs.dtype.type
    thre = T(thre)
    slots = pair_slots(P)
    loss = np.zeros(B, dtype=dtype)
    cd = np.zeros((B, P, P), dtype=dtype)
    flag = np.zeros((B, len(slots)), dtype=np.uint8)
    found = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(B):
            s = T(0)
            for k, (i, j) in enumerate(slots):
                if valids[b, i] != 1 or valids[b, j] != 1:
                    continue
                if prune and pruned(pcs[b, i], pcs[b, j], thre):
                    continue
                d1, i1, d2, i2 = pair_search(pcs[b, i], pcs[b, j])
                c = mean(d1) + mean(d2)
                h = thre - c
                cd[b, i, j] = cd[b, j, i] = c
                flag[b, k] = HINGED if h >= 0 else SEARCHED
                s = s + (h if h > 0 else T(0))
                if details:
                    found[(b, i, j)] = (d1, i1, d2, i2)
            nv = T((valids[b] == 1).sum())
            loss[b] = (nv * thre + T(2) * s) / (nv * nv)
    return (loss, cd, flag, found) if details else (loss, cd, flag)


def repulsion_cd_grad(part_pcs, valids, thre, grad_loss, dtype=np.float32, prune=True):
    """d (sum_b grad_loss[b] loss_b) / d part_pcs [B, P, N, 3] as `mpa_repulsion_cd_backward` forms it, in `dtype`.

    c_b = (-grad_loss[b] * 2) / ((nv * nv) * N).  Point n of part i takes, over its HINGED partners j in ascending order,
    first c_b * (2 (a_n - b_{idx_ij[n]})) for its own minimum and then c_b * (2 (a_n - b_m)) for every point m of j whose
    minimum lands on it, in ascending m; every product and sum rounded, per coordinate.  An index of -1 contributes
    nothing.  Padded slots, samples without a valid part and points without a HINGED partner get exactly zero."""
    pcs = np.asarray(part_pcs, dtype=dtype)
    valids = np.asarray(valids)
    B, P, N, _ = pcs.shape
    T = pcs.dtype.type
    gl = np.asarray(grad_loss, dtype=dtype)
    _, _, flag, found = repulsion_cd(pcs, valids, thre, dtype=dtype, prune=prune, details=True)
    slot_of = {ij: k for k, ij in enumerate(pair_slots(P))}
    grad = np.zeros_like(pcs)
    for b in range(B):
        nv = T((valids[b] == 1).sum())
        if nv == 0:
            continue
        c = (-gl[b] * T(2)) / ((nv * nv) * T(N))
        for i in range(P):
            if valids[b, i] != 1:
                continue
            acc = np.zeros((N, 3), dtype=dtype)
            for j in range(P):
                if j == i:
                    continue
                lo, hi = min(i, j), max(i, j)
                if flag[b, slot_of[(lo, hi)]] != HINGED:
                    continue
                d1, i1, d2, i2 = found[(b, lo, hi)]
                own, landing = (i1, i2) if i < j else (i2, i1)
                a, o = pcs[b, i], pcs[b, j]
                hit = own >= 0
                acc[hit] = acc[hit] + c * (T(2) * (a[hit] - o[own[hit]]))
                for m in range(N):  # ascending m
                    n = landing[m]
                    if n >= 0:
                        acc[n] = acc[n] + c * (T(2) * (a[n] - o[m]))
            grad[b, i] = acc
    return grad


def brute_force(part_pcs, valids, thre):
    """The reference's formulation in float64 with library reductions: all P x P pairs, the diagonal included, masked and
    divided by the number of valid pairs.  An independent check of the restatement's algebra."""
    pcs = np.asarray(part_pcs, dtype=np.float64)
    v = (np.asarray(valids) == 1).astype(np.float64)
    B, P, N, _ = pcs.shape
    out = np.zeros(B)
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(B):
            tot = 0.0
            for i in range(P):
                for j in range(P):
                    if v[b, i] and v[b, j]:
                        d = ((pcs[b, i][:, None, :] - pcs[b, j][None, :, :]) ** 2).sum(-1)
                        tot += max(thre - (d.min(1).mean() + d.min(0).mean()), 0.0)
            out[b] = tot / (v[b].sum() ** 2)
    return out
