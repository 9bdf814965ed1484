"""numpy restatement of the PointNet++ sampling, grouping and interpolation operators (include/mpa_hip.h,
csrc/pointnet2_ops.hip, csrc/pointnet2_interp.hip): what the reference's CUDA-only `pointnet2_ops` extension computes (its
`_ext-src/src/sampling_gpu.cu`, `ball_query_gpu.cu`, `group_points_gpu.cu`, `interpolate_gpu.cu`), written as definitions
instead of as thread programs.  Every operation is one IEEE float32
operation in the written order, with no contraction.  It is the specification the device kernels are held to, and what
`pointnet2_utils` runs for host tensors.  Imports nothing but numpy.

`sa_mlp_max` / `sa_scale_shift` at the end restate the evaluation kernel of a whole set-abstraction level
(csrc/pointnet2_sa_mlp.hip) the same way, in the dtype of their inputs: the float64 evaluation is the anchor of its tests.

Furthest point sampling needs one remark.  The reference reduces (distance, index) pairs over a block of T threads with a
tree whose `max` keeps the LOWER thread on equal distances, strides T/2 ... 1.  The winner among equal distances is
therefore the thread whose index, read with its log2 T bits REVERSED, is smallest (the last level decides bit 0, the level
before it bit 1, ...); inside one thread (points k = r, r + T, ...) the strict `>` keeps the smallest k.  `fps_key` is
that order as one integer; the restatement and the kernel take the maximum of (distance, -key), whatever block they use.
"""
from __future__ import annotations

import math

import numpy as np

_f32 = np.float32
FPS_START = _f32(1e10)       # the running distance of every point before the first round
FPS_SKIP_BELOW = 1e-3        # a point with |p|^2 <= this (the float32 sum widened to double) is never looked at
MAX_THREADS = 512


def fps_threads(n: int) -> int:
    """The reference's block size for a cloud of n points: max(min(1 << int(log(n) / log(2)), 512), 1) in double
    precision (include/cuda_utils.h's `opt_n_threads`)."""
    pow_2 = int(math.log(float(n)) / math.log(2.0))
    return max(min(1 << pow_2, MAX_THREADS), 1)


def fps_threads_closed_form(n: int) -> int:
    """min(512, 2^floor(log2 n)) in integers: what the kernel computes.  Equal to `fps_threads` for n = 1 ... 4096
    (tests/test_pointnet2_ops.py keeps the table)."""
    return min(MAX_THREADS, 1 << (int(n).bit_length() - 1))


def bit_reverse(r, bits: int):
    r = np.asarray(r, dtype=np.int64)
    out = np.zeros_like(r)
    for b in range(bits):
        out |= ((r >> b) & 1) << (bits - 1 - b)
    return out


def fps_key(n: int, threads: int | None = None):
    """int64 [n]: the tie order of the reference's reduction — on equal distances the point with the smallest key wins.
    High part: the bit-reversed reference thread k mod T; low part: k div T (the order inside one thread)."""
    T = fps_threads_closed_form(n) if threads is None else threads
    bits = T.bit_length() - 1
    k = np.arange(n, dtype=np.int64)
    return (bit_reverse(k % T, bits) << 22) | (k // T)


def furthest_point_sample(xyz, npoint: int, threads: int | None = None):
    """xyz [M, N, 3] float32 -> int32 [M, npoint].  `threads` overrides the reference's block size T(N) (tests).
    Every cloud at once; the points are visited in winning order (ascending key), so that the first maximum along that
    axis is the winner."""
    xyz = np.asarray(xyz, dtype=_f32)
    M, N, _ = xyz.shape
    out = np.zeros((M, max(npoint, 0)), dtype=np.int32)
    if M == 0 or N == 0 or npoint <= 1:
        return out
    order = np.argsort(fps_key(N, threads), kind="stable")
    first = int(np.flatnonzero(order == 0)[0])      # where point 0 sits in that order
    x, y, z = (np.ascontiguousarray(xyz[:, order, a]) for a in range(3))
    mag = (x * x + y * y) + z * z
    live = ~(mag.astype(np.float64) <= FPS_SKIP_BELOW)
    some = live.any(axis=1)
    temp = np.full((M, N), FPS_START, dtype=_f32)
    rows = np.arange(M)
    pos = np.full(M, first)
    for j in range(1, npoint):
        dx, dy, dz = x - x[rows, pos, None], y - y[rows, pos, None], z - z[rows, pos, None]
        d = (dx * dx + dy * dy) + dz * dz
        d2 = np.minimum(d, temp)                    # (non-finite coordinates are outside the specification)
        temp = np.where(live, d2, temp)
        pos = np.where(some, np.argmax(np.where(live, d2, _f32(-1.0)), axis=1), first)
        out[:, j] = order[pos]
    return out


def ball_query(radius: float, nsample: int, xyz, new_xyz):
    """xyz [M, N, 3], new_xyz [M, S, 3] -> int32 [M, S, nsample]: the first nsample indices k, ascending, with
    (cx-x)^2 + (cy-y)^2 + (cz-z)^2 < radius^2 (float32, strict); the remaining slots repeat the first hit; a ball without
    a hit is all zeros."""
    xyz, new_xyz = np.asarray(xyz, dtype=_f32), np.asarray(new_xyz, dtype=_f32)
    M, N, _ = xyz.shape
    S = new_xyz.shape[1]
    r2 = _f32(radius) * _f32(radius)
    out = np.zeros((M, S, nsample), dtype=np.int32)
    for m in range(M):
        c, p = new_xyz[m][:, None, :], xyz[m][None, :, :]
        dx, dy, dz = c[..., 0] - p[..., 0], c[..., 1] - p[..., 1], c[..., 2] - p[..., 2]
        hit = ((dx * dx + dy * dy) + dz * dz) < r2            # [S, N]
        if N == 0 or nsample == 0:
            continue
        out[m] = np.argmax(hit, axis=1)[:, None]              # the first hit everywhere (0 for an empty ball) ...
        rank = np.cumsum(hit, axis=1) - 1
        j, k = np.nonzero(hit & (rank < nsample))
        out[m, j, rank[j, k]] = k                             # ... then the first nsample hits in their slots
    return out


def grouping_operation(features, idx):
    """features [M, C, N], idx [M, S, K] -> [M, C, S, K], a copy; an index outside [0, N) reads as 0."""
    features, idx = np.asarray(features, dtype=_f32), np.asarray(idx)
    M, C, N = features.shape
    ok = (idx >= 0) & (idx < N)
    safe = np.where(ok, idx, 0).astype(np.int64)
    out = np.take_along_axis(features[:, :, None, :], safe.reshape(M, 1, 1, -1), axis=3).reshape(M, C, *idx.shape[1:])
    return np.where(ok[:, None], out, _f32(0)).astype(_f32)


def grouping_backward(grad_out, idx, N: int):
    """grad_out [M, C, S, K], idx [M, S, K] -> [M, C, N]: every element the float32 sum of its contributions, added one
    after the other in ascending flat position j K + l (`np.add.at` on float32 rows); indices outside [0, N) contribute
    nothing."""
    grad_out, idx = np.asarray(grad_out, dtype=_f32), np.asarray(idx)
    M, C = grad_out.shape[:2]
    out = np.zeros((M, C, N), dtype=_f32)
    for m in range(M):
        flat = idx[m].reshape(-1).astype(np.int64)
        ok = (flat >= 0) & (flat < N)
        g = grad_out[m].reshape(C, -1)
        for c in range(C):
            np.add.at(out[m, c], flat[ok], g[c, ok])
    return out


def gather_operation(features, idx):
    """features [M, C, N], idx [M, S] -> [M, C, S]: grouping with K = 1."""
    return grouping_operation(features, np.asarray(idx)[:, :, None])[..., 0]


def gather_backward(grad_out, idx, N: int):
    return grouping_backward(np.asarray(grad_out)[..., None], np.asarray(idx)[:, :, None], N)


def three_nn(unknown, known):
    """unknown [M, n, 3], known [M, m, 3] -> dist [M, n, 3], idx int32 [M, n, 3], in the dtype of `unknown` (float32 or
    float64).  Every unknown point walks the known points in ascending k with
    d = ((ux-x)(ux-x) + (uy-y)(uy-y)) + (uz-z)(uz-z); three running bests start at (+inf, index 0) and take d through the
    strict cascade `d < best1` / `else d < best2` / `else d < best3` (equal distances keep the lower index first, a NaN d
    is never inserted); dist is the square root of the bests.  With m < 3 the unused slots stay (inf, 0)."""
    unknown = np.asarray(unknown)
    dt = unknown.dtype.type
    known = np.asarray(known, dtype=dt)
    M, n, _ = unknown.shape
    m = known.shape[1]
    best = [np.full((M, n), np.inf, dtype=dt) for _ in range(3)]
    besti = [np.zeros((M, n), dtype=np.int32) for _ in range(3)]
    ux, uy, uz = unknown[..., 0], unknown[..., 1], unknown[..., 2]
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(m):
            x, y, z = known[:, k, 0, None], known[:, k, 1, None], known[:, k, 2, None]
            d = ((ux - x) * (ux - x) + (uy - y) * (uy - y)) + (uz - z) * (uz - z)
            first = d < best[0]
            second = ~first & (d < best[1])
            third = ~first & ~second & (d < best[2])
            down = first | second
            best[2], besti[2] = np.where(down, best[1], np.where(third, d, best[2])), \
                np.where(down, besti[1], np.where(third, np.int32(k), besti[2]))
            best[1], besti[1] = np.where(first, best[0], np.where(second, d, best[1])), \
                np.where(first, besti[0], np.where(second, np.int32(k), besti[1]))
            best[0], besti[0] = np.where(first, d, best[0]), np.where(first, np.int32(k), besti[0])
    return np.sqrt(np.stack(best, axis=-1)).astype(dt), np.stack(besti, axis=-1).astype(np.int32)


def three_interpolate(features, idx, weight):
    """features [M, C, m], idx [M, n, 3], weight [M, n, 3] -> [M, C, n] in the dtype of `features`:
    out[b,c,j] = (f1 w1 + f2 w2) + f3 w3 with fk = features[b,c,idx[b,j,k]]; an index outside [0, m) reads as 0."""
    features, idx = np.asarray(features), np.asarray(idx)
    dt = features.dtype.type
    weight = np.asarray(weight, dtype=dt)
    M, C, m = features.shape
    n = idx.shape[1]
    ok = (idx >= 0) & (idx < m)
    safe = np.where(ok, idx, 0).astype(np.int64)
    if m == 0:
        f = np.zeros((M, C, n, 3), dtype=dt)
    else:
        f = np.take_along_axis(features[:, :, None, :], safe.reshape(M, 1, 1, -1), axis=3).reshape(M, C, n, 3)
        f = np.where(ok[:, None], f, dt(0))
    w = weight[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        return ((f[..., 0] * w[..., 0] + f[..., 1] * w[..., 1]) + f[..., 2] * w[..., 2]).astype(dt)


def three_interpolate_backward(grad_out, idx, weight, m: int):
    """grad_out [M, C, n], idx [M, n, 3], weight [M, n, 3] -> [M, C, m] in the dtype of `grad_out`: every element the sum,
    started at 0, of grad_out[b,c,j] * weight[b,j,k] over the pairs with idx[b,j,k] == i, added one after the other in
    ascending flat position 3 j + k (`np.add.at`); indices outside [0, m) contribute nothing."""
    grad_out, idx = np.asarray(grad_out), np.asarray(idx)
    dt = grad_out.dtype.type
    weight = np.asarray(weight, dtype=dt)
    M, C, n = grad_out.shape
    out = np.zeros((M, C, m), dtype=dt)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(M):
            flat = idx[b].reshape(-1).astype(np.int64)
            ok = (flat >= 0) & (flat < m)
            terms = (np.repeat(grad_out[b], 3, axis=1) * weight[b].reshape(1, -1)).astype(dt)    # [C, 3 n]
            for c in range(C):
                np.add.at(out[b, c], flat[ok], terms[c, ok])
    return out


def sa_scale_shift(gamma, beta, running_mean, running_var, eps):
    """The per-channel affine map of a BatchNorm in eval() mode, as `mpa_sa_mlp_pack` stores it:
    scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale, in the dtype of `gamma`."""
    gamma = np.asarray(gamma)
    dt = gamma.dtype.type
    scale = gamma / np.sqrt(np.asarray(running_var, dtype=dt) + dt(eps))
    return scale, np.asarray(beta, dtype=dt) - np.asarray(running_mean, dtype=dt) * scale


def sa_mlp_max(xyz, new_xyz, features, idx, layers):
    """One set-abstraction level in evaluation (`mpa_sa_mlp_max_forward`), in the dtype of `xyz` (float32 or float64):
    xyz [M, N, 3], new_xyz [M, S, 3], features [M, N, C] point-major | None, idx [M, S, K]; new_xyz and idx both None: one
    group of every point (S = 1, K = N).  layers: three (W [Cout, Cin], scale [Cout], shift [Cout]).  -> [M, S, C3].
    Row (m, j, l) is [xyz[m, idx[m,j,l]] - new_xyz[m, j] ; features[m, idx[m,j,l]]]; an index outside [0, N) reads a zero
    point and zero features; a_l = relu(scale_l * (W_l a_{l-1}) + shift_l); the result is the max over l of a_3."""
    xyz = np.asarray(xyz)
    dt = xyz.dtype
    M, N, _ = xyz.shape
    if (new_xyz is None) != (idx is None):
        raise ValueError("sa_mlp_max: new_xyz and idx are given together, or both None")
    if idx is None:
        rows = xyz[:, None]                                                    # [M, 1, N, 3]
        if features is not None:
            rows = np.concatenate([rows, np.asarray(features, dtype=dt)[:, None]], axis=-1)
    else:
        idx = np.asarray(idx)
        ok = (idx >= 0) & (idx < N)
        safe = np.where(ok, idx, 0).astype(np.int64)
        m = np.arange(M)[:, None, None]
        rows = np.where(ok[..., None], xyz[m, safe], dt.type(0)) - np.asarray(new_xyz, dtype=dt)[:, :, None, :]
        if features is not None:
            f = np.where(ok[..., None], np.asarray(features, dtype=dt)[m, safe], dt.type(0))
            rows = np.concatenate([rows, f], axis=-1)
    a = rows.astype(dt)
    for W, scale, shift in layers:
        a = np.maximum(np.asarray(scale, dtype=dt) * (a @ np.asarray(W, dtype=dt).T) + np.asarray(shift, dtype=dt), dt.type(0))
    return a.max(axis=2).astype(dt)
