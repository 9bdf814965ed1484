"""CPU checks of the PointNet++ operators: the numpy restatement (multi_part_assembly_amd/pointnet2_ref.py) against
independent formulations of the definitions in include/mpa_hip.h, and the C boundary of csrc/pointnet2_ops.hip (symbols,
argument refusals, workspace queries) — nothing here launches a kernel."""
import ctypes
import math

import numpy as np
import pytest
import torch

from multi_part_assembly_amd import _build, _lib, pointnet2_ref as ref, pointnet2_utils as pu

f32 = np.float32


# ---- furthest point sampling -----------------------------------------------------------------------------------------
def tree_fps(pts, npoint, T):
    """A literal simulation of the reference's thread program: T threads stride over the points with a strict `>`, then the
    shared-memory tree (strides T/2 ... 1) whose update keeps the lower thread unless the upper one is strictly larger."""
    pts = np.asarray(pts, dtype=f32)
    n = len(pts)
    temp = np.full(n, 1e10, dtype=f32)
    idx = [0]
    old = 0
    for _ in range(1, npoint):
        dists, dists_i = np.full(T, -1, dtype=f32), np.zeros(T, dtype=np.int64)
        x1, y1, z1 = pts[old]
        for t in range(T):
            best, besti = f32(-1), 0
            for k in range(t, n, T):
                x2, y2, z2 = pts[k]
                mag = f32(f32(x2 * x2) + f32(y2 * y2)) + f32(z2 * z2)
                if float(mag) <= 1e-3:
                    continue
                d = f32(f32(f32((x2 - x1)) * f32((x2 - x1))) + f32(f32((y2 - y1)) * f32((y2 - y1)))) \
                    + f32(f32((z2 - z1)) * f32((z2 - z1)))
                d2 = min(d, temp[k])
                temp[k] = d2
                if d2 > best:
                    best, besti = d2, k
            dists[t], dists_i[t] = best, besti
        s = T // 2
        while s >= 1:
            for t in range(s):
                v1, v2 = dists[t], dists[t + s]
                i1, i2 = dists_i[t], dists_i[t + s]
                dists[t] = max(v1, v2)
                dists_i[t] = i2 if v2 > v1 else i1
            s //= 2
        old = int(dists_i[0])
        idx.append(old)
    return np.array(idx, dtype=np.int32)


def brute_fps(pts, npoint):
    """Distance of every point to the chosen SET, recomputed from scratch each round (tie-free clouds, no skipped point)."""
    pts = np.asarray(pts, dtype=f32)
    chosen = [0]
    for _ in range(1, npoint):
        c = pts[chosen]                                                  # [m, 3]
        dx, dy, dz = (pts[:, None, a] - c[None, :, a] for a in range(3))
        d = ((dx * dx + dy * dy) + dz * dz).min(axis=1)
        chosen.append(int(np.argmax(d)))
    return np.array(chosen, dtype=np.int32)


def lattice(n, seed):
    rng = np.random.RandomState(seed)
    return (rng.randint(1, 4, size=(n, 3)) * f32(0.25)).astype(f32)      # 27 sites: ties and duplicates everywhere


def test_fps_equals_the_set_distance_formulation_on_tie_free_clouds():
    rng = np.random.RandomState(0)
    for n, npoint in ((1, 1), (7, 7), (100, 40), (600, 64)):
        pts = (rng.rand(n, 3).astype(f32) + f32(0.5))                    # |p|^2 >= 0.75: nothing is skipped
        got = ref.furthest_point_sample(pts[None], npoint)[0]
        assert np.array_equal(got, brute_fps(pts, npoint))
        assert len(set(got.tolist())) == npoint


@pytest.mark.parametrize("T", [1, 2, 4, 64, 512])
def test_fps_ties_follow_the_reference_tree(T):
    for seed, n in enumerate((T, T + 1, 2 * T + 3, 3 * T + 5)):
        n = min(max(n, 2), 700)
        clouds = [lattice(n, seed)]
        dup = np.random.RandomState(seed).rand(n, 3).astype(f32) + f32(0.2)
        dup[n // 2:] = dup[:n - n // 2]                                  # every point twice
        clouds.append(dup)
        for pts in clouds:
            npoint = min(n, 12)
            want = tree_fps(pts, npoint, T)
            got = ref.furthest_point_sample(pts[None], npoint, threads=T)[0]
            assert np.array_equal(got, want), (T, n)


def test_fps_uses_the_reference_block_size_by_default():
    pts = lattice(100, 5)
    assert np.array_equal(ref.furthest_point_sample(pts[None], 10)[0], tree_fps(pts, 10, 64))


def test_block_size_table():
    for n in range(1, 4097):
        assert ref.fps_threads(n) == ref.fps_threads_closed_form(n) == min(512, 2 ** int(math.floor(math.log2(n)))), n
    assert ref.fps_threads(1) == 1 and ref.fps_threads(511) == 256 and ref.fps_threads(20000) == 512


def _with_square_sum(target, x=0.0):
    """(x, y) in float32 with float32(x * x + y * y) == target: y is walked next to sqrt(target - x^2).  Not every float32
    is the square of one (the squares next to 1e-3 are spaced like its last bit), so a fixed x absorbs most of the sum
    and y's squares are spaced much finer than the target's last bit."""
    x, target = f32(x), f32(target)
    y = f32(np.sqrt(np.float64(target) - np.float64(x) ** 2))
    for _ in range(4096):
        s = f32(f32(x * x) + f32(y * y))
        if s == target:
            return x, y
        y = np.nextafter(y, f32(np.inf) if s < target else f32(0), dtype=f32)
    raise AssertionError("no float32 pair")


def test_fps_skip_rule_on_both_sides_of_the_threshold():
    edge = f32(1e-3)                                   # 0.001000000047...: ABOVE the double 1e-3, so not skipped
    below = np.nextafter(edge, f32(0), dtype=f32)      # the largest float32 that is skipped
    assert float(edge) > 1e-3 and float(below) <= 1e-3
    xa, ya = _with_square_sum(edge, 0.03)
    xb, yb = _with_square_sum(below, 0.03)
    pts = np.array([[1, 1, 1], [xa, ya, 0], [xb, yb, 0], [0, 0, 0]], dtype=f32)
    mag = (pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1]) + pts[:, 2] * pts[:, 2]
    assert mag[1] == edge and mag[2] == below
    got = ref.furthest_point_sample(pts[None], 4)[0]
    assert got[0] == 0 and got[1] == 1                 # the point on the threshold's upper side is sampled
    assert 2 not in got[1:] and 3 not in got[1:]       # the one just below and the zero row never are
    assert np.array_equal(got, tree_fps(pts, 4, 4))


def test_fps_all_skipped_and_more_samples_than_points():
    zeros = np.zeros((2, 9, 3), dtype=f32)
    assert np.array_equal(ref.furthest_point_sample(zeros, 5), np.zeros((2, 5), dtype=np.int32))
    pts = np.random.RandomState(3).rand(5, 3).astype(f32) + f32(0.5)
    got = ref.furthest_point_sample(pts[None], 8)[0]
    assert np.array_equal(got, tree_fps(pts, 8, 4))
    assert sorted(got[:5].tolist()) == [0, 1, 2, 3, 4] and got.min() >= 0 and got.max() < 5


# ---- ball query ------------------------------------------------------------------------------------------------------
def test_ball_query_boundary_padding_and_empty_balls():
    r = f32(0.5)
    r2 = r * r
    # points on the x axis at squared distance exactly r2 (excluded: strict), just inside, well inside, outside
    inside = np.nextafter(r, f32(0), dtype=f32)
    xyz = np.array([[[2, 0, 0], [r, 0, 0], [inside, 0, 0], [0.1, 0, 0], [-r, 0, 0], [0.2, 0, 0], [3, 3, 3]]], dtype=f32)
    assert f32(r * r) == r2 and f32(inside * inside) < r2
    new_xyz = np.array([[[0, 0, 0], [10, 10, 10], [3, 3, 3]]], dtype=f32)
    got = ref.ball_query(float(r), 5, xyz, new_xyz)
    assert got.dtype == np.int32 and got.shape == (1, 3, 5)
    assert got[0, 0].tolist() == [2, 3, 5, 2, 2]       # ascending hits, then the first hit repeated
    assert got[0, 1].tolist() == [0, 0, 0, 0, 0]       # an empty ball: zeros
    assert got[0, 2].tolist() == [6, 6, 6, 6, 6]
    assert ref.ball_query(float(r), 2, xyz, new_xyz)[0, 0].tolist() == [2, 3]   # overfull: the first nsample only
    # the wrapper on host tensors runs the same restatement
    t = pu.ball_query(float(r), 5, torch.from_numpy(xyz), torch.from_numpy(new_xyz))
    assert t.dtype == torch.int32 and np.array_equal(t.numpy(), got)


def test_ball_query_radius_is_squared_in_float32():
    radius = 0.2
    r2 = f32(radius) * f32(radius)
    assert float(r2) != radius * radius
    d = np.sqrt(np.float64(r2))                        # a point whose float32 squared distance sits at r2
    x = f32(radius)                                    # x * x == r2 exactly: on the boundary, excluded
    assert f32(x * x) == r2
    xyz = np.array([[[x, 0, 0], [np.nextafter(x, f32(0), dtype=f32), 0, 0]]], dtype=f32)
    got = ref.ball_query(radius, 2, xyz, np.zeros((1, 1, 3), dtype=f32))
    assert got[0, 0].tolist() == [1, 1] and d > 0


# ---- grouping --------------------------------------------------------------------------------------------------------
def test_grouping_forward_is_a_copy_and_out_of_range_reads_zero():
    rng = np.random.RandomState(1)
    feat = rng.randn(2, 3, 7).astype(f32)
    idx = rng.randint(0, 7, size=(2, 4, 5)).astype(np.int32)
    idx[0, 0, 0], idx[1, 3, 4] = -1, 7
    out = ref.grouping_operation(feat, idx)
    for m in range(2):
        for j in range(4):
            for l in range(5):
                k = idx[m, j, l]
                want = feat[m, :, k] if 0 <= k < 7 else np.zeros(3, dtype=f32)
                assert np.array_equal(out[m, :, j, l], want)
    assert np.array_equal(ref.gather_operation(feat, idx[:, :, 0]), out[..., 0])


def test_grouping_backward_is_a_sequential_float32_sum_within_its_bound():
    """|fl(sum) - sum| <= (n - 1) u sum|terms| / (1 - (n - 1) u) for n terms added one after the other, u = 2^-24: below
    n u sum|terms| for every n here."""
    rng = np.random.RandomState(2)
    M, C, N, S, K = 2, 3, 11, 40, 16
    idx = rng.randint(0, N - 1, size=(M, S, K)).astype(np.int32)        # point N - 1: an empty list
    idx[0, :, :] = 4                                                      # one list of S K = 640 entries
    idx[1, 0, 0], idx[1, 0, 1] = -3, N                                    # skipped
    idx[1, 5, 5] = 9
    g = (rng.randn(M, C, S, K) * (10.0 ** rng.randint(-3, 4, size=(M, C, S, K)))).astype(f32)
    got = ref.grouping_backward(g, idx, N)
    assert got.dtype == f32 and got.shape == (M, C, N)
    flat, g64 = idx.reshape(M, -1), g.reshape(M, C, -1).astype(np.float64)
    for m in range(M):
        for k in range(N):
            sel = flat[m] == k
            n = int(sel.sum())
            exact = g64[m][:, sel].sum(axis=1)
            bound = n * 2.0 ** -24 * np.abs(g64[m][:, sel]).sum(axis=1)
            assert np.all(np.abs(got[m, :, k].astype(np.float64) - exact) <= bound), (m, k, n)
            seq = np.zeros(C, dtype=f32)                                  # the order itself, term by term
            for p in np.flatnonzero(sel):
                seq = seq + g[m].reshape(C, -1)[:, p]
            assert np.array_equal(got[m, :, k], seq)
    assert np.all(got[:, :, N - 1] == 0)
    assert np.array_equal(ref.gather_backward(g[..., 0], idx[..., 0], N),
                          ref.grouping_backward(g[..., :1], idx[..., :1], N))


def test_wrappers_differentiate_on_the_host_path():
    rng = np.random.RandomState(4)
    feat = torch.from_numpy(rng.randn(2, 3, 6).astype(f32)).requires_grad_()
    idx = torch.from_numpy(rng.randint(0, 6, size=(2, 4, 3)).astype(np.int32))
    out = pu.grouping_operation(feat, idx)
    w = torch.from_numpy(rng.randn(*out.shape).astype(f32))
    (out * w).sum().backward()
    assert np.array_equal(feat.grad.numpy(), ref.grouping_backward(w.numpy(), idx.numpy(), 6))
    feat.grad = None
    out = pu.gather_operation(feat, idx[:, :, 0])
    (out * w[..., 0]).sum().backward()
    assert np.array_equal(feat.grad.numpy(), ref.gather_backward(w[..., 0].numpy(), idx[:, :, 0].numpy(), 6))
    xyz = torch.from_numpy(rng.rand(2, 6, 3).astype(f32) + 0.5)
    centres = pu.furthest_point_sample(xyz.double(), 4)                  # cast to float32, as custom_fwd upstream
    assert centres.dtype == torch.int32 and not centres.requires_grad
    assert np.array_equal(centres.numpy(), ref.furthest_point_sample(xyz.numpy(), 4))
    grouped = pu.QueryAndGroup(0.4, 3)(xyz, xyz[:, :2].contiguous(), feat)
    assert grouped.shape == (2, 6, 2, 3)
    assert pu.GroupAll()(xyz, None, feat).shape == (2, 6, 1, 6)


# ---- the C boundary --------------------------------------------------------------------------------------------------
NAMES = ["mpa_furthest_point_sample_workspace", "mpa_furthest_point_sample", "mpa_ball_query", "mpa_group_points_forward",
         "mpa_group_points_workspace", "mpa_group_points_backward"]


@pytest.fixture(scope="module")
def L():
    _build.build()
    return _lib.lib()


def test_symbols_are_declared_on_both_sides_and_the_version_stays(L):
    declared = _lib.declared_functions()
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name)
    assert L.mpa_abi_version() == 10 == _lib.ABI_VERSION


def test_arguments_are_refused_before_the_device_is_touched(L):
    z = ctypes.c_float(0.2)
    assert L.mpa_furthest_point_sample(None, -1, 4, 2, None, None, None) == -1 and b"negative" in L.mpa_last_error()
    assert L.mpa_furthest_point_sample(None, 2, 4, 2, None, None, None) == -1 and b"null" in L.mpa_last_error()
    assert L.mpa_furthest_point_sample(None, 2, 0, 2, None, None, None) == -1 and b"N=0" in L.mpa_last_error()
    assert L.mpa_furthest_point_sample(None, 1 << 20, 1 << 20, 2, None, None, None) == -1 and b"2^31" in L.mpa_last_error()
    assert L.mpa_furthest_point_sample(None, 0, 4, 2, None, None, None) == 0
    assert L.mpa_furthest_point_sample(None, 2, 4, 0, None, None, None) == 0
    assert L.mpa_ball_query(None, None, z, 2, 4, -1, 8, None, None) == -1 and b"negative" in L.mpa_last_error()
    assert L.mpa_ball_query(None, None, z, 2, 4, 3, 8, None, None) == -1 and b"null" in L.mpa_last_error()
    assert L.mpa_ball_query(None, None, z, 2, 4, 0, 8, None, None) == 0
    assert L.mpa_group_points_forward(None, None, 2, 3, -4, 5, 6, None, None) == -1 and b"negative" in L.mpa_last_error()
    assert L.mpa_group_points_forward(None, None, 2, 3, 4, 5, 6, None, None) == -1 and b"null" in L.mpa_last_error()
    assert L.mpa_group_points_forward(None, None, 1 << 12, 1 << 8, 4, 1 << 8, 1 << 8, None, None) == -1
    assert b"2^31" in L.mpa_last_error()
    assert L.mpa_group_points_forward(None, None, 2, 0, 4, 5, 6, None, None) == 0
    assert L.mpa_group_points_backward(None, None, 2, 3, 4, 5, -6, None, None, None) == -1
    assert b"negative" in L.mpa_last_error()
    assert L.mpa_group_points_backward(None, None, 2, 3, 4, 5, 6, None, None, None) == -1 and b"null" in L.mpa_last_error()
    assert L.mpa_group_points_backward(None, None, 0, 3, 4, 5, 6, None, None, None) == 0


def test_workspace_queries_are_pure_arithmetic(L):
    n = ctypes.c_int64(-1)
    assert L.mpa_furthest_point_sample_workspace(352, 1000, ctypes.byref(n)) == 0 and n.value == 0
    assert L.mpa_furthest_point_sample_workspace(32, 4096, ctypes.byref(n)) == 0 and n.value == 0
    assert L.mpa_furthest_point_sample_workspace(32, 20000, ctypes.byref(n)) == 0 and n.value == 32 * 20000 * 4
    assert L.mpa_furthest_point_sample_workspace(3, 4097, ctypes.byref(n)) == 0 and n.value == 49408   # 49164 -> x256
    assert L.mpa_furthest_point_sample_workspace(-1, 5, ctypes.byref(n)) == -1 and b"negative" in L.mpa_last_error()
    assert L.mpa_furthest_point_sample_workspace(3, 5, None) == -1 and b"null" in L.mpa_last_error()
    # per cloud: start and cursor of N + 1 words and the list of S K words, each rounded up to 64 words
    assert L.mpa_group_points_workspace(352, 1000, 512, 64, ctypes.byref(n)) == 0
    assert n.value == 4 * 352 * (1024 + 1024 + 32768)
    assert L.mpa_group_points_workspace(3, 63, 5, 1, ctypes.byref(n)) == 0 and n.value == 4 * 3 * 64 * 3
    assert L.mpa_group_points_workspace(3, 10, -5, 1, ctypes.byref(n)) == -1 and b"negative" in L.mpa_last_error()
    assert _lib.query("mpa_group_points_workspace", 2, 7, 3, 4) == 4 * 2 * 64 * 3
