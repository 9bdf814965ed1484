"""csrc/pointnet2_ops.hip against the numpy restatement (multi_part_assembly_amd/pointnet2_ref.py), index for index and bit
for bit: furthest point sampling across the sizes at which the kernel changes its layout (1, 2, 4, 8 points per thread,
the streaming kernel above 4096) and on clouds full of ties; the ball query across staged and unstaged clouds with points
exactly on the boundary; grouping forward and backward with empty, single and very long contribution lists and indices
out of range; sentinels, run-to-run identity, graph capture, and the shipped shape once."""
import numpy as np
import pytest
import torch

from multi_part_assembly_amd import _lib, pointnet2_ref as ref, pointnet2_utils as pu

pytestmark = pytest.mark.gpu
f32 = np.float32


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def clouds(kind, M, N, seed):
    rng = np.random.RandomState(seed)
    if kind == "random":
        return rng.rand(M, N, 3).astype(f32) + f32(0.1)
    if kind == "lattice":                                   # 27 sites: every round is decided by the tie rule
        return (rng.randint(1, 4, size=(M, N, 3)) * f32(0.25)).astype(f32)
    if kind == "duplicated":
        x = rng.rand(M, N, 3).astype(f32) + f32(0.1)
        x[:, N // 2:] = x[:, :N - N // 2]
        return x
    if kind == "zero_padded":                               # B-Global's padding: rows of zeros, also in front
        x = rng.rand(M, N, 3).astype(f32) - f32(0.5)
        x[:, rng.rand(N) < 0.4] = 0
        x[0, 0] = 0
        return x
    if kind == "all_skipped":
        return (rng.rand(M, N, 3).astype(f32) * f32(0.01)).astype(f32)   # |p|^2 <= 3e-4 everywhere
    raise ValueError(kind)


KINDS = ("random", "lattice", "duplicated", "zero_padded", "all_skipped")


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 511, 512, 513, 1000, 4096, 4097, 20000])
def test_fps_equals_the_restatement(cuda_device, N):
    npoints = [1, min(N, 512)] + ([N + 3] if N <= 65 else [])
    for s, kind in enumerate(KINDS):
        x = clouds(kind, 3, N, 100 + s)
        d = dev(x, cuda_device)
        for npoint in npoints:
            got = pu.furthest_point_sample(d, npoint)
            assert got.dtype == torch.int32 and got.shape == (3, npoint)
            want = ref.furthest_point_sample(x, npoint)
            assert np.array_equal(got.cpu().numpy(), want), (kind, N, npoint)
        if kind == "all_skipped":
            assert not want.any()


def test_fps_nonfinite_coordinates_stay_in_range(cuda_device):
    x = clouds("random", 2, 300, 7)
    x[0, 5], x[1, 17, 1], x[1, 40] = np.nan, np.inf, -np.inf
    got = pu.furthest_point_sample(dev(x, cuda_device), 64).cpu().numpy()
    assert got.min() >= 0 and got.max() < 300


def ball_case(N, S, seed):
    """A cloud with points exactly on and just inside the boundary of the ball around the origin (radius 0.2), centres that
    are points of the cloud, the origin, and one far away (an empty ball)."""
    rng = np.random.RandomState(seed)
    x = rng.rand(3, N, 3).astype(f32) - f32(0.5)
    r = f32(0.2)
    if N >= 4:
        x[:, 1] = (r, 0, 0)                                  # squared distance r * r: excluded
        x[:, 2] = (0, np.nextafter(r, f32(0), dtype=f32), 0)  # just inside
        x[:, 3] = (0, 0, -r)
    c = x[:, rng.randint(0, N, size=S)].copy()
    c[:, 0] = 0
    if S > 1:
        c[:, S - 1] = 9
    return x, c


@pytest.mark.parametrize("N", [1, 65, 1000, 4097])
def test_ball_query_equals_the_restatement(cuda_device, N):
    seen = set()
    for S in (1, 128, 512):
        x, c = ball_case(N, S, N + S)
        dx, dc = dev(x, cuda_device), dev(c, cuda_device)
        d = ((c[:, :, None, :] - x[:, None, :, :]) ** 2)
        d = (d[..., 0] + d[..., 1]) + d[..., 2]
        for nsample in (1, 16, 64, 128):
            for radius in (0.02, 0.2, 3.0):                   # empty / partial / overfull balls
                got = pu.ball_query(radius, nsample, dx, dc).cpu().numpy()
                want = ref.ball_query(radius, nsample, x, c)
                assert got.dtype == np.int32 and np.array_equal(got, want), (N, S, nsample, radius)
                cnt = (d < f32(radius) * f32(radius)).sum(axis=2)
                seen |= {"empty"} if (cnt == 0).any() else set()
                seen |= {"partial"} if ((cnt > 0) & (cnt < nsample)).any() else set()
                seen |= {"overfull"} if (cnt > nsample).any() else set()
    assert seen == ({"empty", "partial", "overfull"} if N > 1 else {"empty", "partial"})


def group_case(M, C, N, S, K, seed):
    rng = np.random.RandomState(seed)
    feat = rng.randn(M, C, N).astype(f32)
    idx = rng.randint(0, N, size=(M, S, K)).astype(np.int32)
    if N > 2:
        idx[idx == N - 1] = 0                                # point N - 1: an empty list
        idx[idx == N - 2] = 1
        idx[0, S - 1, K - 1] = N - 2                         # point N - 2 of cloud 0: a list of one
    if M > 1:
        idx[1] = min(4, N - 1)                               # one index repeated S K times
    g = (rng.randn(M, C, S, K) * 10.0 ** rng.randint(-2, 3, size=(M, 1, S, K))).astype(f32)
    return feat, idx, g


GROUP_SHAPES = [(1, 5, 1), (65, 7, 3), (1000, 128, 16), (1000, 130, 64), (9000, 33, 5)]   # (N, S, K); 9000: rows not staged


@pytest.mark.parametrize("C", [1, 3, 67, 128])
def test_grouping_forward_and_backward_are_bit_equal(cuda_device, C):
    for s, (N, S, K) in enumerate(GROUP_SHAPES):
        feat, idx, g = group_case(3, C, N, S, K, 10 * C + s)
        dfeat = dev(feat, cuda_device).requires_grad_()
        out = pu.grouping_operation(dfeat, dev(idx, cuda_device))
        assert np.array_equal(out.detach().cpu().numpy().view(np.uint32), ref.grouping_operation(feat, idx).view(np.uint32))
        out.backward(dev(g, cuda_device))
        want = ref.grouping_backward(g, idx, N)
        assert np.array_equal(dfeat.grad.cpu().numpy().view(np.uint32), want.view(np.uint32)), (C, N, S, K)
        if N > 2:
            assert S * K <= 1000 or (idx[1] == idx[1, 0, 0]).all()       # a list longer than 1000
            assert not (idx == N - 1).any() and (idx[0] == N - 2).sum() == 1
        # gather_operation: the same kernels with K = 1
        dfeat.grad = None
        out = pu.gather_operation(dfeat, dev(idx[:, :, 0], cuda_device))
        assert np.array_equal(out.detach().cpu().numpy(), ref.gather_operation(feat, idx[:, :, 0]))
        out.backward(dev(g[..., 0], cuda_device))
        assert np.array_equal(dfeat.grad.cpu().numpy().view(np.uint32),
                              ref.gather_backward(g[..., 0], idx[:, :, 0], N).view(np.uint32))


def padded(n, dtype, device, fill):
    """A buffer of n elements with 64 guard elements behind it, all `fill`."""
    buf = torch.full((n + 64,), fill, dtype=dtype, device=device)
    return buf, buf[:n]


def test_out_of_range_indices_are_neither_read_nor_written_through(cuda_device):
    M, C, N, S, K = 2, 5, 40, 9, 7
    feat, idx, g = group_case(M, C, N, S, K, 3)
    idx[0, 1, 1], idx[0, 2, 2], idx[1, 3, 3], idx[1, 4, 4] = -1, N, 2 ** 31 - 1, -2 ** 31
    idx[1, 5, 5] = N + 100000
    fbuf, fview = padded(M * C * N, torch.float32, cuda_device, float("nan"))     # NaN around the features: never read
    fview.copy_(dev(feat, cuda_device).reshape(-1))
    didx, dg = dev(idx, cuda_device), dev(g, cuda_device)
    obuf, oview = padded(M * C * S * K, torch.float32, cuda_device, float("nan"))
    _lib.launch("mpa_group_points_forward", cuda_device, fview, didx, M, C, N, S, K, oview)
    out = oview.cpu().numpy().reshape(M, C, S, K)
    assert np.array_equal(out.view(np.uint32), ref.grouping_operation(feat, idx).view(np.uint32))
    assert (out[0, :, 1, 1] == 0).all() and (out[1, :, 5, 5] == 0).all()
    assert torch.isnan(obuf[M * C * S * K:]).all()
    ws = torch.empty(_lib.query("mpa_group_points_workspace", M, N, S, K), dtype=torch.uint8, device=cuda_device)
    gbuf, gview = padded(M * C * N, torch.float32, cuda_device, float("nan"))
    _lib.launch("mpa_group_points_backward", cuda_device, dg, didx, M, C, N, S, K, ws, gview)
    got = gview.cpu().numpy().reshape(M, C, N)
    assert np.array_equal(got.view(np.uint32), ref.grouping_backward(g, idx, N).view(np.uint32))
    assert torch.isnan(gbuf[M * C * N:]).all()


def test_sentinel_filled_outputs_are_fully_overwritten_and_runs_are_identical(cuda_device):
    x = clouds("zero_padded", 3, 700, 1)
    dx = dev(x, cuda_device)
    runs = []
    for _ in range(2):
        ibuf, iview = padded(3 * 40, torch.int32, cuda_device, -12345)
        _lib.launch("mpa_furthest_point_sample", cuda_device, dx, 3, 700, 40, None, iview)
        assert (iview >= 0).all() and (ibuf[120:] == -12345).all()
        centres = pu.gather_operation(dx.transpose(1, 2).contiguous(), iview.view(3, 40)).transpose(1, 2).contiguous()
        bbuf, bview = padded(3 * 40 * 16, torch.int32, cuda_device, -12345)
        centres[:, 39] = 9                                       # an empty ball is written too (zeros)
        _lib.launch("mpa_ball_query", cuda_device, dx, centres, 0.15, 3, 700, 40, 16, bview)
        assert (bview >= 0).all() and (bview.view(3, 40, 16)[:, 39] == 0).all() and (bbuf[3 * 40 * 16:] == -12345).all()
        g = torch.ones(3, 3, 40, 16, device=cuda_device)
        feat = dx.transpose(1, 2).contiguous().requires_grad_()
        out = pu.grouping_operation(feat, bview.view(3, 40, 16))
        out.backward(g)
        runs.append((iview.clone(), bview.clone(), out.detach().clone(), feat.grad.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert np.array_equal(runs[0][0].view(3, 40).cpu().numpy(), ref.furthest_point_sample(x, 40))


def test_every_operator_is_captured_in_a_graph_and_replayed(cuda_device):
    N, S, K, C = 600, 64, 16, 5
    x1, x2 = clouds("random", 2, N, 1), clouds("duplicated", 2, N, 2)
    feat, _, g = group_case(2, C, N, S, K, 5)
    static_x = dev(x1, cuda_device)
    dfeat, dg = dev(feat, cuda_device), dev(g, cuda_device)
    res = {}

    def call():
        res["idx"] = pu.furthest_point_sample(static_x, S)
        res["centres"] = pu.gather_operation(static_x.transpose(1, 2).contiguous(), res["idx"])
        res["ball"] = pu.ball_query(0.25, K, static_x, res["centres"].transpose(1, 2).contiguous())
        res["grouped"] = pu.grouping_operation(dfeat, res["ball"])
        res["grad"] = pu._group_backward(dg, res["ball"], N)

    side = torch.cuda.Stream(device=cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream(cuda_device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    static_x.copy_(dev(x2, cuda_device))
    for v in res.values():
        v.fill_(-3)
    graph.replay()
    torch.cuda.synchronize()
    idx = ref.furthest_point_sample(x2, S)
    assert np.array_equal(res["idx"].cpu().numpy(), idx)
    centres = ref.gather_operation(x2.transpose(0, 2, 1), idx)
    assert np.array_equal(res["centres"].cpu().numpy(), centres)
    ball = ref.ball_query(0.25, K, x2, centres.transpose(0, 2, 1))
    assert np.array_equal(res["ball"].cpu().numpy(), ball)
    assert np.array_equal(res["grouped"].cpu().numpy(), ref.grouping_operation(feat, ball))
    assert np.array_equal(res["grad"].cpu().numpy().view(np.uint32), ref.grouping_backward(g, ball, N).view(np.uint32))


def test_shipped_shape_once(cuda_device):
    """M = 352, N = 1000 -> 512 centres, 64 samples, C = 128: the indices in full; the copy and the backward sums on
    eight (cloud, channel) rows of the 1.4e9-element tensors (the kernels compute all of them)."""
    M, N, S, K, C = 352, 1000, 512, 64, 128
    rng = np.random.RandomState(0)
    x = rng.rand(M, N, 3).astype(f32) - f32(0.5)
    x[5, 700:] = 0
    dx = dev(x, cuda_device)
    idx = pu.furthest_point_sample(dx, S)
    want_idx = ref.furthest_point_sample(x, S)
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    centres = pu.gather_operation(dx.transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()
    want_centres = np.take_along_axis(x, want_idx[:, :, None].astype(np.int64), axis=1)
    assert np.array_equal(centres.cpu().numpy(), want_centres)
    ball = pu.ball_query(0.2, K, dx, centres)
    want_ball = ref.ball_query(0.2, K, x, want_centres)
    assert np.array_equal(ball.cpu().numpy(), want_ball)
    gen = torch.Generator(device=cuda_device).manual_seed(1)
    feat = torch.randn(M, C, N, device=cuda_device, generator=gen).requires_grad_()
    out = pu.grouping_operation(feat, ball)
    assert out.shape == (M, C, S, K)
    g = torch.randn(M, C, S, K, device=cuda_device, generator=gen)
    out.backward(g)
    rows = [(0, 0), (0, 127), (5, 3), (100, 64), (200, 1), (351, 0), (351, 127), (17, 99)]
    for m, c in rows:
        f_row, g_row = feat[m, c].detach().cpu().numpy(), g[m, c].cpu().numpy()
        assert np.array_equal(out[m, c].detach().cpu().numpy(), ref.grouping_operation(f_row[None, None], want_ball[m:m + 1])[0, 0])
        want = ref.grouping_backward(g_row[None, None], want_ball[m:m + 1], N)[0, 0]
        assert np.array_equal(feat.grad[m, c].cpu().numpy().view(np.uint32), want.view(np.uint32)), (m, c)
