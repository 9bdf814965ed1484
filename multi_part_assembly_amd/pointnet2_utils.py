"""The operator module of the reference's `pointnet2_ops` extension (pointnet2_ops/pointnet2_utils.py) over
csrc/pointnet2_ops.hip and csrc/pointnet2_interp.hip: the same function and class names and argument orders, so the
reference's `pointnet2_modules.py` binds to it unchanged — the set-abstraction modules and, through
`three_nn` / `three_interpolate`, its `PointnetFPModule`.

Inputs are cast to float32, as `custom_fwd(cast_inputs=torch.float32)` does upstream.  The wrappers check shapes, never
index values, and never synchronise.  CUDA tensors run the HIP kernels; CPU tensors run the numpy restatement
`pointnet2_ref` — slow, and the one exception to the package's "no CPU fallback" rule: it exists for the tests and for the
fixture generators (tests/golden/make_golden_pointnet2*.py), which drive the reference's own modules on the host.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib, pointnet2_ref

__all__ = ["furthest_point_sample", "gather_operation", "grouping_operation", "ball_query", "three_nn", "three_interpolate",
           "QueryAndGroup", "GroupAll", "FurthestPointSampling", "GatherOperation", "GroupingOperation", "BallQuery",
           "ThreeNN", "ThreeInterpolate"]


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def _i32(t):
    return t.detach().to(torch.int32).contiguous()


def _workspace(name, dev, *sizes):
    return torch.empty(max(1, _lib.query(name, *sizes)), dtype=torch.uint8, device=dev)


def _group_forward(features, idx):
    """features [M, C, N] float32, idx [M, S, K] int32, both contiguous -> [M, C, S, K]."""
    M, C, N = features.shape
    _, S, K = idx.shape
    if not features.is_cuda:
        return torch.from_numpy(pointnet2_ref.grouping_operation(features.numpy(), idx.numpy()))
    out = torch.empty((M, C, S, K), dtype=torch.float32, device=features.device)
    _lib.launch("mpa_group_points_forward", features.device, features, idx, M, C, N, S, K, out,
                timer=f"group_points_forward[{M}x{C}x{S}x{K}]")
    return out


def _group_backward(grad_out, idx, N):
    """grad_out [M, C, S, K] float32, idx [M, S, K] int32 -> [M, C, N], summed in ascending position."""
    M, C, S, K = grad_out.shape
    if not grad_out.is_cuda:
        return torch.from_numpy(pointnet2_ref.grouping_backward(grad_out.numpy(), idx.numpy(), N))
    dev = grad_out.device
    grad = torch.empty((M, C, N), dtype=torch.float32, device=dev)
    ws = _workspace("mpa_group_points_workspace", dev, M, N, S, K)
    _lib.launch("mpa_group_points_backward", dev, grad_out, idx, M, C, N, S, K, ws, grad,
                timer=f"group_points_backward[{M}x{C}x{S}x{K}]")
    return grad


def _check(name, t, dims, last=None):
    if t.dim() != dims or (last is not None and t.shape[-1] != last):
        raise ValueError(f"{name}: expected a {dims}-d tensor" + (f" ending in {last}" if last else "")
                         + f", got {tuple(t.shape)}")


class FurthestPointSampling(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, npoint):
        """xyz [M, N, 3], npoint -> int32 [M, npoint]: iterative furthest point sampling from point 0."""
        _check("furthest_point_sample", xyz, 3, 3)
        xyz = _f32(xyz)
        M, N, _ = xyz.shape
        npoint = int(npoint)
        if not xyz.is_cuda:
            out = torch.from_numpy(pointnet2_ref.furthest_point_sample(xyz.numpy(), npoint))
        else:
            out = torch.empty((M, npoint), dtype=torch.int32, device=xyz.device)
            ws = _workspace("mpa_furthest_point_sample_workspace", xyz.device, M, N)
            _lib.launch("mpa_furthest_point_sample", xyz.device, xyz, M, N, npoint, ws, out,
                        timer=f"furthest_point_sample[{M}x{N}->{npoint}]")
        ctx.mark_non_differentiable(out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return None, None


furthest_point_sample = FurthestPointSampling.apply


class GatherOperation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, idx):
        """features [M, C, N], idx [M, S] -> [M, C, S]."""
        _check("gather_operation", features, 3)
        _check("gather_operation", idx, 2)
        features, idx = _f32(features), _i32(idx)
        ctx.save_for_backward(idx)
        ctx.N = features.shape[2]
        return _group_forward(features, idx[:, :, None])[..., 0]

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        return _group_backward(_f32(grad_out)[..., None], idx[:, :, None], ctx.N), None


gather_operation = GatherOperation.apply


class ThreeNN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, unknown, known):
        """unknown [M, n, 3], known [M, m, 3] -> dist [M, n, 3] (l2 distances to the three nearest known points, nearest
        first), idx int32 [M, n, 3]; neither is differentiable."""
        _check("three_nn", unknown, 3, 3)
        _check("three_nn", known, 3, 3)
        unknown, known = _f32(unknown), _f32(known)
        M, n, _ = unknown.shape
        m = known.shape[1]
        if known.shape[0] != M:
            raise ValueError(f"three_nn: unknown {tuple(unknown.shape)} and known {tuple(known.shape)} differ in clouds")
        if not unknown.is_cuda:
            dist, idx = (torch.from_numpy(a) for a in pointnet2_ref.three_nn(unknown.numpy(), known.numpy()))
        else:
            dist = torch.empty((M, n, 3), dtype=torch.float32, device=unknown.device)
            idx = torch.empty((M, n, 3), dtype=torch.int32, device=unknown.device)
            _lib.launch("mpa_three_nn", unknown.device, unknown, known, M, n, m, dist, idx, timer=f"three_nn[{M}x{n}x{m}]")
        ctx.mark_non_differentiable(dist, idx)
        return dist, idx

    @staticmethod
    def backward(ctx, grad_dist, grad_idx):
        return None, None


three_nn = ThreeNN.apply


def _interpolate_forward(features, idx, weight):
    """features [M, C, m] float32, idx [M, n, 3] int32, weight [M, n, 3] float32, all contiguous -> [M, C, n]."""
    M, C, m = features.shape
    n = idx.shape[1]
    if not features.is_cuda:
        return torch.from_numpy(pointnet2_ref.three_interpolate(features.numpy(), idx.numpy(), weight.numpy()))
    out = torch.empty((M, C, n), dtype=torch.float32, device=features.device)
    _lib.launch("mpa_three_interpolate_forward", features.device, features, idx, weight, M, C, m, n, out,
                timer=f"three_interpolate_forward[{M}x{C}x{m}->{n}]")
    return out


def _interpolate_backward(grad_out, idx, weight, m):
    """grad_out [M, C, n] float32 -> [M, C, m], summed in ascending position 3 j + k."""
    M, C, n = grad_out.shape
    if not grad_out.is_cuda:
        return torch.from_numpy(pointnet2_ref.three_interpolate_backward(grad_out.numpy(), idx.numpy(), weight.numpy(), m))
    dev = grad_out.device
    grad = torch.empty((M, C, m), dtype=torch.float32, device=dev)
    ws = _workspace("mpa_three_interpolate_workspace", dev, M, n, m)
    _lib.launch("mpa_three_interpolate_backward", dev, grad_out, idx, weight, M, C, n, m, ws, grad,
                timer=f"three_interpolate_backward[{M}x{C}x{n}->{m}]")
    return grad


class ThreeInterpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, idx, weight):
        """features [M, C, m], idx [M, n, 3], weight [M, n, 3] -> [M, C, n]: the weighted sum of three feature columns;
        the gradient goes to `features` only."""
        _check("three_interpolate", features, 3)
        _check("three_interpolate", idx, 3, 3)
        _check("three_interpolate", weight, 3, 3)
        if idx.shape != weight.shape or idx.shape[0] != features.shape[0]:
            raise ValueError(f"three_interpolate: features {tuple(features.shape)}, idx {tuple(idx.shape)} and weight "
                             f"{tuple(weight.shape)} do not belong together")
        features, idx, weight = _f32(features), _i32(idx), _f32(weight)
        ctx.save_for_backward(idx, weight)
        ctx.m = features.shape[2]
        return _interpolate_forward(features, idx, weight)

    @staticmethod
    def backward(ctx, grad_out):
        idx, weight = ctx.saved_tensors
        return _interpolate_backward(_f32(grad_out), idx, weight, ctx.m), None, None


three_interpolate = ThreeInterpolate.apply


class GroupingOperation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, idx):
        """features [M, C, N], idx [M, S, K] -> [M, C, S, K]."""
        _check("grouping_operation", features, 3)
        _check("grouping_operation", idx, 3)
        features, idx = _f32(features), _i32(idx)
        ctx.save_for_backward(idx)
        ctx.N = features.shape[2]
        return _group_forward(features, idx)

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        return _group_backward(_f32(grad_out), idx, ctx.N), None


grouping_operation = GroupingOperation.apply


class BallQuery(torch.autograd.Function):
    @staticmethod
    def forward(ctx, radius, nsample, xyz, new_xyz):
        """radius, nsample, xyz [M, N, 3], new_xyz [M, S, 3] -> int32 [M, S, nsample]."""
        _check("ball_query", xyz, 3, 3)
        _check("ball_query", new_xyz, 3, 3)
        xyz, new_xyz = _f32(xyz), _f32(new_xyz)
        M, N, _ = xyz.shape
        S, nsample = new_xyz.shape[1], int(nsample)
        if new_xyz.shape[0] != M:
            raise ValueError(f"ball_query: xyz {tuple(xyz.shape)} and new_xyz {tuple(new_xyz.shape)} differ in clouds")
        if not xyz.is_cuda:
            out = torch.from_numpy(pointnet2_ref.ball_query(float(radius), nsample, xyz.numpy(), new_xyz.numpy()))
        else:
            out = torch.empty((M, S, nsample), dtype=torch.int32, device=xyz.device)
            _lib.launch("mpa_ball_query", xyz.device, xyz, new_xyz, float(radius), M, N, S, nsample, out,
                        timer=f"ball_query[{M}x{N}x{S}x{nsample}]")
        ctx.mark_non_differentiable(out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return None, None, None, None


ball_query = BallQuery.apply


class QueryAndGroup(nn.Module):
    """Ball query around the centres, then the grouped, centre-relative coordinates in front of the grouped features:
    xyz [M, N, 3], new_xyz [M, S, 3], features [M, C, N] | None -> [M, 3 + C, S, nsample]."""

    def __init__(self, radius, nsample, use_xyz=True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz, new_xyz, features=None):
        idx = ball_query(self.radius, self.nsample, xyz, new_xyz)
        grouped_xyz = grouping_operation(xyz.transpose(1, 2).contiguous(), idx)
        grouped_xyz = grouped_xyz - new_xyz.transpose(1, 2).unsqueeze(-1)
        if features is None:
            if not self.use_xyz:
                raise ValueError("QueryAndGroup: neither features nor use_xyz")
            return grouped_xyz
        grouped_features = grouping_operation(features, idx)
        return torch.cat([grouped_xyz, grouped_features], dim=1) if self.use_xyz else grouped_features


class GroupAll(nn.Module):
    """One group of every point: xyz [M, N, 3], features [M, C, N] | None -> [M, 3 + C, 1, N] (new_xyz is ignored)."""

    def __init__(self, use_xyz=True):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz, new_xyz, features=None):
        grouped_xyz = xyz.transpose(1, 2).unsqueeze(2)
        if features is None:
            return grouped_xyz
        grouped_features = features.unsqueeze(2)
        return torch.cat([grouped_xyz, grouped_features], dim=1) if self.use_xyz else grouped_features
