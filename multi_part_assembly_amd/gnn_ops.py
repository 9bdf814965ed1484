"""The small per-iteration pieces of the graph networks on the HIP library (csrc/gnn_glue.hip): the 7-wide first layer
of the pose encoder, the 512 -> 1 relation head with its sigmoid and valid-pair mask, the relation-weighted mean of the
edge features, the [part i ; part j] pair rows the edge MLP and the relation net read and the merging of equivalent
parts (reference models/dgl/modules.py:61-86, models/dgl/network.py:75-152).  The torch modules keep
holding the parameters (same state_dict keys); this only replaces what they compute."""
from __future__ import annotations

import torch

from . import _lib
from .gradsink import GradSink


def _f32c(t):
    return t.to(torch.float32).contiguous()


class _NarrowLinearReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        R, K = x.shape
        N = weight.shape[0]
        out = torch.empty((R, N), dtype=torch.float32, device=x.device)
        _lib.launch("mpa_narrow_linear_relu_forward", x.device, x, weight, bias, R, K, N, out,
                    timer=f"narrow_linear_relu_forward[{R}x{K}x{N}]")
        GradSink.register(ctx, (weight, bias))
        ctx.save_for_backward(x, weight, out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, weight, out = ctx.saved_tensors
        R, K = x.shape
        N = weight.shape[0]
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        grads = GradSink.outputs(ctx.params)
        grad_out = grad_out.contiguous()
        ws = torch.empty(_lib.query("mpa_narrow_linear_relu_workspace", R, K, N), dtype=torch.float32, device=x.device)
        _lib.launch("mpa_narrow_linear_relu_backward", x.device, grad_out, out, x, weight, R, K, N, ws, gx, *grads.buffers,
                    timer=f"narrow_linear_relu_backward[{R}x{K}x{N}]")
        return (gx, *grads.handed_back())


NARROW_MAX_IN = 16


def narrow_linear_relu(x, weight, bias=None):
    """relu(x W^T + b) for an input of at most 16 columns: x [..., K] -> [..., N]."""
    _lib.require_hip("narrow_linear_relu", x)
    lead = x.shape[:-1]
    out = _NarrowLinearReLU.apply(_f32c(x).reshape(-1, x.shape[-1]), weight, bias)
    return out.view(*lead, weight.shape[0])


class _RelationHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, weight, bias, mask):
        R, K = h.shape
        dev = h.device
        ws = torch.empty(_lib.query("mpa_relation_head_workspace", R, K), dtype=torch.float32, device=dev)
        out = torch.empty(R, dtype=torch.float32, device=dev)
        w = weight.reshape(-1)  # the Linear weight [1, K]: the same bytes
        _lib.launch("mpa_relation_head_forward", dev, h, w, bias, mask, R, K, ws, out,
                    timer=f"relation_head_forward[{R}x{K}]")
        GradSink.register(ctx, (weight, bias))
        ctx.save_for_backward(h, w, mask, ws)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        h, w, mask, ws = ctx.saved_tensors
        R, K = h.shape
        dev = h.device
        gh = torch.empty_like(h) if ctx.needs_input_grad[0] else None
        grads = GradSink.outputs(ctx.params)
        grad_out = grad_out.contiguous()
        _lib.launch("mpa_relation_head_backward", dev, grad_out, h, w, mask, R, K, ws, gh, *grads.buffers,
                    timer=f"relation_head_backward[{R}x{K}]")
        return (gh, *grads.handed_back(), None)


def relation_head_supported(width):
    return width % 4 == 0 and 4 <= width <= 4096


def relation_head(h, weight, bias=None, mask=None):
    """sigmoid(h . w + b) [* mask]: h [..., K], weight [1, K] -> [...] (mask, if given, has the leading shape of h)."""
    _lib.require_hip("relation_head", h)
    lead = h.shape[:-1]
    m = None if mask is None else _f32c(mask.detach()).reshape(-1)
    return _RelationHead.apply(_f32c(h).reshape(-1, h.shape[-1]), weight, bias, m).view(*lead)


class _RelationMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, edge, rel):
        G, P, C = edge.shape
        out = torch.empty((G, C), dtype=torch.float32, device=edge.device)
        _lib.launch("mpa_relation_mean_forward", edge.device, edge, rel, G, P, C, out,
                    timer=f"relation_mean_forward[{G}x{P}x{C}]")
        ctx.save_for_backward(edge, rel, out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        edge, rel, out = ctx.saved_tensors
        G, P, C = edge.shape
        ge = torch.empty_like(edge) if ctx.needs_input_grad[0] else None
        gr = torch.empty_like(rel) if ctx.needs_input_grad[1] else None
        grad_out = grad_out.contiguous()
        _lib.launch("mpa_relation_mean_backward", edge.device, grad_out, edge, rel, out, G, P, C, ge, gr,
                    timer=f"relation_mean_backward[{G}x{P}x{C}]")
        return ge, gr


RELATION_MEAN_MAX_PARTS = 64


def relation_mean(edge, rel):
    """edge [B, P, P, C], rel [B, P, P] -> [B, P, C]: sum_j edge_ij rel_ij / (sum_j rel_ij + 1e-6)."""
    _lib.require_hip("relation_mean", edge)
    B, P, P2, C = edge.shape
    out = _RelationMean.apply(_f32c(edge).reshape(B * P, P2, C), _f32c(rel).reshape(B * P, P2))
    return out.view(B, P, C)


class _PairRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, swap):
        S, P, F = a.shape
        out = torch.empty((S, P, P, 2 * F), dtype=torch.float32, device=a.device)
        _lib.launch("mpa_pair_rows_forward", a.device, a, b, S, P, F, int(swap), out,
                    timer=f"pair_rows_forward[{S}x{P}x{F}]")
        ctx.dims = (S, P, F, int(swap))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        S, P, F, swap = ctx.dims
        dev = grad_out.device
        ga = torch.empty((S, P, F), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        gb = torch.empty((S, P, F), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        grad_out = grad_out.contiguous()
        _lib.launch("mpa_pair_rows_backward", dev, grad_out, S, P, F, swap, ga, gb,
                    timer=f"pair_rows_backward[{S}x{P}x{F}]")
        return ga, gb, None


def pair_rows_supported(width):
    return width % 4 == 0 and 4 <= width <= 65536


def pair_rows(a, b, swap=False):
    """a, b [S, P, F] -> [S, P, P, 2F]: row (s, i, j) = [a[s, i] ; b[s, j]] (swap: [b[s, j] ; a[s, i]])."""
    _lib.require_hip("pair_rows", a)
    return _PairRows.apply(_f32c(a), _f32c(b), bool(swap))


class _MergeEqualParts(torch.autograd.Function):
    @staticmethod
    def forward(ctx, part_feats, pose_feats, valids, ids):
        B, P, C1 = part_feats.shape
        C2 = pose_feats.shape[-1]
        dev = part_feats.device
        part_out, pose_out = torch.empty_like(part_feats), torch.empty_like(pose_feats)
        arg_part = torch.empty((B, P, C1), dtype=torch.uint8, device=dev)
        arg_pose = torch.empty((B, P, C2), dtype=torch.uint8, device=dev)
        _lib.launch("mpa_merge_equal_parts", dev, part_feats, pose_feats, valids, ids, B, P, C1, C2, part_out, pose_out,
                    arg_part, arg_pose, timer=f"merge_equal_parts[{B}x{P}x{C1}+{C2}]")
        ctx.save_for_backward(arg_part, arg_pose, valids, ids)
        ctx.mark_non_differentiable(arg_part, arg_pose)
        return part_out, pose_out, arg_part, arg_pose

    @staticmethod
    def backward(ctx, g_part, g_pose, _ga, _gb):
        arg_part, arg_pose, valids, ids = ctx.saved_tensors
        B, P, C1 = arg_part.shape
        C2 = arg_pose.shape[-1]
        dev = arg_part.device
        g_part = torch.zeros((B, P, C1), dtype=torch.float32, device=dev) if g_part is None else _f32c(g_part)
        g_pose = torch.zeros((B, P, C2), dtype=torch.float32, device=dev) if g_pose is None else _f32c(g_pose)
        grad_part, grad_pose = torch.empty_like(g_part), torch.empty_like(g_pose)
        _lib.launch("mpa_merge_equal_parts_backward", dev, g_part, g_pose, arg_part, arg_pose, valids, ids, B, P, C1,
                    C2, grad_part, grad_pose, timer=f"merge_equal_parts_backward[{B}x{P}x{C1}+{C2}]")
        return grad_part, grad_pose, None, None


MERGE_MAX_PARTS = 64


def merge_equal_parts(part_feats, pose_feats, part_valids, part_ids, ret_arg=False):
    """Every class of equivalent parts (valid slots of a sample with equal `part_ids`) shares the channel-wise max of its
    members' features: part_feats [B, P, C1], pose_feats [B, P, C2] -> the two merged tensors, in one launch, with no
    host copy of the ids (`DGLModel._merge_nodes` is the host loop it replaces; bit-equal).  Valid parts come first in
    every sample.  ret_arg: also the uint8 slot every value came from (the lowest on ties)."""
    _lib.require_hip("merge_equal_parts", part_feats)
    valids = _f32c(part_valids.detach())
    ids = part_ids.detach().to(torch.int32).contiguous()
    out = _MergeEqualParts.apply(_f32c(part_feats), _f32c(pose_feats), valids, ids)
    return out if ret_arg else out[:2]
