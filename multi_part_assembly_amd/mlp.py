"""One MLP layer (Linear / Conv1d k=1 [+ BatchNorm1d] [+ ReLU]) over rows on the HIP library (csrc/mlp.hip) — the building
block of the graph networks' edge / node MLPs and relation nets (reference models/dgl/modules.py:5-73,
models/rgl_net/modules.py:5-30).  The torch modules keep holding the parameters (same state_dict keys); this only
replaces what `conv(x)`, `bn(.)`, `relu(.)` compute."""
from __future__ import annotations

import torch

from . import _lib
from .gradsink import GradSink


class _MLPLayerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, running, training, momentum, eps, relu):
        R, K = x.shape
        N = weight.shape[0]
        w = weight.reshape(N, -1)  # a Conv1d weight [N, K, 1] or a Linear weight [N, K]: the same bytes
        dev = x.device
        ws = torch.empty(_lib.query("mpa_mlp_layer_workspace", R, K, N), dtype=torch.uint8, device=dev)
        out = torch.empty((R, N), dtype=torch.float32, device=dev)
        rm, rv = running if running is not None else (None, None)
        _lib.launch("mpa_mlp_layer_forward", dev, x, x.stride(0), w, bias, gamma, beta, rm, rv, int(training),
                    float(momentum), float(eps), int(relu), R, K, N, ws, out, timer=f"mlp_layer_forward[{R}x{K}x{N}]")
        ctx.meta = (bool(relu), bool(training), gamma is not None)
        # the parameters themselves (not views of them): with a GradSink active their gradients are written straight
        # into the flat gradient buffer instead of going through one AccumulateGrad `add` launch per parameter
        GradSink.register(ctx, (weight, bias, gamma, beta))
        ctx.save_for_backward(x, w, gamma, out, ws)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if getattr(ctx, "consumed", False):
            raise RuntimeError("MLP layer: the backward pass overwrites its saved workspace: a second backward over the "
                               "same forward (retain_graph=True) is not supported — run the forward again")
        ctx.consumed = True
        x, w, gamma, out, ws = ctx.saved_tensors
        relu, training, has_bn = ctx.meta
        if has_bn and not training:
            raise RuntimeError("MLP layer: backward is implemented for training-mode BatchNorm only")
        R, K = x.shape
        N = w.shape[0]
        dev = x.device
        gx = torch.empty((R, K), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        grads = GradSink.outputs(ctx.params)  # (weight, bias, gamma, beta): None where the layer has none
        grad_out = grad_out.contiguous()
        _lib.launch("mpa_mlp_layer_backward", dev, grad_out, x, x.stride(0), w, gamma, out, int(relu), R, K, N, ws, gx,
                    *grads.buffers, timer=f"mlp_layer_backward[{R}x{K}x{N}]")
        return (gx, *grads.handed_back(), None, None, None, None, None)


class _PairLayerFn(torch.autograd.Function):
    """First layer of the P x P edge MLP on (a_i, b_j) pairs without the pair tensor (csrc/mlp.hip: mpa_pair_layer_*)."""

    @staticmethod
    def forward(ctx, a, b, weight, bias, gamma, beta, running, training, momentum, eps, relu):
        B, P, F = a.shape
        N = weight.shape[0]
        w = weight.reshape(N, -1)  # Conv1d weight [N, 2F, 1]: the same bytes
        dev = a.device
        ws = torch.empty(_lib.query("mpa_pair_layer_workspace", B, P, F, N), dtype=torch.uint8, device=dev)
        out = torch.empty((B * P * P, N), dtype=torch.float32, device=dev)
        rm, rv = running
        _lib.launch("mpa_pair_layer_forward", dev, a, b, w, bias, gamma, beta, rm, rv, int(training), float(momentum),
                    float(eps), int(relu), B, P, F, N, ws, out, timer=f"pair_layer_forward[{B}x{P}x{P}x{2 * F}x{N}]")
        ctx.meta = (bool(relu), bool(training))
        ctx.same = a.data_ptr() == b.data_ptr() and a.shape == b.shape
        GradSink.register(ctx, (weight, bias, gamma, beta))
        ctx.save_for_backward(a, b, w, gamma, out, ws)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if getattr(ctx, "consumed", False):
            raise RuntimeError("pair layer: the backward pass overwrites its saved workspace: a second backward over the "
                               "same forward (retain_graph=True) is not supported — run the forward again")
        ctx.consumed = True
        a, b, w, gamma, out, ws = ctx.saved_tensors
        relu, training = ctx.meta
        if not training:
            raise RuntimeError("pair layer: backward is implemented for training-mode BatchNorm only")
        B, P, F = a.shape
        N = w.shape[0]
        dev = a.device
        ga = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        gb = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        same = ctx.same and ga is not None and gb is not None
        if same:
            gb = ga  # one tensor in both roles: the library adds the second half's gradient into the first's buffer
        grads = GradSink.outputs(ctx.params)  # (weight, bias, gamma, beta): None for an absent bias
        grad_out = grad_out.contiguous()
        _lib.launch("mpa_pair_layer_backward", dev, grad_out, a, b, w, gamma, out, int(relu), B, P, F, N, ws, ga, gb,
                    *grads.buffers, timer=f"pair_layer_backward[{B}x{P}x{P}x{2 * F}x{N}]")
        if same:
            gb = None  # (already inside ga)
        return (ga, gb, *grads.handed_back(), None, None, None, None, None)


def pair_layer_supported(feat, out_dim):
    return feat % 64 == 0 and 64 <= feat <= 2048 and supported(2 * feat, out_dim)


def pair_layer(a, b, weight, bias, bn, relu=True, training=True):
    """a, b [B, P, F] (CUDA) -> [B*P*P, N] = act(bn([a_i ; b_j] W^T + bias)), row (s, i, j) at (s*P + i)*P + j: the first
    Conv1d(k=1) + BatchNorm1d (+ ReLU) of the edge MLP over all part pairs, computed from two GEMMs over the B*P part rows
    (the pair tensor of dgl/network.py:135-144 is never built).  `weight` [N, 2F] or the Conv1d weight [N, 2F, 1]."""
    _lib.require_hip("pair_layer", a)
    a, b = a.float().contiguous(), b.float().contiguous()
    if training:
        _count_batch(bn)
    return _PairLayerFn.apply(a, b, weight, bias, bn.weight, bn.bias, (bn.running_mean, bn.running_var), training,
                              bn.momentum, bn.eps, relu)


class bn_counter_batch:
    """`with bn_counter_batch():` — the `num_batches_tracked += 1` of every BatchNorm layer that `mlp_layer` runs in
    training mode inside the block becomes ONE multi-tensor launch at its end instead of one launch per layer (18 per
    step for the graph networks).  A layer used k times in the block is advanced by k."""
    pending = None

    def __enter__(self):
        self.prev, bn_counter_batch.pending = bn_counter_batch.pending, {}
        return self

    def __exit__(self, *exc):
        items, bn_counter_batch.pending = bn_counter_batch.pending, self.prev
        if items:
            with torch.no_grad():
                torch._foreach_add_([t for t, _ in items.values()], [k for _, k in items.values()])
        return False


def _count_batch(bn):
    """bn.num_batches_tracked += 1 — now, or with the other layers' counters at the end of a bn_counter_batch block."""
    pend, t = bn_counter_batch.pending, bn.num_batches_tracked
    if pend is not None:
        pend[id(t)] = (t, pend.get(id(t), (t, 0))[1] + 1)
    else:
        with torch.no_grad():
            t += 1


def supported(in_dim, out_dim):
    return in_dim % 64 == 0 and out_dim % 64 == 0 and 64 <= in_dim <= 4096 and 64 <= out_dim <= 4096


def mlp_layer(x, weight, bias=None, bn=None, relu=True, training=True):
    """x [R, K] (CUDA, fp32, rows contiguous) -> [R, N] = act(bn(x W^T + b)).  `weight` [N, K] or a Conv1d weight
    [N, K, 1]; `bn`: an nn.BatchNorm1d (its running statistics are updated in training mode) or None."""
    _lib.require_hip("mlp_layer", x)
    x = x.float()
    if x.stride(1) != 1 or x.stride(0) % 4 != 0:
        x = x.contiguous()
    if bn is None:
        return _MLPLayerFn.apply(x, weight, bias, None, None, None, training, 0.0, 0.0, relu)
    if training:
        _count_batch(bn)
    return _MLPLayerFn.apply(x, weight, bias, bn.weight, bn.bias, (bn.running_mean, bn.running_var), training,
                             bn.momentum, bn.eps, relu)
