"""Evaluation path of the PointNet++ set-abstraction levels on csrc/pointnet2_sa_mlp.hip: in eval() mode every BatchNorm
is a fixed per-channel affine map, so a level is gather -> three (GEMM, scale / shift, ReLU) -> max over the samples, and
one kernel does it per centre without the [M, C, S, K] tensors of the library chain (`PointnetSAModule.forward`).

Sampling (furthest point sampling, ball query) and the centres' gather are the calls of `pointnet2_utils`, unchanged.
Features travel POINT-major ([n, N, C]) between the levels — a gathered row is contiguous — and are transposed only
where the module contract [n, C', S] is asked for.

The layers are packed (bf16 split planes of W, scale and shift from the running statistics) on the device on EVERY
forward and never cached: the trainer's fused Adam writes the parameters through the flat buffer's raw pointer, which
moves no tensor `_version`, so a cache could serve stale weights at the next validation pass.  Three small launches a level.

CPU tensors run the numpy restatement `pointnet2_ref.sa_mlp_max` in their own dtype (float32 or float64), as every
function of `pointnet2_utils` does.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import _lib, pointnet2_ref, pointnet2_utils

K_CHUNK = 32            # Cin of a packed layer is zero-padded to this
MAX_WIDTH = 512


def packed_bytes(cout: int, cin: int) -> int:
    return _lib.query("mpa_sa_mlp_packed_bytes", cout, cin)


def pack_layer(conv: nn.Conv2d, bn: nn.BatchNorm2d) -> torch.Tensor:
    """One (1x1 Conv2d without bias, BatchNorm2d) pair -> the packed layer of mpa_sa_mlp_pack, a uint8 device tensor."""
    cout, cin = conv.weight.shape[0], conv.weight.shape[1]
    w = conv.weight.detach().reshape(cout, cin).float().contiguous()
    dev = w.device
    buf = torch.empty(packed_bytes(cout, cin), dtype=torch.uint8, device=dev)
    _lib.launch("mpa_sa_mlp_pack", dev, w, bn.weight.detach().float().contiguous(), bn.bias.detach().float().contiguous(),
                bn.running_mean.float().contiguous(), bn.running_var.float().contiguous(), float(bn.eps), cout, cin, buf)
    return buf


def unpack_layer(buf: torch.Tensor, cout: int, cin: int):
    """The contents of a packed layer: planes [3, Cout, Cinp] (h, m, l as float32), scale [Cout], shift [Cout]."""
    cinp = -(-cin // K_CHUNK) * K_CHUNK
    nplane = 6 * cout * cinp
    planes = buf[:nplane].view(torch.bfloat16).view(cinp // K_CHUNK, cout, 3, K_CHUNK)
    planes = planes.permute(2, 1, 0, 3).reshape(3, cout, cinp).float()
    ss = buf[nplane:nplane + 8 * cout].view(torch.float32)
    return planes, ss[:cout].clone(), ss[cout:].clone()


def sa_mlp_max(xyz, new_xyz, features_pm, idx, packed, widths):
    """mpa_sa_mlp_max_forward: xyz [M, N, 3], new_xyz [M, S, 3] | None, features_pm [M, N, C] | None, idx [M, S, K] | None
    (both None: one group of every point), three packed layers of `widths` -> [M, S, C3]."""
    M, N, _ = xyz.shape
    S, K = (1, N) if idx is None else (idx.shape[1], idx.shape[2])
    C = 0 if features_pm is None else features_pm.shape[2]
    out = torch.empty((M, S, widths[2]), dtype=torch.float32, device=xyz.device)
    _lib.launch("mpa_sa_mlp_max_forward", xyz.device, xyz, new_xyz, features_pm, idx, M, N, S, K, C, *packed, *widths, out,
                timer=f"sa_mlp_max_forward[{M}x{S}x{K} {3 + C}-{'-'.join(map(str, widths))}]")
    return out


def envelope_miss(module) -> str | None:
    """Why a `PointnetSAModule` is outside the fused kernel's envelope (None: it is inside)."""
    if len(module.mlps) != 1:
        return f"{len(module.mlps)} scales"
    grouper, mlp = module.groupers[0], module.mlps[0]
    if not grouper.use_xyz:
        return "use_xyz = False"
    layers = list(mlp)
    if len(layers) != 9:
        return f"a shared MLP of {len(layers)} sub-modules (three Conv2d / BatchNorm2d / ReLU layers are built)"
    for i in range(0, 9, 3):
        conv, bn = layers[i], layers[i + 1]
        if not (isinstance(conv, nn.Conv2d) and conv.bias is None and isinstance(bn, nn.BatchNorm2d)):
            return "a layer without BatchNorm"
        if bn.running_mean is None or bn.weight is None:
            return "a BatchNorm without running statistics or affine parameters"
        if conv.out_channels % 32 != 0 or not 32 <= conv.out_channels <= MAX_WIDTH:
            return f"width {conv.out_channels}"
    if layers[0].in_channels - 3 > MAX_WIDTH:
        return f"{layers[0].in_channels - 3} input features"
    return None


def _level_layers(module):
    layers = list(module.mlps[0])
    return [(layers[i], layers[i + 1]) for i in range(0, 9, 3)]


def _host_layers(pairs, dtype):
    """(W, scale, shift) of every layer in numpy, in `dtype`: the pack call's definition."""
    out = []
    for conv, bn in pairs:
        w = conv.weight.detach().reshape(conv.weight.shape[0], -1).numpy().astype(dtype)
        scale, shift = pointnet2_ref.sa_scale_shift(*[t.detach().numpy().astype(dtype) for t in
                                                      (bn.weight, bn.bias, bn.running_mean, bn.running_var)], bn.eps)
        out.append((w, scale, shift))
    return out


def sa_level_eval(module, xyz, features_pm):
    """One level in evaluation: xyz [n, N, 3], features_pm [n, N, C] | None -> new_xyz [n, S, 3] | None, features
    [n, S, C'] point-major (S = 1 for the level that groups every point)."""
    new_xyz = idx = None
    if module.npoint is not None:
        grouper = module.groupers[0]
        centres = pointnet2_utils.furthest_point_sample(xyz, module.npoint)
        new_xyz = pointnet2_utils.gather_operation(xyz.transpose(1, 2).contiguous(), centres)
        new_xyz = new_xyz.transpose(1, 2).contiguous().to(xyz.dtype)
        idx = pointnet2_utils.ball_query(grouper.radius, grouper.nsample, xyz, new_xyz)
    pairs = _level_layers(module)
    if not xyz.is_cuda:
        dtype = np.float64 if xyz.dtype == torch.float64 else np.float32
        out = pointnet2_ref.sa_mlp_max(xyz.detach().numpy().astype(dtype),
                                       None if new_xyz is None else new_xyz.numpy().astype(dtype),
                                       None if features_pm is None else features_pm.detach().numpy().astype(dtype),
                                       None if idx is None else idx.numpy(), _host_layers(pairs, dtype))
        return new_xyz, torch.from_numpy(out)
    packed = [pack_layer(conv, bn) for conv, bn in pairs]
    widths = [conv.out_channels for conv, _ in pairs]
    feats = None if features_pm is None else features_pm.float().contiguous()
    return new_xyz, sa_mlp_max(xyz.float().contiguous(), new_xyz, feats, idx, packed, widths)
