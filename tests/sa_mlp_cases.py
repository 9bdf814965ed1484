"""Shared pieces of tests/test_pointnet2_fused.py and tests/test_pointnet2_fused_gpu.py (a plain module, imported like
tests/anchored.py): seeded set-abstraction levels whose activations stay O(1) through three layers, the library chain of a
level (the grouped tensor, Conv2d / BatchNorm2d.eval() / ReLU, max_pool2d) on GIVEN indices in any dtype, and the reading
of the compacted records of tests/golden/pointnet2_ssg.npz."""
import sys

import numpy as np
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from multi_part_assembly_amd import pointnet2_fused as fused
from multi_part_assembly_amd import pointnet2_ref as ref
from multi_part_assembly_amd.pointnet2 import build_shared_mlp

sys.path.insert(0, str(GOLDEN))
import param_fill  # noqa: E402


def make_mlp(C, widths, seed):
    """A shared MLP 3 + C -> widths (float32, eval mode) with seeded weights of unit gain (He scale: a ReLU halves the
    second moment), perturbed BatchNorm scales of both signs, shifts and running statistics."""
    g = torch.Generator().manual_seed(seed)
    mlp = build_shared_mlp([3 + C, *widths], bn=True).eval()
    with torch.no_grad():
        for m in mlp:
            if isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / m.weight.shape[1]) ** 0.5)
            elif isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(1.0 + 0.3 * torch.rand(m.weight.shape, generator=g))
                m.weight[::5] *= -1.0
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
    return mlp


def pairs(mlp):
    layers = list(mlp)
    return [(layers[i], layers[i + 1]) for i in range(0, len(layers), 3)]


def host_layers(mlp, dtype):
    return fused._host_layers(pairs(mlp), dtype)


def make_inputs(M, N, S, K, C, seed, group_all=False):
    """xyz [M, N, 3], new_xyz [M, S, 3] | None, features point-major [M, N, C] | None, idx int32 [M, S, K] | None."""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(M, N, 3, generator=g) - 0.5
    feats = torch.randn(M, N, C, generator=g) if C > 0 else None
    if group_all:
        return xyz, None, feats, None
    new_xyz = xyz[:, torch.randint(0, N, (S,), generator=g)].contiguous() + 0.01
    idx = torch.randint(0, N, (M, S, K), generator=g, dtype=torch.int32)
    return xyz, new_xyz, feats, idx


def grouped(xyz, new_xyz, feats_pm, idx):
    """What QueryAndGroup / GroupAll hand to the shared MLP, [M, 3 + C, S, K], in the dtype of `xyz`, on given indices (an
    index outside [0, N) reads as zero, the rule of `grouping_operation`)."""
    M, N, _ = xyz.shape
    if idx is None:
        rows = xyz[:, None]
        if feats_pm is not None:
            rows = torch.cat([rows, feats_pm[:, None]], dim=-1)
        return rows.permute(0, 3, 1, 2).contiguous()
    ok = (idx >= 0) & (idx < N)
    safe = torch.where(ok, idx, torch.zeros_like(idx)).long()
    m = torch.arange(M)[:, None, None]
    rows = torch.where(ok[..., None], xyz[m, safe], torch.zeros((), dtype=xyz.dtype)) - new_xyz[:, :, None, :]
    if feats_pm is not None:
        rows = torch.cat([rows, torch.where(ok[..., None], feats_pm[m, safe], torch.zeros((), dtype=xyz.dtype))], dim=-1)
    return rows.permute(0, 3, 1, 2).contiguous()


def library_chain(mlp, g):
    """The library chain of `PointnetSAModule.forward` on a grouped tensor: [M, 3 + C, S, K] -> point-major [M, S, C3]."""
    with torch.no_grad():
        h = mlp(g)
        return F.max_pool2d(h, kernel_size=[1, h.size(3)]).squeeze(-1).transpose(1, 2).contiguous()


def references(mlp, xyz, new_xyz, feats, idx):
    """(r32, r64) of one level: the float32 library chain and the float64 restatement, on the same indices."""
    r32 = library_chain(mlp, grouped(xyz, new_xyz, feats, idx))
    d = lambda t: None if t is None else t.double().numpy()
    r64 = ref.sa_mlp_max(d(xyz), d(new_xyz), d(feats), None if idx is None else idx.numpy(), host_layers(mlp, np.float64))
    return r32, torch.from_numpy(r64)


def picked(a):
    """The elements `param_fill.compact` keeps of a tensor: all of a small one, a strided sample of a large one."""
    a = a.detach().cpu().reshape(-1)
    if a.numel() <= param_fill.FULL_LIMIT:
        return a
    return a[torch.from_numpy(np.linspace(0, a.numel() - 1, param_fill.SAMPLE).astype(np.int64))]


def records(fixture, prefix):
    out = {}
    for k, v in fixture.items():
        if k.startswith(prefix) and not k.endswith("#norms"):
            out[k[len(prefix):].replace("#sample", "")] = torch.from_numpy(v)
    return out


def fixture_encoder(fixture, device="cpu", feat_dim=128):
    """The fixture's encoder after its one training forward on the library chain (the running statistics are then the
    fixture's), in eval mode; and the fixture's points."""
    from multi_part_assembly_amd.pointnet2 import PointNet2SSG
    enc = PointNet2SSG(feat_dim)
    param_fill.fill_parameters(enc, int(fixture["seed"]))
    enc = enc.to(device).train()
    pts = torch.from_numpy(fixture["points"]).to(device)
    with torch.no_grad():
        enc(pts)
    return enc.eval(), pts
