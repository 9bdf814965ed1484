"""Cost of the PointNet++ operators (csrc/pointnet2_ops.hip) at the shapes of the SSG encoder, each next to the same operator
composed from library operators, and of the encoder's forward + backward.  One JSON line:

  ms_fps_sa1 / ms_fps_sa2        furthest point sampling [M, 1000] -> 512 and [M, 512] -> 128
  ms_fps_sa1_torch / ..._sa2_torch   the yardstick: a `torch` loop, one round per iteration (min, arg-max, gather) — not the
                                 pinned tie order, a yardstick for time only
  ms_ball_sa1 / ms_ball_sa2      ball query (radius 0.2 / 0.4, 64 samples); `_torch`: `cdist`, a sort of the masked indices
  ms_group_fwd_* / ms_group_bwd_*   grouping forward and backward at SA1's (C = 3, N = 1000, 512 x 64) and SA2's (C = 128,
                                 N = 512, 128 x 64) shapes; `_torch`: `gather` / `index_add_` (float atomics: another order)
  ms_encoder_fwd_bwd             `PointNet2SSG(128)` training forward + backward on --parts valid parts of 1000 points
  encoder_peak_mib               torch's peak allocated memory over one such forward + backward
  *_windows                      all arms in ONE process, alternating windows after a warm-up; each figure is a host clock
                                 around a window that ends in a device synchronise, divided by its calls; the median is reported

GPU only:  python tools/pointnet2_rate.py [--clouds 352] [--parts 88] [--calls 5] [--windows 5] [--out FILE]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_rig as rig  # noqa: E402  (puts the repository root on sys.path)
from multi_part_assembly_amd import pointnet2_utils as pu  # noqa: E402
from multi_part_assembly_amd.pointnet2 import PointNet2SSG  # noqa: E402


def fps_torch(xyz, npoint):
    M, N, _ = xyz.shape
    live = (xyz * xyz).sum(-1) > 1e-3
    temp = torch.full((M, N), 1e10, device=xyz.device)
    idx = torch.zeros((M, npoint), dtype=torch.int64, device=xyz.device)
    old = idx[:, 0]
    for j in range(1, npoint):
        d = (xyz - xyz.gather(1, old[:, None, None].expand(M, 1, 3))).square().sum(-1)
        temp = torch.where(live, torch.minimum(d, temp), temp)
        old = torch.where(live, temp, -1.0).argmax(dim=1)
        idx[:, j] = old
    return idx.int()


def ball_torch(radius, nsample, xyz, new_xyz):
    M, N, _ = xyz.shape
    hit = torch.cdist(new_xyz, xyz) < radius
    k = torch.arange(N, device=xyz.device).expand_as(hit)
    first = torch.where(hit, k, N).sort(dim=-1).values[..., :nsample]
    return torch.where(first < N, first, first[..., :1].clamp(max=N - 1) * (first[..., :1] < N)).int()


def group_torch(features, idx):
    M, C, N = features.shape
    flat = idx.long().reshape(M, 1, -1).expand(-1, C, -1)
    return features.gather(2, flat).reshape(M, C, *idx.shape[1:])


def group_bwd_torch(grad_out, idx, N):
    M, C = grad_out.shape[:2]
    out = torch.zeros((M * C, N), device=grad_out.device)
    flat = idx.long().reshape(M, 1, -1).expand(-1, C, -1).reshape(M * C, -1)
    return out.scatter_add_(1, flat, grad_out.reshape(M * C, -1)).reshape(M, C, N)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clouds", type=int, default=352)
    ap.add_argument("--parts", type=int, default=88)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default="")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    dev = torch.device("cuda:0")
    M = args.clouds
    g = torch.Generator(device=dev).manual_seed(0)
    xyz1 = torch.rand(M, 1000, 3, device=dev, generator=g) - 0.5
    idx1 = pu.furthest_point_sample(xyz1, 512)
    xyz2 = pu.gather_operation(xyz1.transpose(1, 2).contiguous(), idx1).transpose(1, 2).contiguous()
    idx2 = pu.furthest_point_sample(xyz2, 128)
    xyz3 = pu.gather_operation(xyz2.transpose(1, 2).contiguous(), idx2).transpose(1, 2).contiguous()
    ball1, ball2 = pu.ball_query(0.2, 64, xyz1, xyz2), pu.ball_query(0.4, 64, xyz2, xyz3)
    f1, f2 = xyz1.transpose(1, 2).contiguous(), torch.randn(M, 128, 512, device=dev, generator=g)
    g1, g2 = torch.randn(M, 3, 512, 64, device=dev, generator=g), torch.randn(M, 128, 128, 64, device=dev, generator=g)
    result = {"clouds": M, "encoder_parts": args.parts, "calls_per_window": args.calls, "windows": args.windows,
              "mean_ball_fill_sa1": round(float((ball1 != ball1[..., :1]).sum(-1).float().mean()) + 1, 2),
              "ball_torch_agrees": bool(torch.equal(ball_torch(0.2, 64, xyz1, xyz2), ball1)),
              "group_torch_agrees": bool(torch.equal(group_torch(f2, ball2), pu.grouping_operation(f2, ball2)))}
    arms = {
        "fps_sa1": lambda i: pu.furthest_point_sample(xyz1, 512),
        "fps_sa2": lambda i: pu.furthest_point_sample(xyz2, 128),
        "fps_sa1_torch": lambda i: fps_torch(xyz1, 512),
        "fps_sa2_torch": lambda i: fps_torch(xyz2, 128),
        "ball_sa1": lambda i: pu.ball_query(0.2, 64, xyz1, xyz2),
        "ball_sa2": lambda i: pu.ball_query(0.4, 64, xyz2, xyz3),
        "ball_sa1_torch": lambda i: ball_torch(0.2, 64, xyz1, xyz2),
        "ball_sa2_torch": lambda i: ball_torch(0.4, 64, xyz2, xyz3),
        "group_fwd_sa1": lambda i: pu._group_forward(f1, ball1),
        "group_fwd_sa2": lambda i: pu._group_forward(f2, ball2),
        "group_fwd_sa1_torch": lambda i: group_torch(f1, ball1),
        "group_fwd_sa2_torch": lambda i: group_torch(f2, ball2),
        "group_bwd_sa1": lambda i: pu._group_backward(g1, ball1, 1000),
        "group_bwd_sa2": lambda i: pu._group_backward(g2, ball2, 512),
        "group_bwd_sa1_torch": lambda i: group_bwd_torch(g1, ball1, 1000),
        "group_bwd_sa2_torch": lambda i: group_bwd_torch(g2, ball2, 512),
    }
    enc = PointNet2SSG(128).to(dev).train()
    parts = xyz1[:args.parts].contiguous()
    w = torch.randn(args.parts, 128, device=dev, generator=g)

    def encoder_step(i):
        enc.zero_grad(set_to_none=True)
        (enc(parts) * w).sum().backward()

    arms["encoder_fwd_bwd"] = encoder_step
    rig.window(encoder_step, 1)  # the peak is a warmed-up step's
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    rig.window(encoder_step, 1)
    result["encoder_peak_mib"] = round((torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20, 1)
    calls = {k: 1 if k in ("fps_sa1_torch", "fps_sa2_torch") else args.calls for k in arms}  # the torch loops are slow
    rig.report(result, rig.alternate(arms, calls, args.windows, 1), key="ms_{name}")
    rig.emit(result, args.out)


if __name__ == "__main__":
    main()
