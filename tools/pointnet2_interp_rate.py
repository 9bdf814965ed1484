"""Cost of the PointNet++ feature-propagation operators (csrc/pointnet2_interp.hip) on 352 clouds of n = 1000 unknown points,
m = 128 and m = 512 known points, C = 256 channels, each next to the same operator composed from library operators.  One
JSON line:

  ms_three_nn_m{128,512}         three nearest neighbours (distances and indices); `_torch`: `cdist`, `topk(3, largest=False)`
                                 — not the pinned tie order or arithmetic, a yardstick for time only
  ms_interp_fwd_m{128,512}       three_interpolate forward; `_torch`: `gather`, a multiply and a sum over the three
  ms_interp_bwd_m{128,512}       its backward; `_torch`: `index_add_` of the weighted gradients (float atomics: another order)
  *_torch_agrees                 whether the composition chose the same neighbours / came within 1e-5 of the operator
  *_windows                      all arms in ONE process, alternating windows after a warm-up; each figure is a host clock
                                 around a window that ends in a device synchronise, divided by its calls; the median is reported

GPU only:  python tools/pointnet2_interp_rate.py [--clouds 352] [--calls 5] [--windows 5] [--out FILE]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_rig as rig  # noqa: E402  (puts the repository root on sys.path)
from multi_part_assembly_amd import pointnet2_utils as pu  # noqa: E402


def three_nn_torch(unknown, known):
    dist, idx = torch.cdist(unknown, known).topk(3, dim=2, largest=False)
    return dist, idx.int()


def interp_torch(features, idx, weight):
    M, C, _ = features.shape
    n = idx.shape[1]
    flat = idx.long().reshape(M, 1, -1).expand(-1, C, -1)
    return (features.gather(2, flat).reshape(M, C, n, 3) * weight[:, None]).sum(-1)


def interp_bwd_torch(grad_out, idx, weight, m):
    M, C, n = grad_out.shape
    out = torch.zeros((M, m, C), device=grad_out.device)
    terms = (grad_out[..., None] * weight[:, None]).reshape(M, C, 3 * n).transpose(1, 2)            # [M, 3 n, C]
    flat = (idx.long().reshape(M, -1) + m * torch.arange(M, device=idx.device)[:, None]).reshape(-1)
    return out.reshape(M * m, C).index_add_(0, flat, terms.reshape(-1, C)).reshape(M, m, C).transpose(1, 2)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clouds", type=int, default=352)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default="")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    dev = torch.device("cuda:0")
    M, n, C = args.clouds, args.points, args.channels
    g = torch.Generator(device=dev).manual_seed(0)
    unknown = torch.rand(M, n, 3, device=dev, generator=g) - 0.5
    result = {"clouds": M, "unknown_points": n, "channels": C, "calls_per_window": args.calls, "windows": args.windows}
    arms = {}
    for m in (128, 512):
        known = torch.rand(M, m, 3, device=dev, generator=g) - 0.5
        dist, idx = pu.three_nn(unknown, known)
        recip = 1.0 / (dist + 1e-8)
        weight = recip / recip.sum(dim=2, keepdim=True)
        feat = torch.randn(M, C, m, device=dev, generator=g)
        grad = torch.randn(M, C, n, device=dev, generator=g)
        out, back = pu._interpolate_forward(feat, idx, weight), pu._interpolate_backward(grad, idx, weight, m)
        result[f"three_nn_m{m}_torch_agrees"] = bool(torch.equal(three_nn_torch(unknown, known)[1], idx))
        result[f"interp_fwd_m{m}_torch_agrees"] = bool((interp_torch(feat, idx, weight) - out).abs().max() <= 1e-5 * out.abs().max())
        result[f"interp_bwd_m{m}_torch_agrees"] = bool((interp_bwd_torch(grad, idx, weight, m) - back).abs().max()
                                                       <= 1e-5 * back.abs().max())
        arms.update({
            f"three_nn_m{m}": lambda i, known=known: pu.three_nn(unknown, known),
            f"three_nn_m{m}_torch": lambda i, known=known: three_nn_torch(unknown, known),
            f"interp_fwd_m{m}": lambda i, a=(feat, idx, weight): pu._interpolate_forward(*a),
            f"interp_fwd_m{m}_torch": lambda i, a=(feat, idx, weight): interp_torch(*a),
            f"interp_bwd_m{m}": lambda i, a=(grad, idx, weight, m): pu._interpolate_backward(*a),
            f"interp_bwd_m{m}_torch": lambda i, a=(grad, idx, weight, m): interp_bwd_torch(*a),
        })
    rig.report(result, rig.alternate(arms, args.calls, args.windows, 1), key="ms_{name}")
    rig.emit(result, args.out)


if __name__ == "__main__":
    main()
