"""Evaluation cost of the PointNet++ SSG encoder: `PointNet2SSG(128).eval()` under `no_grad` on --clouds clouds of 1000
points (352: the valid parts of a B = 32 everyday batch), its two evaluation paths side by side.  One JSON line:

  ms_library / ms_fused            one forward with eval_mlp = "library" (Conv2d / BatchNorm2d / ReLU / max_pool2d over the
                                   grouped tensors) and with eval_mlp = "fused" (csrc/pointnet2_sa_mlp.hip)
  peak_mib_library / peak_mib_fused   rise of torch.cuda.max_memory_allocated over one such forward
  ms_sa{1,2,3}_library / _fused    per level on the same centres and indices: the library chain of the level (grouping, the
                                   shared MLP, the max) next to the level's three pack launches + the fused kernel
  ms_sa{1,2,3}_kernel              the fused kernel alone (layers packed beforehand)
  max_rel_diff                     max |fused - library| / max |library| of the encoder output
  *_windows                        all arms in ONE process, alternating windows after a warm-up; each figure is a host clock
                                   around a window that ends in a device synchronise, divided by its calls; the median is reported

GPU only:  python tools/pointnet2_eval_rate.py [--clouds 352] [--calls 5] [--windows 5] [--out FILE]"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_rig as rig  # noqa: E402  (puts the repository root on sys.path)
from multi_part_assembly_amd import pointnet2_fused as fused  # noqa: E402
from multi_part_assembly_amd import pointnet2_utils as pu  # noqa: E402
from multi_part_assembly_amd.pointnet2 import PointNet2SSG  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clouds", type=int, default=352)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default="")
    return ap.parse_args(argv)


@torch.no_grad()
def main(argv=None):
    args = parse_args(argv)
    dev = torch.device("cuda:0")
    M = args.clouds
    g = torch.Generator(device=dev).manual_seed(0)
    pts = torch.rand(M, 1000, 3, device=dev, generator=g) - 0.5
    torch.manual_seed(0)
    enc = PointNet2SSG(128).to(dev).train()
    enc(pts[:8])                                   # running statistics of a forward, not the initial (0, 1)
    enc.eval()
    arms = {"library": lambda: enc.set_eval_mlp("library")(pts), "fused": lambda: enc.set_eval_mlp("fused")(pts)}
    # per level, on the library run's own centres, indices and features
    levels = []
    enc.set_eval_mlp("library")(pts, record=levels)
    xyz, feats = pts, None
    for i, (module, (new_xyz, out)) in enumerate(zip(enc.SA_modules, levels)):
        idx = None if new_xyz is None else pu.ball_query(module.groupers[0].radius, module.groupers[0].nsample, xyz, new_xyz)
        feats_pm = None if feats is None else feats.transpose(1, 2).contiguous()
        pairs = fused._level_layers(module)
        widths = [conv.out_channels for conv, _ in pairs]
        packed = [fused.pack_layer(conv, bn) for conv, bn in pairs]

        def library(module=module, xyz=xyz, new_xyz=new_xyz, feats=feats):
            h = module.mlps[0](module.groupers[0](xyz, new_xyz, feats))
            return F.max_pool2d(h, kernel_size=[1, h.size(3)])

        def level(xyz=xyz, new_xyz=new_xyz, feats_pm=feats_pm, idx=idx, pairs=pairs, widths=widths):
            return fused.sa_mlp_max(xyz, new_xyz, feats_pm, idx, [fused.pack_layer(c, b) for c, b in pairs], widths)

        def kernel(xyz=xyz, new_xyz=new_xyz, feats_pm=feats_pm, idx=idx, packed=packed, widths=widths):
            return fused.sa_mlp_max(xyz, new_xyz, feats_pm, idx, packed, widths)

        arms[f"sa{i + 1}_library"], arms[f"sa{i + 1}_fused"], arms[f"sa{i + 1}_kernel"] = library, level, kernel
        xyz, feats = (new_xyz, out)
    result = {"clouds": M, "points": 1000, "calls_per_window": args.calls, "windows": args.windows}
    outs = {}
    for k in ("library", "fused"):
        arms[k]()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        outs[k] = arms[k]()
        torch.cuda.synchronize()
        result[f"peak_mib_{k}"] = round((torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20, 1)
    result["max_rel_diff"] = float((outs["fused"] - outs["library"]).abs().max() / outs["library"].abs().max())
    timed = rig.alternate({k: lambda i, fn=fn: fn() for k, fn in arms.items()}, args.calls, args.windows, 1)
    rig.report(result, timed, key="ms_{name}")
    rig.emit(result, args.out)


if __name__ == "__main__":
    main()
