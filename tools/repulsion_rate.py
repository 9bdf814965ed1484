"""Cost of the repulsion loss: csrc/repulsion.hip (`loss.repulsion_cd_loss(fused=True)`) against the reference's composition
(`fused=False`: two [B P P, N, 3] expansions and one Chamfer call over all P x P pairs), B = 32, P = 20, N = 1000, the
benchmark's synthetic batch with the part counts of `bench.representative_parts`.  One JSON line:

  cells              one per (pose set, threshold): `gt` = the parts posed by their ground truth (neighbours touch, most pairs
                     pruned), `origin` = every part at the origin (nothing pruned: the worst case).  In a cell:
    ms_{composed,fused}_{fwd,fwdbwd}   ms per call, forward alone (no graph) and forward + backward to the posed points; all
                     four arms in ONE process, alternating windows after a warm-up; each figure is a host clock around a
                     window that ends in a device synchronise, divided by its calls; the median of the windows, with the
                     windows beside it
    peak_mb_*        peak of the allocator above the resting level during one forward + backward of the arm
    pairs            valid pairs, and how many of them the fused forward searched / found hinged
    rel_diff         max |fused - composed| / max |composed| of the loss
    fused_wins       the fused arm is not slower than the composed arm of the same run, forward and forward + backward
  step               a c2 training step (pn_transformer + PointNet, eager `Trainer.train_step`) without the term and with it
                     (`repulsion_thre` = the first threshold, weight 1), same protocol

GPU only:  python tools/repulsion_rate.py [--calls 5] [--windows 5] [--thre 0.01 0.05] [--out profiles/r18_repulsion_rate.json]"""
import argparse
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_rig as rig  # noqa: E402  (puts the repository root on sys.path)
from multi_part_assembly_amd import config, synthetic  # noqa: E402
from multi_part_assembly_amd import loss as L  # noqa: E402
from multi_part_assembly_amd.transforms import transform_pc  # noqa: E402


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    rest = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn(0)
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - rest) / 2 ** 20, 1)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--parts", type=int, default=20)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--thre", type=float, nargs=2, default=(0.01, 0.05))
    ap.add_argument("--no-step", action="store_true", help="skip the training-step arms")
    ap.add_argument("--out", default="")
    return ap.parse_args(argv)


def cell(posed, valids, thre, args):
    x = posed.clone().requires_grad_()
    w = torch.ones(posed.shape[0], device=posed.device)

    def fwd(fused):
        with torch.no_grad():
            return L.repulsion_cd_loss(posed, valids, thre, fused=fused)

    def fwdbwd(fused):
        loss = L.repulsion_cd_loss(x, valids, thre, fused=fused)
        return torch.autograd.grad((loss * w).sum(), x)[0]

    arms = {"composed_fwd": lambda i: fwd(False), "fused_fwd": lambda i: fwd(True),
            "composed_fwdbwd": lambda i: fwdbwd(False), "fused_fwdbwd": lambda i: fwdbwd(True)}
    res = {"thre": thre}
    a, b = fwd(True), fwd(False)
    res["rel_diff"] = float(((a - b).abs().max() / b.abs().max()).item())
    flag = L.repulsion_cd_search(posed, valids, thre)["flag"]
    v = valids == 1
    res["pairs"] = {"valid": int(sum(int(n) * (int(n) - 1) // 2 for n in v.sum(1).tolist())),
                    "searched": int((flag > 0).sum().item()), "hinged": int((flag == 2).sum().item())}
    rig.report(res, rig.alternate(arms, args.calls, args.windows, 2), key="ms_{name}")
    res["peak_mb_composed"], res["peak_mb_fused"] = peak_mb(arms["composed_fwdbwd"]), peak_mb(arms["fused_fwdbwd"])
    res["fused_wins"] = bool(res["ms_fused_fwd"] <= res["ms_composed_fwd"] and res["ms_fused_fwdbwd"] <= res["ms_composed_fwdbwd"]
                             and res["peak_mb_fused"] < res["peak_mb_composed"])
    return res


def step_arms(batch, thre, args, dev):
    from multi_part_assembly_amd.pn_transformer import build_model
    from multi_part_assembly_amd.trainer import Trainer

    def trainer(term):
        cfg = config.pn_transformer_everyday()
        cfg.data.max_num_part = args.parts
        if term:
            cfg.loss.use_repulsion_loss, cfg.loss.repulsion_thre, cfg.loss.repulsion_loss_w = True, thre, 1.0
        torch.manual_seed(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return Trainer(build_model(cfg).to(dev), cfg)

    plain, term = trainer(False), trainer(True)
    arms = {"step": lambda i: plain.train_step(batch), "step_with_term": lambda i: term.train_step(batch)}
    timed = rig.alternate(arms, max(args.calls, 10), args.windows, 2)
    return {f"ms_{k}": (round(med, 4), [round(t, 4) for t in ts]) for k, (med, ts) in timed.items()}  # a pair per arm


def main(argv=None):
    args = parse_args(argv)
    dev = torch.device("cuda:0")
    B, P, N = args.batch, args.parts, args.points
    result = {"B": B, "P": P, "N": N, "calls_per_window": args.calls, "windows": args.windows, "cells": {}}
    parts = rig.representative_parts(1234)
    parts = [min(P, parts[b % len(parts)]) for b in range(B)]
    batch = synthetic.make_batch(B, P, N, seed=1234, device=dev, num_parts=parts)
    pcs, valids = batch["part_pcs"], batch["part_valids"]
    poses = {"gt": transform_pc(batch["part_trans"], batch["part_quat"], pcs, "quat").detach(),
             "origin": transform_pc(torch.zeros_like(batch["part_trans"]), batch["part_quat"], pcs, "quat").detach()}
    for name, posed in poses.items():
        for thre in args.thre:
            result["cells"][f"{name}@{thre:g}"] = cell(posed, valids, float(thre), args)
    result["fused_wins_every_cell"] = all(c["fused_wins"] for c in result["cells"].values())
    if not args.no_step:
        result["step"] = step_arms(batch, float(args.thre[0]), args, dev)
    rig.emit(result, args.out)


if __name__ == "__main__":
    main()
