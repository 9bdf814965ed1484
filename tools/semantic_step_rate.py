"""Cost of one semantic (PartNet-like) training step with the host in the loop and without it.  One JSON line:

  models   global_partnet_chair, dgl_partnet_chair, rgl_net_partnet_chair at B = 32, P = 20, N = 1000 on
           `synthetic.make_partnet_like_batch`; and `c1`: B-Global at the plumbing shape B = 4, P = 2 (`make_semantic_batch`)
  arms     a  matching sub-samples drawn on the host (torch.randperm per group, pinned copy), equivalent parts merged by
              the host loop — the path before csrc/match_sample.hip and the merge kernels existed
           b  cfg.loss.match_sample = "device" and merge_on_device: eager launches
           c  arm b captured as one HIP graph (Trainer(use_graph=True))
  *_ms     ms per `Trainer.train_step`: a host clock around a window of steps that ends in a device synchronise, divided
           by its steps; the three arms run in ONE process, in alternating windows after a warm-up of every arm (the
           capture included); the median of the windows is reported, the windows themselves beside it
  *_spread_a   max - min of arm a's windows: the margin of `b_not_slower` (b_ms <= a_ms + spread_a)

GPU only:  python tools/semantic_step_rate.py [--steps 10] [--windows 5] [--models global,dgl,rgl_net,c1] [--arms a,b,c]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_rig as rig  # noqa: E402  (puts the repository root on sys.path)
from multi_part_assembly_amd import config, synthetic  # noqa: E402
from multi_part_assembly_amd.pn_transformer import build_model  # noqa: E402
from multi_part_assembly_amd.trainer import Trainer  # noqa: E402

PRESETS = {"global": config.global_partnet_chair, "dgl": config.dgl_partnet_chair, "rgl_net": config.rgl_net_partnet_chair,
           "c1": config.global_partnet_chair}


def make_arm(name, arm, dev, P):
    cfg = PRESETS[name]()
    cfg.data.max_num_part = P
    if arm != "a":
        cfg.loss.match_sample = "device"
    torch.manual_seed(0)
    model = build_model(cfg).to(dev)
    if hasattr(model, "merge_on_device"):
        model.merge_on_device = arm != "a"
    return Trainer(model, cfg, use_graph=arm == "c", graph_warmup=2)


def measure(name, dev, args):
    if name == "c1":
        B, P, N = 4, 2, 1000
        batches = [synthetic.make_semantic_batch(B, max_parts=P, num_points=N, seed=1234 + i, device=dev) for i in range(2)]
    else:
        B, P, N = 32, 20, 1000
        batches = [synthetic.make_partnet_like_batch(B, P, N, seed=1234 + i, device=dev) for i in range(2)]
    for b in batches:
        b.pop("num_parts", None)
    steps = args.steps * (8 if name == "c1" else 1)  # a window of a fraction of a second measures the clock
    trainers = {arm: make_arm(name, arm, dev, P) for arm in args.arms}

    def step(tr):
        return lambda i: tr.train_step(batches[i % len(batches)], i)

    # warm-up of every arm: first launches, allocator, the capture of arm c
    timed = rig.alternate({arm: step(tr) for arm, tr in trainers.items()}, steps, args.windows, 4)
    out = {"B": B, "P": P, "N": N, "steps_per_window": steps,
           "valid_parts": int(sum(float(b["part_valids"].sum()) for b in batches) / len(batches)),
           "groups": int(sum(float(b["match_ids"].max(dim=1)[0].sum()) for b in batches) / len(batches))}
    rig.report(out, timed)
    if "c" in trainers:
        out["c_captured"] = trainers["c"]._graph is not None
    if "a" in timed:
        out["spread_a"] = round(max(timed["a"][1]) - min(timed["a"][1]), 4)
        if "b" in timed:
            out["b_not_slower"] = out["b_ms"] <= out["a_ms"] + out["spread_a"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--models", default="global,dgl,rgl_net,c1")
    ap.add_argument("--arms", default="a,b,c")
    args = ap.parse_args()
    args.arms = [a for a in args.arms.split(",") if a]
    rig.require_gpu("semantic_step_rate")
    dev = torch.device("cuda:0")
    result = {"windows": args.windows}
    for name in args.models.split(","):
        result[name] = measure(name, dev, args)
    rig.emit(result, None)


if __name__ == "__main__":
    main()
