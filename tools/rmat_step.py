"""Time the c2 training step (PNTransformer + PointNet, B=32, P=20, N=1000, everyday-like clouds) with quaternion and with
6D / rotation-matrix poses (`cfg.model.rot_type = 'quat' | 'rmat'`), on bench.py's protocol: its four batches, the same
initial weights, W untimed warm-up steps, the garbage collector off, then K steps between two device fences.

    python tools/rmat_step.py [--steps 100] [--warmup 20] [--repeats 3]

Prints one JSON line: ms per step of each form (best of `repeats` alternating runs) and the rmat / quat ratio.
"""
from __future__ import annotations

import argparse
import gc
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_rig as rig  # noqa: E402  (puts the repository root on sys.path)
import bench  # noqa: E402
from multi_part_assembly_amd.pn_transformer import build_model  # noqa: E402
from multi_part_assembly_amd.trainer import Trainer  # noqa: E402


def run(rot_type, batches, steps, warmup, dev):
    cfg = bench.workload("c2", 0, dev)[0]
    cfg.model.rot_type = rot_type
    torch.manual_seed(0)
    model = build_model(cfg).to(dev)
    trainer = Trainer(model, cfg)
    gc.collect()
    gc.disable()
    try:
        for i in range(warmup):
            trainer.train_step(batches[i % len(batches)], i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            loss = trainer.train_step(batches[i % len(batches)], i)
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
    finally:
        gc.enable()
    return 1e3 * elapsed / steps, float(loss)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    batches = [bench.workload("c2", 0, dev, k)[1] for k in range(bench.N_BATCHES)]
    for b in batches:
        b.pop("num_parts")
    best = {"quat": float("inf"), "rmat": float("inf")}
    losses = {}
    for _ in range(args.repeats):
        for rot_type in ("quat", "rmat"):
            ms, loss = run(rot_type, batches, args.steps, args.warmup, dev)
            best[rot_type] = min(best[rot_type], ms)
            losses[rot_type] = loss
    rig.emit({"workload": "c2", "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
              "quat_ms_per_step": best["quat"], "rmat_ms_per_step": best["rmat"],
              "rmat_over_quat": best["rmat"] / best["quat"], "final_loss": losses}, None)


if __name__ == "__main__":
    main()
