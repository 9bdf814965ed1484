"""Cost of gradient accumulation (`Trainer(accumulate=K)`: csrc/grad_accumulate.hip mpa_grad_accumulate behind every
micro-batch's backward, the step's tail once per window) on the c2 configuration: pn_transformer, everyday preset, B = 32,
P = 20, N = 1000, part counts of `bench.representative_parts`.  One JSON line, also written to `--out` (default
profiles/r22_accumulate_rate.json):

  arms                  K in {1, 2, 4}  x  eager / captured (use_graph): six trainers in ONE process, alternating windows
                        after a warm-up (the captured arms warm up past their capture).  K = 1 is the yardstick: the step
                        of a trainer built without the argument.  A window is `--steps` optimiser steps = K x steps
                        `train_step` calls, so every window ends on a closed accumulation window
  *_micro_ms            ms per `train_step` (one micro-batch): a host clock around the window, which ends in a device
                        synchronise, divided by its calls; the median of the windows, the windows beside it
  *_step_ms             ms per optimiser step: K times that
  micro_minus_k1_ms     per arm with K > 1: its *_micro_ms minus the K = 1 arm's of the same mode.  A micro-batch saves
                        (K - 1) / K of a tail (the Adam launches) and pays one accumulate launch
  k1_spread_ms          max - min of the K = 1 arm's windows, per mode: the yardstick's own noise
  accumulate_*_alone_ms mpa_grad_accumulate alone in each mode on the model's flat gradient (back-to-back calls between
                        synchronises), its bytes (8 per parameter in FIRST, 12 in ADD and LAST) and GB/s from the median;
                        adam_step_dev_alone_ms likewise, on the same flat buffer
  peak_memory_*         torch.cuda.max_memory_allocated() after building and stepping a K = 1 / a K = 2 trainer alone, and
                        what the accumulator holds (`accumulator_bytes` = one flat buffer)

GPU only:  python tools/accumulate_rate.py [--steps 32] [--windows 5]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_rig as rig  # noqa: E402  (puts the repository root on sys.path)
from multi_part_assembly_amd import _lib, config  # noqa: E402
from multi_part_assembly_amd.pn_transformer import build_model  # noqa: E402
from multi_part_assembly_amd.trainer import Trainer  # noqa: E402

KS = (1, 2, 4)
MODES = (("first", 0, 8), ("add", 1, 12), ("last", 2, 12))


def arm_name(k, graph):
    return f"k{k}_{'graph' if graph else 'eager'}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32, help="optimiser steps per window (K times as many micro-batches)")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(rig.ROOT, "profiles", "r22_accumulate_rate.json"))
    args = ap.parse_args()
    rig.require_gpu("accumulate_rate")
    dev = torch.device("cuda:0")
    B, P, N = 32, 20, 1000
    batches = rig.c2_batches(dev, 4, B=B, P=P, N=N)

    def make(k, graph):
        torch.manual_seed(0)
        cfg = config.pn_transformer_everyday()
        return Trainer(build_model(cfg).to(dev), cfg, use_graph=graph) if k == 1 else \
            Trainer(build_model(cfg).to(dev), cfg, use_graph=graph, accumulate=k)

    def step(trainer):
        return lambda i: trainer.train_step(batches[i % len(batches)])

    result = {"B": B, "P": P, "N": N, "optimizer_steps_per_window": args.steps, "windows": args.windows, "K": list(KS)}
    # peak memory of one trainer alone, K = 1 then K = 2, before anything else lives on the device
    for k in (1, 2):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        trainer = make(k, False)
        rig.window(step(trainer), 4)
        result[f"peak_memory_k{k}_bytes"] = torch.cuda.max_memory_allocated(dev) - base
        if k > 1:
            result["accumulator_bytes"] = trainer.accumulator.acc.numel() * 4
        del trainer
    result["peak_memory_k2_minus_k1_bytes"] = result["peak_memory_k2_bytes"] - result["peak_memory_k1_bytes"]

    arms = {(k, graph): make(k, graph) for graph in (False, True) for k in KS}
    result["numel"] = arms[(2, False)].flat.numel
    names = {key: arm_name(*key) for key in arms}
    # warm-up of 8 calls (a multiple of every K): code objects, lazily built buffers, the capture (3 eager calls first)
    timed = rig.alternate({names[key]: step(trainer) for key, trainer in arms.items()},
                          {names[key]: key[0] * args.steps for key in arms}, args.windows, 8)
    rig.report(result, timed, key="{name}_micro_ms")
    for (k, graph), name in names.items():
        med, ts = timed[name]
        result[f"{name}_step_ms"] = round(k * med, 4)
        assert arms[(k, graph)].window == 0, "a timed window ended inside an accumulation window"
    for graph in (False, True):
        mode = "graph" if graph else "eager"
        base, base_ts = timed[arm_name(1, graph)]
        result.setdefault("k1_spread_ms", {})[mode] = round(max(base_ts) - min(base_ts), 4)
        for k in KS[1:]:
            result.setdefault("micro_minus_k1_ms", {})[arm_name(k, graph)] = round(timed[arm_name(k, graph)][0] - base, 4)

    # the kernel alone in each mode, on the model's own flat gradient and accumulator (a window is open on neither)
    on = arms[(2, False)]
    grad, acc, numel = on.flat.flat_grad, on.accumulator.acc, on.flat.numel
    grad.zero_(), acc.zero_()  # (sums of zeros: nothing overflows over the repeated calls)
    calls = 1000
    for name, mode, per_param in MODES:
        fn = lambda i, mode=mode: _lib.launch("mpa_grad_accumulate", dev, grad, acc, numel, mode, None)  # noqa: E731
        rig.report(result, rig.alternate({name: fn}, calls, args.windows, 20), key="accumulate_{name}_alone_ms", digits=5)
        result[f"accumulate_{name}_bytes"] = per_param * numel
        result[f"accumulate_{name}_gbps"] = round(per_param * numel / (result[f"accumulate_{name}_alone_ms"] * 1e-3) / 1e9, 1)
    param, moments, hyper = on.flat.flat_param.clone(), [torch.zeros_like(grad) for _ in range(2)], on.optimizer._hyper_dev.clone()
    adam = lambda i: _lib.launch("mpa_adam_step_dev", dev, param, grad, moments[0], moments[1], numel, hyper, 0.9, 0.999,  # noqa: E731
                                 1e-8, 0.0, 0, None)
    rig.report(result, rig.alternate({"adam_step_dev": adam}, calls, args.windows, 20), key="{name}_alone_ms", digits=5)
    rig.emit(result, args.out)


if __name__ == "__main__":
    main()
