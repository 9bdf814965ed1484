"""Cost of the guarded optimiser step (`Trainer(guard_step=True)`: csrc/adam.hip mpa_step_guard + mpa_adam_step_guarded)
and of its buffer rollback (`guard_buffers=True`: mpa_guard_commit on the model's buffer slab) on the c2 configuration: pn_transformer, everyday preset, B = 32, P = 20, N = 1000, part counts of
`bench.representative_parts`.  One JSON line:

  arms                  guard off / on / rollback (on + guard_buffers)  x  eager / captured (use_graph)  x  clip_grad
                        off / on: twelve trainers in ONE process, alternating windows after a warm-up (the captured arms
                        warm up past their capture)
  *_ms                  ms per `train_step`: a host clock around a window of steps that ends in a device synchronise,
                        divided by its steps; the median of the windows, with the windows beside it (`*_ms_windows`)
  *_optimizer_launches  kernels the optimiser's library calls of one step launch (recorded entry points x the kernels
                        each launches: grad_clip_coef 2, adam_step_dev 2, step_guard 2, adam_step_guarded 1,
                        guard_commit 1)
  step_guard_alone_ms   mpa_step_guard alone at the model's numel (back-to-back calls between synchronises);
                        grad_clip_coef_alone_ms, adam_step_dev_alone_ms likewise, for scale
  guard_commit_alone_ms mpa_guard_commit alone on the c2 model's buffer slab, `slab_bytes` bytes (verdict word 0)
  rollback_minus_guard_on_ms  per (mode, clip): the rollback arm's median minus the guard-on arm's
  guard_off_spread_ms   max - min of the guard-off arm's windows, per (mode, clip): the yardstick's own noise

The yardstick of every guarded arm is the guard-off arm of the same (mode, clip) in the same run; the yardstick of a
rollback arm is the guard-on arm beside it.

GPU only:  python tools/guard_rate.py [--steps 30] [--windows 5] [--clip 1.0]"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multi_part_assembly_amd import _lib, config, synthetic  # noqa: E402
from multi_part_assembly_amd.pn_transformer import build_model  # noqa: E402
from multi_part_assembly_amd.trainer import Trainer  # noqa: E402

KERNELS = {"mpa_grad_clip_coef": 2, "mpa_adam_step_dev": 2, "mpa_step_guard": 2, "mpa_adam_step_guarded": 1,
           "mpa_guard_commit": 1}
GUARDS = ("off", "on", "rollback")


def representative_parts(seed):
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench.representative_parts("everyday", seed)


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def arm_name(guard, graph, clip):
    return f"guard_{guard}_{'graph' if graph else 'eager'}_{'clip' if clip else 'noclip'}"


def optimizer_launches(optimizer):
    """Kernels behind the library calls of one `step_dev` (recorded, nothing runs)."""
    names, real = [], _lib.launch
    _lib.launch = lambda name, dev, *a, **k: names.append(name)
    try:
        optimizer.step_dev()
    finally:
        _lib.launch = real
    return sum(KERNELS[n] for n in names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--clip", type=float, default=1.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, P, N = 32, 20, 1000
    batches = [{k: v for k, v in synthetic.make_batch(B, P, N, seed=1234 + i, device=dev,
                                                      num_parts=representative_parts(1234 + i)).items() if k != "num_parts"}
               for i in range(4)]
    arms = {}
    for clip in (False, True):
        for graph in (False, True):
            for guard in GUARDS:
                torch.manual_seed(0)
                cfg = config.pn_transformer_everyday()
                cfg.optimizer.clip_grad = args.clip if clip else None
                trainer = Trainer(build_model(cfg).to(dev), cfg, use_graph=graph, guard_step=guard != "off",
                                  guard_buffers=guard == "rollback")
                arms[(guard, graph, clip)] = trainer
    result = {"B": B, "P": P, "N": N, "steps_per_window": args.steps, "windows": args.windows, "clip_grad": args.clip,
              "numel": arms[("off", False, False)].flat.numel}

    def step(trainer):
        return lambda i: trainer.train_step(batches[i % len(batches)])

    for trainer in arms.values():  # warm-up: code objects, lazily built buffers, the capture (3 eager steps, then replays)
        window(step(trainer), 6)
    times = {key: [] for key in arms}
    for _ in range(args.windows):  # alternating windows in one process
        for key, trainer in arms.items():
            times[key].append(window(step(trainer), args.steps))
    for key, trainer in arms.items():
        name = arm_name(*key)
        result[f"{name}_ms"] = round(statistics.median(times[key]), 4)
        result[f"{name}_ms_windows"] = [round(t, 4) for t in times[key]]
        result[f"{name}_optimizer_launches"] = optimizer_launches(trainer.optimizer)
        if key[0] != "off":
            words = trainer.optimizer.guard_words().tolist()
            result[f"{name}_applied_skipped"] = words[1:3]
    result["guard_off_spread_ms"] = {arm_name(*k)[10:]: round(max(t) - min(t), 4) for k, t in times.items()
                                     if k[0] == "off"}
    result["rollback_minus_guard_on_ms"] = {
        arm_name(*k)[15:]: round(statistics.median(t) - statistics.median(times[("on",) + k[1:]]), 4)
        for k, t in times.items() if k[0] == "rollback"}

    # the guard's two launches alone, at the model's numel
    opt = arms[("on", False, True)].optimizer
    plain = arms[("off", False, True)].optimizer
    calls = 200

    def guard_alone(i):
        _lib.launch("mpa_step_guard", dev, opt.flat_grad, opt.numel, float(args.clip), opt._hyper_dev.data_ptr() + 12, 1.0,
                    opt.launch_status, opt.guard_workspace(), opt._hyper_dev, opt.guard_words(), 0.9, 0.999)

    def clip_alone(i):
        _lib.launch("mpa_grad_clip_coef", dev, plain.flat_grad, plain.numel, float(args.clip),
                    plain._hyper_dev.data_ptr() + 12, 1.0, plain._clip_ws, plain._hyper_dev.data_ptr() + 20)

    scratch = [torch.zeros_like(plain.flat_param) for _ in range(3)]
    hyper = plain._hyper_dev.clone()

    def adam_alone(i):
        _lib.launch("mpa_adam_step_dev", dev, scratch[0], plain.flat_grad, scratch[1], scratch[2], plain.numel, hyper, 0.9,
                    0.999, 1e-8, 0.0, 0, None)

    # the commit alone, on slabs of the c2 model's size (a trainer's own slab keeps its statistics)
    slab = arms[("rollback", False, True)].buffer_slab
    result["slab_bytes"], result["slab_buffers"] = slab.nbytes, len(slab.names)
    live, shadow = slab.live.clone(), slab.shadow.clone()
    applied = torch.zeros(8, dtype=torch.int32, device=dev)

    def commit_alone(i):
        _lib.launch("mpa_guard_commit", dev, applied, live, shadow, slab.nbytes)

    for name, fn in (("step_guard", guard_alone), ("grad_clip_coef", clip_alone), ("adam_step_dev", adam_alone),
                     ("guard_commit", commit_alone)):
        window(fn, 20)
        ws = [window(fn, calls) for _ in range(args.windows)]
        result[f"{name}_alone_ms"] = round(statistics.median(ws), 5)
        result[f"{name}_alone_ms_windows"] = [round(t, 5) for t in ws]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
