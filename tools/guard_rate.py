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
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_rig as rig  # noqa: E402  (puts the repository root on sys.path)
from multi_part_assembly_amd import _lib, config  # noqa: E402
from multi_part_assembly_amd.pn_transformer import build_model  # noqa: E402
from multi_part_assembly_amd.trainer import Trainer  # noqa: E402

KERNELS = {"mpa_grad_clip_coef": 2, "mpa_adam_step_dev": 2, "mpa_step_guard": 2, "mpa_adam_step_guarded": 1,
           "mpa_guard_commit": 1}
GUARDS = ("off", "on", "rollback")


def arm_name(guard, graph, clip):
    return f"guard_{guard}_{'graph' if graph else 'eager'}_{'clip' if clip else 'noclip'}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--clip", type=float, default=1.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, P, N = 32, 20, 1000
    batches = rig.c2_batches(dev, 4, B=B, P=P, N=N)
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

    # warm-up of 6: code objects, lazily built buffers, the capture (3 eager steps, then replays)
    timed = rig.alternate({key: step(trainer) for key, trainer in arms.items()}, args.steps, args.windows, 6)
    rig.report(result, {arm_name(*key): v for key, v in timed.items()})
    for key, trainer in arms.items():
        name = arm_name(*key)
        # kernels behind the library calls of one `step_dev`
        result[f"{name}_optimizer_launches"] = sum(KERNELS[n] for n in rig.recorded_launches(trainer.optimizer.step_dev))
        if key[0] != "off":
            words = trainer.optimizer.guard_words().tolist()
            result[f"{name}_applied_skipped"] = words[1:3]
    result["guard_off_spread_ms"] = {arm_name(*k)[10:]: round(max(ts) - min(ts), 4) for k, (_, ts) in timed.items()
                                     if k[0] == "off"}
    result["rollback_minus_guard_on_ms"] = {arm_name(*k)[15:]: round(med - timed[("on",) + k[1:]][0], 4)
                                            for k, (med, _) in timed.items() if k[0] == "rollback"}

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
        rig.report(result, rig.alternate({name: fn}, calls, args.windows, 20), key="{name}_alone_ms", digits=5)
    rig.emit(result, None)


if __name__ == "__main__":
    main()
