"""Cost of the weight average (`Trainer(ema_decay=...)`: csrc/weight_average.hip mpa_ema_update as the last launch of
every optimiser step) on the c2 configuration: pn_transformer, everyday preset, B = 32, P = 20, N = 1000, part counts of
`bench.representative_parts`.  One JSON line, also written to `--out` (default profiles/r21_ema_rate.json):

  arms                 averaging off / on  x  eager / captured (use_graph): four trainers in ONE process, alternating
                       windows after a warm-up (the captured arms warm up past their capture)
  *_ms                 ms per `train_step`: a host clock around a window of steps that ends in a device synchronise,
                       divided by its steps; the median of the windows, with the windows beside it (`*_ms_windows`)
  *_optimizer_launches kernels the optimiser's library calls of one step launch (adam_step_dev 2, ema_update 1)
  ema_on_minus_off_ms  per mode: the averaging arm's median minus the off arm's (the parent's step, in the same run)
  ema_off_spread_ms    max - min of the off arm's windows, per mode: the yardstick's own noise
  ema_update_alone_ms  mpa_ema_update alone on the model's flat buffer and slab (back-to-back calls between synchronises);
                       ema_swap_alone_ms and adam_step_dev_alone_ms likewise, on the same flat buffer
  ema_update_bytes     bytes mpa_ema_update moves per call (12 per parameter, 48 per 16-byte slab unit at most), and
                       ema_update_gbps from the median
  peak_memory_*        torch.cuda.max_memory_allocated() after building and stepping an off / an on trainer alone, and
                       what the average holds (`average_bytes` = one flat buffer + one slab)

GPU only:  python tools/ema_rate.py [--steps 30] [--windows 5] [--decay 0.999]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_rig as rig  # noqa: E402  (puts the repository root on sys.path)
from multi_part_assembly_amd import _lib, config  # noqa: E402
from multi_part_assembly_amd.pn_transformer import build_model  # noqa: E402
from multi_part_assembly_amd.trainer import Trainer  # noqa: E402

KERNELS = {"mpa_grad_clip_coef": 2, "mpa_adam_step_dev": 2, "mpa_ema_update": 1}


def arm_name(ema, graph):
    return f"ema_{'on' if ema else 'off'}_{'graph' if graph else 'eager'}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--decay", type=float, default=0.999, help="any value in [0, 1): the cost does not depend on it")
    ap.add_argument("--out", default=os.path.join(rig.ROOT, "profiles", "r21_ema_rate.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, P, N = 32, 20, 1000
    batches = rig.c2_batches(dev, 4, B=B, P=P, N=N)

    def make(ema, graph):
        torch.manual_seed(0)
        cfg = config.pn_transformer_everyday()
        return Trainer(build_model(cfg).to(dev), cfg, use_graph=graph, ema_decay=args.decay if ema else None)

    def step(trainer):
        return lambda i: trainer.train_step(batches[i % len(batches)])

    result = {"B": B, "P": P, "N": N, "steps_per_window": args.steps, "windows": args.windows, "decay": args.decay}
    # peak memory of one trainer alone, off then on, before anything else lives on the device
    for ema in (False, True):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        trainer = make(ema, False)
        rig.window(step(trainer), 3)
        result[f"peak_memory_{'on' if ema else 'off'}_bytes"] = torch.cuda.max_memory_allocated(dev) - base
        if ema:
            result["average_bytes"] = trainer.average.ema_param.numel() * 4 + trainer.average.ema_state.numel()
        del trainer
    result["peak_memory_on_minus_off_bytes"] = result["peak_memory_on_bytes"] - result["peak_memory_off_bytes"]

    arms = {(ema, graph): make(ema, graph) for graph in (False, True) for ema in (False, True)}
    result["numel"] = arms[(True, False)].flat.numel
    # warm-up of 6: code objects, lazily built buffers, the capture (3 eager steps, then replays)
    timed = rig.alternate({key: step(trainer) for key, trainer in arms.items()}, args.steps, args.windows, 6)
    rig.report(result, {arm_name(*key): v for key, v in timed.items()})
    for key, trainer in arms.items():  # kernels behind the library calls of one `step_dev`
        names = rig.recorded_launches(trainer.optimizer.step_dev)
        result[f"{arm_name(*key)}_optimizer_launches"] = sum(KERNELS[n] for n in names)
    result["ema_off_spread_ms"] = {arm_name(*k)[8:]: round(max(ts) - min(ts), 4) for k, (_, ts) in timed.items() if not k[0]}
    result["ema_on_minus_off_ms"] = {arm_name(*k)[7:]: round(med - timed[(False, k[1])][0], 4)
                                     for k, (med, _) in timed.items() if k[0]}

    # the three kernels alone, on the model's own flat buffer (copies: a trainer's weights stay what they are)
    on = arms[(True, False)]
    opt, avg, slab = on.optimizer, on.average, on.buffer_slab
    result["slab_bytes"], result["slab_buffers"] = slab.nbytes, len(slab.names)
    param, ema_param = on.flat.flat_param.clone(), avg.ema_param.clone()
    live, ema_state = slab.live.clone(), avg.ema_state.clone()
    hyper = opt._hyper_dev.clone()
    moments = [torch.zeros_like(param) for _ in range(2)]
    calls = 200

    def update_alone(i):
        _lib.launch("mpa_ema_update", dev, param, ema_param, on.flat.numel, live, ema_state, slab.nbytes, avg._table_host,
                    avg._table_dev, len(avg.segments), hyper, args.decay, 1, None)

    def swap_alone(i):
        _lib.launch("mpa_ema_swap", dev, param, ema_param, on.flat.numel * 4, live, ema_state, slab.nbytes)

    def adam_alone(i):
        _lib.launch("mpa_adam_step_dev", dev, param, on.flat.flat_grad, moments[0], moments[1], on.flat.numel, hyper, 0.9,
                    0.999, 1e-8, 0.0, 0, None)

    for name, fn in (("ema_update", update_alone), ("ema_swap", swap_alone), ("adam_step_dev", adam_alone)):
        rig.report(result, rig.alternate({name: fn}, calls, args.windows, 20), key="{name}_alone_ms", digits=5)
    result["ema_update_bytes"] = 12 * on.flat.numel + 3 * slab.nbytes
    result["ema_update_gbps"] = round(result["ema_update_bytes"] / (result["ema_update_alone_ms"] * 1e-3) / 1e9, 1)
    result["ema_update_not_slower_than_adam"] = result["ema_update_alone_ms"] <= result["adam_step_dev_alone_ms"]
    rig.emit(result, args.out)


if __name__ == "__main__":
    main()
