"""B-LSTM training step (everyday preset, B = 32, P = 20, N = 1000) on the HIP path and on the library path of the
seq2seq module, alternating in one process and timed with device events; prints the aten-op and kernel-launch counts
of one step of each.  GPU only:  python tools/lstm_step.py [--steps 20]

`--draws` instead measures where the per-forward draws come from (one JSON line, profiles/r15_lstm_step_rate.json):

  models   lstm_everyday on `synthetic.make_batch`, lstm_partnet_chair on `make_partnet_like_batch` (its matching draws on
           the device in every arm: `cfg.loss.match_sample = "device"`), both at B = 32, P = 20, N = 1000
  arms     a  coin, noise and masks from the host generators, eager launches — the path of `lstm_draws = "host"`
           b  cfg.model.lstm_draws = "device" (csrc/seq2seq_draw.hip + the coin read by the decoder launch), eager
           c  arm b captured as one HIP graph (Trainer(use_graph=True))
  *_ms     ms per `Trainer.train_step`: a host clock around a window of steps that ends in a device synchronise; the arms
           run in ONE process in alternating windows after a warm-up of every arm (the capture included); the median of
           the windows, the windows themselves beside it; spread_a = max - min of arm a's windows, the margin of
           `b_not_slower` (b_ms <= a_ms + spread_a)
  draw_us  device time of one `mpa_seq2seq_draw` kernel at B = 32, T = 20 with a mask (the profiler's kernel records)
  launches_fwd_a / _b   kernel launches of one training-mode seq2seq forward (profiler count), host and device draws

  python tools/lstm_step.py --draws [--steps 10] [--windows 5] [--models everyday,partnet] [--arms a,b,c]"""
import argparse
import os
import sys
import warnings

import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_rig as rig  # noqa: E402  (puts the repository root on sys.path)
from multi_part_assembly_amd import config, synthetic  # noqa: E402
from multi_part_assembly_amd.pn_transformer import build_model  # noqa: E402
from multi_part_assembly_amd.trainer import Trainer  # noqa: E402


class OpCount(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


DRAW_PRESETS = {"everyday": config.lstm_everyday, "partnet": config.lstm_partnet_chair}


def _draws_arm(name, arm, dev, P):
    cfg = DRAW_PRESETS[name]()
    cfg.data.max_num_part = P
    if cfg.data.dataset != "geometry":
        cfg.loss.match_sample = "device"
    if arm != "a":
        cfg.model.lstm_draws = "device"
    torch.manual_seed(0)
    return Trainer(build_model(cfg).to(dev), cfg, use_graph=arm == "c", graph_warmup=2)


def _forward_launches(trainer, batch):
    """Kernel launches of one training-mode seq2seq forward on the trainer's model."""
    model = trainer.model.train()
    P = batch["part_valids"].shape[1]
    x = torch.randn(P, batch["part_valids"].shape[0], 128, device=batch["part_valids"].device)
    with torch.no_grad():
        model.seq2seq(x, x, valids=batch["part_valids"])
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            model.seq2seq(x, x, valids=batch["part_valids"])
            torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


def _draw_us(dev, B, P, reps=50):
    """Device time of one draw kernel, from the profiler's kernel records (events around back-to-back launches would
    measure the host's launch rate: the kernel is shorter than a launch)."""
    from multi_part_assembly_amd import lstm
    for _ in range(10):
        lstm.draw(B, P, 0.2, 0.5, True, seed=1, counter=1, device=dev)
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        for k in range(reps):
            lstm.draw(B, P, 0.2, 0.5, True, seed=1, counter=k, device=dev)
        torch.cuda.synchronize()
    rows = [e for e in prof.key_averages() if "seq2seq_draw" in e.key]
    total = sum(getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0) for e in rows)
    count = sum(e.count for e in rows)
    return total / max(count, 1)


def measure_draws(name, dev, args):
    B, P, N = 32, 20, 1000
    if name == "partnet":
        batches = [synthetic.make_partnet_like_batch(B, P, N, seed=1234 + i, device=dev) for i in range(2)]
    else:
        batches = [synthetic.make_batch(B, P, N, seed=1234 + i, device=dev) for i in range(2)]
    for b in batches:
        b.pop("num_parts", None)
    trainers = {arm: _draws_arm(name, arm, dev, P) for arm in args.arms}

    def step(tr):
        return lambda i: tr.train_step(batches[i % len(batches)], i)

    # warm-up of every arm: first launches, allocator, the capture of arm c
    timed = rig.alternate({arm: step(tr) for arm, tr in trainers.items()}, args.steps, args.windows, 4)
    out = {"B": B, "P": P, "N": N, "steps_per_window": args.steps, "sample_iter": trainers[args.arms[0]].model.sample_iter}
    rig.report(out, timed)
    if "c" in trainers:
        out["c_captured"] = trainers["c"]._graph is not None
    if "a" in timed:
        out["spread_a"] = round(max(timed["a"][1]) - min(timed["a"][1]), 4)
        if "b" in timed:
            out["b_not_slower"] = out["b_ms"] <= out["a_ms"] + out["spread_a"]
    for arm in ("a", "b"):
        if arm in trainers:
            out[f"launches_fwd_{arm}"] = _forward_launches(trainers[arm], batches[0])
    for tr in trainers.values():
        tr.check_health(synchronize=True)
    return out


def main_draws(args):
    dev = torch.device("cuda:0")
    warnings.simplefilter("ignore")
    args.arms = [a for a in args.arms.split(",") if a]
    result = {"windows": args.windows}
    for name in args.models.split(","):
        result[name] = measure_draws(name, dev, args)
    result["draw_us"] = round(_draw_us(dev, 32, 20), 3)
    rig.emit(result, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", action="store_true", help="time host draws / device draws / device draws captured")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--models", default="everyday,partnet")
    ap.add_argument("--arms", default="a,b,c")
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-counts", action="store_true", help="skip the op / launch counts (under an outside profiler)")
    ap.add_argument("--paths", default="hip,library", help="comma-separated subset of hip,library")
    args = ap.parse_args()
    rig.require_gpu("lstm_step")
    if args.draws:
        args.steps = 10 if args.steps is None else args.steps
        return main_draws(args)
    args.steps = 20 if args.steps is None else args.steps
    dev = torch.device("cuda:0")
    warnings.simplefilter("ignore")
    cfg = config.lstm_everyday()
    torch.manual_seed(0)
    model = build_model(cfg).to(dev)
    trainer = Trainer(model, cfg)
    batch = synthetic.make_batch(32, 20, 1000, seed=1234, device=dev)
    paths = {p: v for p, v in {"hip": None, "library": False}.items() if p in args.paths.split(",")}

    def step(path):
        model.seq2seq.hip = paths[path]
        trainer.train_step(batch)

    for _ in range(args.warmup):
        for p in paths:
            step(p)
    torch.cuda.synchronize()
    times = {p: [] for p in paths}
    for _ in range(args.steps):
        for p in paths:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(p)
            e1.record()
            torch.cuda.synchronize()
            times[p].append(e0.elapsed_time(e1))
    trainer.check_health(synchronize=True)
    for p in paths:
        t = sorted(times[p])
        if args.no_counts:
            print(f"{p:8s} step median {t[len(t) // 2]:.3f} ms  min {t[0]:.3f} ms  ({len(t)} steps)")
            continue
        with OpCount() as c:
            step(p)
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            step(p)
            torch.cuda.synchronize()
        launches = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
        print(f"{p:8s} step median {t[len(t) // 2]:.3f} ms  min {t[0]:.3f} ms  ({len(t)} steps)  aten ops/step {c.n}  "
              f"kernel launches/step {launches}")
    model.seq2seq.hip = None


if __name__ == "__main__":
    main()
