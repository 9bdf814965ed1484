"""B-LSTM training step (everyday preset, B = 32, P = 20, N = 1000) on the HIP path and on the library path of the
seq2seq module, alternating in one process and timed with device events; prints the aten-op and kernel-launch counts
of one step of each.  GPU only:  python tools/lstm_step.py [--steps 20]"""
import argparse
import os
import sys
import warnings

import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-counts", action="store_true", help="skip the op / launch counts (under an outside profiler)")
    ap.add_argument("--paths", default="hip,library", help="comma-separated subset of hip,library")
    args = ap.parse_args()
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
