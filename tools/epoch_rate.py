"""What the device-side epoch order and the device-index geometry batches cost and buy.  One JSON line (also written to --out):

  order.S<S>_ms              one `mpa_epoch_order` call (keys + counting ranks) at S = 1 000, 40 000 and the maximum 2^18:
                             `--order-reps` calls between two HIP events, per call
  batch.host_idx_ms          DeviceGeometryProducer.batch(list): slot table in numpy, one pinned copy, one launch
  batch.device_idx_ms        DeviceGeometryProducer.batch(device int64 vector): two launches, no host table
  epoch.fit_ms               per step of an epoch of the c2 model (pn_transformer_everyday, B = 32, P = 20, N = 1000) on a
                             synthetic store, driven by `Trainer.fit` with an `EpochSampler`
  epoch.hand_ms              the same steps driven by hand: `np.random.permutation` on the host, Python index lists into the
                             producer, `loss.item()` after every step

The batch and epoch arms are host clocks around windows that end in a device synchronise, divided by the calls in the window;
the arms of a group run in alternating windows after a warm-up of every arm, and the median of the windows is reported with
the windows beside it (the protocol of tools/rate_rig.py).

GPU only:  python tools/epoch_rate.py [--windows 5] [--batches 100] [--shapes 256] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_rig as rig  # noqa: E402  (puts the repository root on sys.path)
from multi_part_assembly_amd import _lib, config, datasets, sampler_ref, synthetic  # noqa: E402
from multi_part_assembly_amd.pn_transformer import build_model  # noqa: E402
from multi_part_assembly_amd.sampler import EpochSampler  # noqa: E402
from multi_part_assembly_amd.trainer import Trainer  # noqa: E402

B, P, N = 32, 20, 1000


def order_ms(dev, S, reps, windows):
    out = torch.empty(S, dtype=torch.int64, device=dev)
    ws = torch.empty(_lib.query("mpa_epoch_order_workspace", S) // 8, dtype=torch.int64, device=dev)
    call = lambda e: _lib.launch("mpa_epoch_order", dev, S, 1, 0, 1234, e, None, ws, out)  # noqa: E731
    call(0)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for w in range(windows):
        start.record()
        for i in range(reps):
            call(1 + w * reps + i)
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop) / reps)
    return statistics.median(times), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batches", type=int, default=100, help="producer calls per window")
    ap.add_argument("--order-reps", type=int, default=5, help="mpa_epoch_order calls per window")
    ap.add_argument("--shapes", type=int, default=256, help="shapes in the synthetic store (an epoch: shapes // 32 steps)")
    ap.add_argument("--faces", type=int, default=2000)
    ap.add_argument("--epochs", type=int, default=5, help="epochs per window of the fit / hand arms")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    rig.require_gpu("epoch_rate")
    dev = torch.device("cuda:0")
    out = {"tool": "epoch_rate", "device": torch.cuda.get_device_name(0), "B": B, "P": P, "N": N, "shapes": args.shapes,
           "faces_per_part": args.faces, "windows": args.windows, "calls_per_window": args.batches, "order": {}}

    # ---- (a) the order of an epoch ----
    for S in (1000, 40000, sampler_ref.MAX_SHAPES):
        rig.report(out, {f"S{S}": order_ms(dev, S, args.order_reps, args.windows)}, group="order")

    # ---- (b) a geometry batch from host indices and from device indices ----
    counts = np.random.RandomState(args.seed).randint(2, P + 1, size=args.shapes).tolist()
    store = datasets.MeshStore.from_arrays(synthetic.make_fracture_meshes(args.seed, args.shapes, counts, args.faces), 2, P)
    prod = datasets.DeviceGeometryProducer(store, num_points=N, max_num_part=P, seed=args.seed, device=dev)
    rng = np.random.RandomState(args.seed)
    index_lists = [rng.permutation(len(store))[:B].tolist() for _ in range(64)]
    index_tensors = [torch.tensor(ix, dtype=torch.int64, device=dev) for ix in index_lists]
    arms = {"host_idx": lambda i: prod.batch(index_lists[i % 64], batch_counter=i),
            "device_idx": lambda i: prod.batch(index_tensors[i % 64], batch_counter=i)}
    rig.report(out, rig.alternate(arms, args.batches, args.windows, 10), group="batch")
    prod.check()

    # ---- (c) an epoch of c2 steps: fit against the hand-written loop ----
    cfg = config.pn_transformer_everyday()
    trainers = {}
    for arm in ("fit", "hand"):
        torch.manual_seed(0)
        trainers[arm] = Trainer(build_model(cfg).to(dev), cfg)
    sampler = EpochSampler(len(store), B, seed=args.seed, device=dev)
    steps = len(sampler)

    def fit_epoch(i):
        trainers["fit"].fit(prod, sampler, epochs=1, log_every=50)

    def hand_epoch(i):
        trainers["hand"].set_epoch(0)
        order = np.random.permutation(len(store))
        for k in range(steps):
            loss = trainers["hand"].train_step(prod.batch(order[k * B:(k + 1) * B].tolist()))
            trainers["hand"].check_health()
            loss.item()

    result = rig.alternate({"fit": fit_epoch, "hand": hand_epoch}, args.epochs, args.windows, 1)
    out["epoch"] = {"steps": steps, "epochs_per_window": args.epochs}
    per_step = {arm: (med / steps, [t / steps for t in ts]) for arm, (med, ts) in result.items()}  # a call is an epoch
    rig.report(out, per_step, group="epoch")
    for t in trainers.values():
        t.check_health(synchronize=True)
    rig.emit(out, args.out)


if __name__ == "__main__":
    main()
