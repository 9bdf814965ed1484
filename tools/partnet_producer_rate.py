"""Cost of a PartNet batch on the host path and on the device path, next to the captured semantic step it feeds
(B = 32, P = 20, N = 1000, shapes of `synthetic.make_partnet_like_store`).  One JSON line (also written to --out):

  producer.host_ms           PartNetBatchProducer.batch: the store written to a temporary folder in the reference's format,
                             so every batch loads its 2 x B files, builds the labels in Python and copies key by key
  producer.device_ms         DevicePartNetProducer.batch(list): one pinned copy of the indices + one launch
  producer.device_idx_ms     DevicePartNetProducer.batch(device int64 tensor): the launch alone
  step.<model>.alone_ms      the captured step (Trainer(use_graph=True), match_sample = "device") replaying on its static batch
  step.<model>.host_fed_ms   host producer + step in one loop (the step copies every key into its static batch)
  step.<model>.device_fed_ms DevicePartNetProducer.batch(device indices, out=trainer.static_batch) + step in one loop
  gather.event_ms            the gather kernel's own time: 50 launches (50 index sets, fixed outputs) captured into one
                             graph, ten replays between two HIP events, per launch; with the bytes a launch moves by the
                             formula in gather.traffic_formula, and their ratio

Every other *_ms is the median of the arm's windows, the windows themselves beside it: the arms of a group run in
alternating windows after a warm-up of every arm (captures included), the protocol of tools/rate_rig.py.  Another set of
indices every batch.

GPU only:  python tools/partnet_producer_rate.py [--windows 5] [--batches 100] [--host-batches 10] [--out FILE]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_rig as rig  # noqa: E402  (puts the repository root on sys.path)
from multi_part_assembly_amd import config, datasets, synthetic  # noqa: E402
from multi_part_assembly_amd.pn_transformer import build_model  # noqa: E402
from multi_part_assembly_amd.trainer import Trainer  # noqa: E402

PRESETS = {"global": config.global_partnet_chair, "dgl": config.dgl_partnet_chair}
B, P, N = 32, 20, 1000
REPS = 50  # gather launches in the graph that gather.event_ms times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batches", type=int, default=100, help="calls per device / step window")
    ap.add_argument("--host-batches", type=int, default=10, help="calls per window of an arm with the host producer in it")
    ap.add_argument("--shapes", type=int, default=512, help="shapes in the store")
    ap.add_argument("--models", default="dgl,global")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    rig.require_gpu("partnet_producer_rate")
    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    store = synthetic.make_partnet_like_store(args.shapes, max_parts=P, num_points=N, seed=args.seed)
    make_s = time.perf_counter() - t0
    rng = np.random.RandomState(args.seed)
    index_lists = [rng.permutation(len(store))[:B].tolist() for _ in range(64)]
    index_tensors = [torch.tensor(ix, dtype=torch.int64, device=dev) for ix in index_lists]
    pick = lambda seq, i: seq[i % len(seq)]
    counts = np.diff(store.shape_part_off)
    valid = float(np.mean([counts[ix].sum() for ix in index_lists]))
    pairs = float(np.mean([(counts[ix] ** 2).sum() for ix in index_lists]))
    out = {"tool": "partnet_producer_rate", "device": torch.cuda.get_device_name(0), "B": B, "P": P, "N": N,
           "shapes": len(store), "store_bytes": int(store.nbytes), "store_make_s": round(make_s, 3),
           "valid_parts_per_batch": round(valid, 1), "windows": args.windows, "calls_per_window": args.batches,
           "host_calls_per_window": args.host_batches}

    with tempfile.TemporaryDirectory() as tmp:
        synthetic.write_partnet_folder(store, tmp)
        keys = tuple(config.dgl_partnet_chair().data.data_keys)
        host = datasets.PartNetBatchProducer(tmp, "Chair.train.npy", keys, max_num_part=P, device=dev)
        device = datasets.DevicePartNetProducer(store, keys, max_num_part=P, device=dev)
        out["data_keys"] = list(keys)

        # ---- the producers alone ----
        arms = {"host": lambda i: host.batch(pick(index_lists, i)),
                "device": lambda i: device.batch(pick(index_lists, i)),
                "device_idx": lambda i: device.batch(pick(index_tensors, i))}
        calls = {"host": args.host_batches, "device": args.batches, "device_idx": args.batches}
        rig.report(out, rig.alternate(arms, calls, args.windows, {"host": 2, "device": 10, "device_idx": 10}), group="producer")
        out["producer"]["device_below_host"] = out["producer"]["device_ms"] < out["producer"]["host_ms"]

        # ---- the gather launch between two events, against the bytes it moves ----
        fixed = device.batch(index_tensors[0])
        fixed.pop("data_id")
        # REPS launches captured into one graph: between the two events there is no host launch cost, only the kernels
        for i in range(3):
            device.batch(index_tensors[0], out=fixed)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            for i in range(REPS):
                device.batch(index_tensors[i], out=fixed)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        event_ms = []
        for w in range(args.windows):
            graph.replay()
            torch.cuda.synchronize()
            start.record()
            for i in range(10):
                graph.replay()
            stop.record()
            torch.cuda.synchronize()
            event_ms.append(start.elapsed_time(stop) / (10 * REPS))
        per_part = 12 * N + 28 + 12 * ("sym" in keys)  # cloud, pose (7 floats), sym (3 floats)
        slot_labels = 1 + ("part_ids" in keys) + ("match_ids" in keys)  # part_valids and the per-slot label vectors
        written = B * P * per_part + B * (8 + 4 * P * slot_labels + 4 * P * P * (1 + ("valid_matrix" in keys))
                                          + 16 * P * P * ("contact_points" in keys))
        read = valid * (per_part + 4) + 16 * pairs * ("contact_points" in keys) + 24 * B
        med = statistics.median(event_ms)
        out["gather"] = {"event_ms": round(med, 5), "event_ms_windows": [round(t, 5) for t in event_ms],
                         "bytes_read": int(read), "bytes_written": int(written),
                         "traffic_formula": "read = valid_parts * (12 N + 28 pose + 12 sym + 4 geo id) + 16 * sum p^2 (contacts) "
                                            "+ 24 B (index, offsets); written = B P (12 N + 28 + 12 sym) + B * (8 shape_id + 4 P * "
                                            "[part_valids, part_ids, match_ids] + 4 P^2 * [instance_label, valid_matrix] + "
                                            "16 P^2 contact_points); requested keys only",
                         "GB_per_s": round((read + written) / (med * 1e-3) / 1e9, 1)}
        device.check()

        # ---- the captured step fed by each producer ----
        out["step"] = {}
        for name in [m for m in args.models.split(",") if m]:
            cfg = PRESETS[name]()
            cfg.loss.match_sample = "device"
            cfg.data.max_num_part = P
            mkeys = tuple(cfg.data.data_keys)
            m_host = datasets.PartNetBatchProducer(tmp, "Chair.train.npy", mkeys, max_num_part=P, device=dev)
            m_dev = datasets.DevicePartNetProducer(store, mkeys, max_num_part=P, device=dev)
            trainers = {}
            for arm in ("alone", "host_fed", "device_fed"):
                torch.manual_seed(0)
                trainers[arm] = Trainer(build_model(cfg).to(dev), cfg, use_graph=True, graph_warmup=2)
            for i in range(4):  # every trainer captures on the kind of batch it will be fed
                trainers["host_fed"].train_step(m_host.batch(pick(index_lists, i)))
                for arm in ("alone", "device_fed"):
                    trainers[arm].train_step(m_dev.batch(pick(index_tensors, i)))
            assert all(t._graph is not None for t in trainers.values())
            static = {arm: {k: v for k, v in trainers[arm].static_batch.items() if k != "data_id"}
                      for arm in ("alone", "device_fed")}

            def device_fed(i):
                trainers["device_fed"].train_step(m_dev.batch(pick(index_tensors, i), out=static["device_fed"]))

            arms = {"alone": lambda i: trainers["alone"].train_step(static["alone"]),
                    "host_fed": lambda i: trainers["host_fed"].train_step(m_host.batch(pick(index_lists, i))),
                    "device_fed": device_fed}
            calls = {"alone": args.batches, "host_fed": args.host_batches, "device_fed": args.batches}
            out["step"][name] = {"data_keys": list(mkeys)}
            rig.report(out["step"], rig.alternate(arms, calls, args.windows, {"alone": 5, "host_fed": 2, "device_fed": 5}),
                       group=name)
            for t in trainers.values():
                t.check_health(synchronize=True)
            m_dev.check()
    rig.emit(out, args.out)


if __name__ == "__main__":
    main()
