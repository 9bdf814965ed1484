"""Cost of a geometry batch on the host path and on the device path, next to the training step it feeds (c2:
pn_transformer, everyday preset, B = 32, P = 20, N = 1000, part counts of `bench.representative_parts`).  One JSON line:

  a_host_obj_ms       GeometryBatchProducer.batch + ObjSurfaceSampler on .obj files written to a temporary folder
  b_host_parsed_ms    the same with the meshes already parsed (sampling, rotation, shuffle on the host)
  c_device_ms         DeviceGeometryProducer.batch on a MeshStore of the same meshes
  d_step_ms           Trainer.train_step alone, on one device-produced batch
  e_device_and_step_ms  DeviceGeometryProducer.batch + train_step in one loop

Every figure is a host clock around a window that ends in a device synchronise, after a warm-up, divided by the number
of batches in the window.  GPU only:  python tools/geometry_producer_rate.py [--batches 200] [--host-batches 1]"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multi_part_assembly_amd import config, datasets, synthetic  # noqa: E402
from multi_part_assembly_amd.pn_transformer import build_model  # noqa: E402
from multi_part_assembly_amd.trainer import Trainer  # noqa: E402


def representative_parts(seed):
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench.representative_parts("everyday", seed)


def write_obj_folders(root, shapes):
    data_list = []
    for s, parts in enumerate(shapes):
        rel = os.path.join(f"shape_{s:03d}", "fractured_0")
        os.makedirs(os.path.join(root, rel))
        for k, (v, f) in enumerate(parts):
            with open(os.path.join(root, rel, f"piece_{k:02d}.obj"), "w") as fh:
                fh.writelines("v %r %r %r\n" % tuple(p) for p in v.tolist())
                fh.writelines("f %d %d %d\n" % tuple(t) for t in (f + 1).tolist())
        data_list.append(rel)
    return data_list


def window(fn, batches, warmup):
    """ms per call of fn(i) over `batches` calls, the window closed by a synchronise."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(batches):
        fn(warmup + i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / batches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=200, help="batches per device window")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-batches", type=int, default=1,
                    help="batches per host window (about 11 s each with parsing); 0 skips the host path")
    ap.add_argument("--faces", type=int, default=5000, help="triangles per part")
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geometry_producer_rate: needs a GPU (a host timing says nothing about the device path)")
    dev = torch.device("cuda:0")
    cfg = config.pn_transformer_everyday()
    B, P, N = 32, cfg.data.max_num_part, cfg.data.num_pc_points
    parts = representative_parts(args.seed)
    shapes = synthetic.make_fracture_meshes(args.seed, B, parts, args.faces)
    indices = list(range(B))

    t0 = time.perf_counter()
    store = datasets.MeshStore.from_arrays(shapes)
    pack_s = time.perf_counter() - t0
    device = datasets.DeviceGeometryProducer(store, num_points=N, max_num_part=P, data_keys=cfg.data.data_keys,
                                             seed=args.seed, device=dev)
    torch.manual_seed(0)
    trainer = Trainer(build_model(cfg).to(dev), cfg)
    fixed = device.batch(indices)

    a_ms = b_ms = None
    if args.host_batches > 0:
        with tempfile.TemporaryDirectory() as tmp:
            data_list = write_obj_folders(tmp, shapes)
            np.random.seed(args.seed)
            host_obj = datasets.GeometryBatchProducer(
                num_points=N, max_num_part=P, data_keys=cfg.data.data_keys, device=dev, data_list=data_list,
                sampler=datasets.ObjSurfaceSampler(tmp, num_points=N, max_num_part=P))
            a_ms = window(lambda i: host_obj.batch(indices), args.host_batches, 0)
        parsed = dict(zip(data_list, shapes))
        host_parsed = datasets.GeometryBatchProducer(
            num_points=N, max_num_part=P, data_keys=cfg.data.data_keys, device=dev, data_list=data_list,
            sampler=lambda rel: np.stack([datasets.sample_surface(v, f, N) for v, f in parsed[rel]]))
        b_ms = window(lambda i: host_parsed.batch(indices), args.host_batches, 0)

    c_ms = window(lambda i: device.batch(indices), args.batches, args.warmup)
    d_ms = window(lambda i: trainer.train_step(fixed), args.batches, args.warmup)
    e_ms = window(lambda i: trainer.train_step(device.batch(indices)), args.batches, args.warmup)
    c2_ms = window(lambda i: device.batch(indices), args.batches, args.warmup)  # again: the spread of (c)
    trainer.check_health(synchronize=True)
    print(json.dumps({
        "tool": "geometry_producer_rate", "device": torch.cuda.get_device_name(0), "B": B, "P": P, "N": N,
        "valid_parts": int(sum(parts)), "faces_per_part": int(store.part_face_off[1]), "store_bytes": int(store.nbytes),
        "store_pack_s": round(pack_s, 3), "batches": args.batches, "host_batches": args.host_batches,
        "a_host_obj_ms": a_ms and round(a_ms, 1), "b_host_parsed_ms": b_ms and round(b_ms, 1), "c_device_ms": round(c_ms, 4),
        "c_device_ms_repeat": round(c2_ms, 4), "d_step_ms": round(d_ms, 4), "e_device_and_step_ms": round(e_ms, 4),
        "launch": "eager"}))


if __name__ == "__main__":
    main()
