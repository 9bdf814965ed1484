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
import os
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


def single(fn, batches, warmup):
    """ms per call of one window of `batches` calls of fn(i), after `warmup` untimed calls (a rig.alternate of one arm)."""
    return rig.alternate({"arm": fn}, batches, 1, warmup)["arm"][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=200, help="batches per device window")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-batches", type=int, default=1,
                    help="batches per host window (about 11 s each with parsing); 0 skips the host path")
    ap.add_argument("--faces", type=int, default=5000, help="triangles per part")
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()
    rig.require_gpu("geometry_producer_rate")
    dev = torch.device("cuda:0")
    cfg = config.pn_transformer_everyday()
    B, P, N = 32, cfg.data.max_num_part, cfg.data.num_pc_points
    parts = rig.representative_parts(args.seed)
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
            a_ms = single(lambda i: host_obj.batch(indices), args.host_batches, 0)
        parsed = dict(zip(data_list, shapes))
        host_parsed = datasets.GeometryBatchProducer(
            num_points=N, max_num_part=P, data_keys=cfg.data.data_keys, device=dev, data_list=data_list,
            sampler=lambda rel: np.stack([datasets.sample_surface(v, f, N) for v, f in parsed[rel]]))
        b_ms = single(lambda i: host_parsed.batch(indices), args.host_batches, 0)

    c_ms = single(lambda i: device.batch(indices), args.batches, args.warmup)
    d_ms = single(lambda i: trainer.train_step(fixed), args.batches, args.warmup)
    e_ms = single(lambda i: trainer.train_step(device.batch(indices)), args.batches, args.warmup)
    c2_ms = single(lambda i: device.batch(indices), args.batches, args.warmup)  # again: the spread of (c)
    trainer.check_health(synchronize=True)
    rig.emit({
        "tool": "geometry_producer_rate", "device": torch.cuda.get_device_name(0), "B": B, "P": P, "N": N,
        "valid_parts": int(sum(parts)), "faces_per_part": int(store.part_face_off[1]), "store_bytes": int(store.nbytes),
        "store_pack_s": round(pack_s, 3), "batches": args.batches, "host_batches": args.host_batches,
        "a_host_obj_ms": a_ms and round(a_ms, 1), "b_host_parsed_ms": b_ms and round(b_ms, 1), "c_device_ms": round(c_ms, 4),
        "c_device_ms_repeat": round(c2_ms, 4), "d_step_ms": round(d_ms, 4), "e_device_and_step_ms": round(e_ms, 4),
        "launch": "eager"}, None)


if __name__ == "__main__":
    main()
