"""Evaluate a model on a dataset — the counterpart of the reference's scripts/test.py, a thin caller of
`multi_part_assembly_amd.evaluate`.

  python tools/evaluate.py --preset pn_transformer_everyday --weight ckpt.pt --data-dir data/breaking_bad \\
      --data-fn everyday.val.txt [--category Bottle | --category all] [--min-num-part 2] [--max-num-part 20]
      [--connectivity] [--encoder pointnet2_ssg [--pointnet2-eval fused]] [--weights ema]

`--preset` names a function of multi_part_assembly_amd.config; `--weight` a file written by `torch.save` holding either
`Trainer.state_dict()`, a Lightning-style `{"state_dict": ...}` or a bare model state dict (not needed for the identity
presets).  `--data-fn` lists shape folders (`everyday/Bottle/<id>`), one per line, as the Breaking-Bad split files do;
every `fractured_*` / `mode_*` folder below them whose part count is in range is evaluated.  `--category all` evaluates
every category of the everyday subset and prints the paper-table rows.  `--connectivity` adds the data key
`contact_points` — the contact table of every batch's own clouds and ground-truth poses, computed on the device — so
that the connectivity accuracy is reported too (a `connectivity_acc` value, and a row of the table)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multi_part_assembly_amd import config, datasets  # noqa: E402
from multi_part_assembly_amd.evaluate import Evaluator, evaluate_categories, format_table  # noqa: E402
from multi_part_assembly_amd.pn_transformer import build_model  # noqa: E402


def averaged_entry(state, path):
    """The averaged model state of a `Trainer.state_dict()` checkpoint (`ckpt["ema"]["model"]`); SystemExit if it has none."""
    ema = state.get("ema") if isinstance(state, dict) else None
    if not (isinstance(ema, dict) and isinstance(ema.get("model"), dict)):
        raise SystemExit(f"--weights ema: {path} holds no weight average (no \"ema\" entry: it was written by a run "
                         "without tools/train.py --ema, or is not a Trainer.state_dict() checkpoint)")
    return ema["model"]


def load_weights(model, path, device, weights="live"):
    # (weights_only=False: a checkpoint of `Trainer.fit` also holds the run's generator states, numpy's among them)
    state = torch.load(path, map_location=device, weights_only=False)
    if weights == "ema":
        model.load_state_dict(averaged_entry(state, path))
        return
    for key in ("model", "state_dict"):
        if isinstance(state, dict) and key in state and isinstance(state[key], dict):
            state = state[key]
            break
    model.load_state_dict(state)


def mesh_store(cfg, args, category):
    """The fractures of the data list as a `MeshStore`: the shape folders the list names are expanded into their
    `fractured_*` / `mode_*` sub-folders, restricted to `category` ('' or 'all': every shape), and fractures whose part
    count lies outside [min_num_part, max_num_part] are skipped, as the reference's dataset does."""
    folders = datasets.read_fracture_list(args.data_dir, args.data_fn, category, cfg.data.min_num_part,
                                          cfg.data.max_num_part)
    if not folders:
        raise ValueError(f"{args.data_fn}: no fracture of category '{category}' with {cfg.data.min_num_part} to "
                         f"{cfg.data.max_num_part} parts under {args.data_dir}")
    return datasets.MeshStore.from_folders(args.data_dir, folders, cfg.data.min_num_part, cfg.data.max_num_part)


def batches_for(cfg, args, category, device):
    """Batches of `exp.batch_size` fractures of `category` from the data list."""
    producer = datasets.DeviceGeometryProducer(mesh_store(cfg, args, category), num_points=cfg.data.num_pc_points,
                                               min_num_part=cfg.data.min_num_part, max_num_part=cfg.data.max_num_part,
                                               data_keys=cfg.data.data_keys, device=device)
    size = cfg.exp.batch_size
    for start in range(0, len(producer), size):
        yield producer.batch(list(range(start, min(start + size, len(producer)))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--preset", required=True)
    ap.add_argument("--weight", default="")
    ap.add_argument("--weights", choices=("live", "ema"), default="live",
                    help="which weights of the checkpoint to evaluate: the trained ones, or the exponential moving average "
                         "a run with tools/train.py --ema keeps beside them")
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--data-fn", required=True)
    ap.add_argument("--category", default="")
    ap.add_argument("--min-num-part", type=int, default=-1)
    ap.add_argument("--max-num-part", type=int, default=-1)
    ap.add_argument("--encoder", choices=("pointnet", "dgcnn", "pointnet2_ssg"), default=None,
                    help="cfg.model.encoder: the part encoder the weights were trained with (default: the preset's)")
    ap.add_argument("--pointnet2-eval", choices=("library", "fused"), default=None,
                    help="cfg.model.pointnet2_eval: how a pointnet2_ssg encoder evaluates — its library Conv2d / BatchNorm2d "
                         "chain (default) or the fused set-abstraction kernel; other encoders ignore it")
    ap.add_argument("--connectivity", action="store_true",
                    help="compute every batch's contact table and report the connectivity accuracy")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    cfg = getattr(config, args.preset)()
    if cfg.data.dataset != "geometry":
        raise SystemExit("tools/evaluate.py reads the Breaking-Bad folder layout; semantic presets need a PartNetBatchProducer")
    if args.min_num_part > 0:
        cfg.data.min_num_part = args.min_num_part
    if args.max_num_part > 0:
        cfg.data.max_num_part = args.max_num_part
    if args.encoder is not None:
        cfg.model.encoder = args.encoder
    if args.pointnet2_eval is not None:
        cfg.model.pointnet2_eval = args.pointnet2_eval
    if args.connectivity and "contact_points" not in cfg.data.data_keys:
        cfg.data.data_keys = tuple(cfg.data.data_keys) + ("contact_points",)
    device = torch.device("cuda:0")
    model = build_model(cfg).to(device)
    if args.weight:
        load_weights(model, args.weight, device, args.weights)
    elif cfg.model.name != "identity":
        raise SystemExit("please provide --weight (only the identity baseline needs none)")
    evaluator = Evaluator(model)
    if args.category != "all":
        res = evaluator.run(batches_for(cfg, args, args.category, device), prefix="test")
        print("; ".join(f"{k}: {v:.6f}" for k, v in res.items()))
        return
    table = evaluate_categories(evaluator, lambda cat: batches_for(cfg, args, cat, device), config.EVERYDAY_CATEGORIES,
                                connectivity=args.connectivity)
    print(format_table(table))


if __name__ == "__main__":
    main()
