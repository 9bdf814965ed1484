"""Train a model — the counterpart of the reference's scripts/train.py, a thin caller of `Trainer.fit`.

  python tools/train.py --preset pn_transformer_everyday --data-dir data/breaking_bad --data-fn everyday.train.txt \\
      --val-fn everyday.val.txt [--category Bottle] [--epochs 400] [--graph] [--ckpt-dir ckpt] [--resume]
  python tools/train.py --preset pn_transformer_everyday --skip-nonfinite --skip-limit 20 ...  (bad steps skipped on the device)
  python tools/train.py --preset pn_transformer_everyday --skip-nonfinite --rollback-buffers ...  (and their BatchNorm statistics undone)
  python tools/train.py --preset pn_transformer_everyday --ema DECAY [--no-ema-warmup] ...  (averaged weights kept, validated, saved)
  python tools/train.py --preset pn_transformer_everyday --accumulate K ...         (one optimiser step per K batches, on their mean)
  python tools/train.py --preset pn_transformer_everyday --repulsion 0.01 1.0 ...   (the opt-in repulsion term: THRE W)
  python tools/train.py --preset lstm_everyday --lstm-draws device --graph ...      (B-LSTM captured: its draws on the device)
  python tools/train.py --preset dgl_partnet_chair --data-dir data/partnet --data-fn Chair.train.npy --val-fn Chair.val.npy
  python tools/train.py --preset pn_transformer_everyday --synthetic --epochs 2
  torchrun --nproc-per-node 8 tools/train.py ...      (one rank per GPU; every rank keeps its stride of the epoch's order)

`--preset` names a function of multi_part_assembly_amd.config.  The training split is parsed once into a device-resident
store (`MeshStore` for the Breaking-Bad folders, `PartNetStore` for the PartNet files), the order of every epoch is drawn
on the device (`EpochSampler`) and the batches are built there (`DeviceGeometryProducer`, `DevicePartNetProducer`): the
host only launches.  `--synthetic` trains on seeded stand-in data (`synthetic.make_fracture_meshes` /
`make_partnet_like_store`), so the tool runs with no dataset on disk.  `--ckpt-dir` receives `model-epoch=NNN.pt` (the
best 5 by `--monitor`) and `last.pt`; `--resume` continues from `last.pt`.  One line is printed per `--log-every` steps and
per epoch."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--preset", required=True)
    ap.add_argument("--data-dir", default="")
    ap.add_argument("--data-fn", default="")
    ap.add_argument("--val-fn", default="")
    ap.add_argument("--category", default="")
    ap.add_argument("--epochs", type=int, default=-1, help="cfg.exp.num_epochs (the cosine schedule spans it)")
    ap.add_argument("--batch-size", type=int, default=-1, help="per rank; default cfg.exp.batch_size")
    ap.add_argument("--graph", action="store_true", help="capture the step as a HIP graph")
    ap.add_argument("--lstm-draws", choices=("host", "device"), default=None,
                    help="cfg.model.lstm_draws: B-LSTM's coin, noise and masks from the host generators (the presets' "
                         "default) or from a kernel — what --graph needs for the lstm presets")
    ap.add_argument("--encoder", choices=("pointnet", "dgcnn", "pointnet2_ssg"), default=None,
                    help="cfg.model.encoder: the part encoder (default: the preset's)")
    ap.add_argument("--pointnet2-eval", choices=("library", "fused"), default=None,
                    help="cfg.model.pointnet2_eval: how a pointnet2_ssg encoder evaluates — its library Conv2d / BatchNorm2d "
                         "chain (default) or the fused set-abstraction kernel; other encoders ignore it")
    ap.add_argument("--repulsion", nargs=2, type=float, default=None, metavar=("THRE", "W"),
                    help="add the repulsion term: cfg.loss.use_repulsion_loss = True, repulsion_thre = THRE (the Chamfer "
                         "distance below which a pair of parts is pushed apart), repulsion_loss_w = W; no default exists")
    ap.add_argument("--ckpt-dir", default="")
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--synthetic-shapes", type=int, default=64)
    ap.add_argument("--val-every", type=int, default=-1)
    ap.add_argument("--monitor", default="val/part_acc")
    ap.add_argument("--log-every", type=int, default=50)
    ap.add_argument("--max-steps", type=int, default=-1, help="stop after this many steps, leaving last.pt to resume from")
    ap.add_argument("--skip-nonfinite", action="store_true",
                    help="cfg.optimizer.skip_nonfinite: skip, on the device, every optimiser step whose gradient holds a NaN "
                         "or an inf or behind which a launch gave up (parameters, moments and step count keep their bits)")
    ap.add_argument("--skip-limit", type=int, default=-1, metavar="N",
                    help="with --skip-nonfinite: stop at a log line that finds N steps skipped in a row")
    ap.add_argument("--rollback-buffers", action="store_true",
                    help="with --skip-nonfinite: cfg.optimizer.skip_rollback_buffers: a skipped step also rolls back every "
                         "module buffer (BatchNorm running statistics, num_batches_tracked) on the device")
    ap.add_argument("--ema", type=float, default=None, metavar="DECAY",
                    help="cfg.optimizer.ema_decay in [0, 1): keep an exponential moving average of the weights on the device; "
                         "validation and the checkpoint ranking then use it, and the checkpoints carry it (tools/evaluate.py "
                         "--weights ema); no default exists")
    ap.add_argument("--no-ema-warmup", action="store_true",
                    help="with --ema: cfg.optimizer.ema_warmup = False, the decay is DECAY from the first step instead of "
                         "min(DECAY, (1 + t) / (10 + t))")
    ap.add_argument("--accumulate", type=int, default=None, metavar="K",
                    help="cfg.optimizer.accumulate_grad_batches: one optimiser step per K batches, on the mean of their "
                         "gradients (BatchNorm statistics per batch, as K ranks would keep them); --batch-size, --log-every "
                         "and --max-steps then count micro-batches, and an epoch's last window may be shorter")
    ap.add_argument("--seed", type=int, default=0)
    return ap


def parse_args(argv=None):
    ap = parser()
    args = ap.parse_args(argv)
    if not args.synthetic and not (args.data_dir and args.data_fn):
        ap.error("--data-dir and --data-fn are needed unless --synthetic is given")
    if args.resume and not args.ckpt_dir:
        ap.error("--resume needs --ckpt-dir")
    if args.skip_limit > 0 and not args.skip_nonfinite:
        ap.error("--skip-limit needs --skip-nonfinite")
    if args.rollback_buffers and not args.skip_nonfinite:
        ap.error("--rollback-buffers needs --skip-nonfinite")
    if args.ema is not None and not 0.0 <= args.ema < 1.0:
        ap.error("--ema DECAY must lie in [0, 1)")
    if args.no_ema_warmup and args.ema is None:
        ap.error("--no-ema-warmup needs --ema")
    if args.accumulate is not None and args.accumulate < 1:
        ap.error("--accumulate K must be at least 1")
    return args


def stores(cfg, args):
    """(training store, validation store or None) for the preset's dataset."""
    import numpy as np

    from multi_part_assembly_amd import datasets, synthetic
    lo, hi, n = cfg.data.min_num_part, cfg.data.max_num_part, args.synthetic_shapes
    if cfg.data.dataset == "geometry":
        if args.synthetic:
            def make(seed, shapes):
                counts = np.random.RandomState(seed).randint(lo, min(hi, 8) + 1, size=shapes).tolist()
                return datasets.MeshStore.from_arrays(synthetic.make_fracture_meshes(seed, shapes, counts, 200), lo, hi)
            return make(args.seed + 1, n), make(args.seed + 2, max(n // 4, 1))

        def load(fn):
            folders = datasets.read_fracture_list(args.data_dir, fn, args.category, lo, hi)
            if not folders:
                raise SystemExit(f"{fn}: no fracture of category '{args.category}' with {lo} to {hi} parts")
            return datasets.MeshStore.from_folders(args.data_dir, folders, lo, hi)
    else:
        if args.synthetic:
            make = lambda seed, shapes: synthetic.make_partnet_like_store(  # noqa: E731
                shapes, max_parts=hi, num_points=cfg.data.num_pc_points, seed=seed,
                num_part_category=cfg.data.num_part_category, min_parts=lo)
            return make(args.seed + 1, n), make(args.seed + 2, max(n // 4, 1))
        load = lambda fn: datasets.PartNetStore.from_folder(args.data_dir, fn, lo, hi)  # noqa: E731
    return load(args.data_fn), (load(args.val_fn) if args.val_fn else None)


def producer(cfg, store, device, seed, train):
    from multi_part_assembly_amd import datasets
    if cfg.data.dataset == "geometry":
        return datasets.DeviceGeometryProducer(store, num_points=cfg.data.num_pc_points,
                                               min_num_part=cfg.data.min_num_part, max_num_part=cfg.data.max_num_part,
                                               rot_range=cfg.data.get("rot_range", -1), data_keys=cfg.data.data_keys,
                                               seed=seed, device=device)
    return datasets.DevicePartNetProducer(store, cfg.data.data_keys, num_part_category=cfg.data.num_part_category,
                                          min_num_part=cfg.data.min_num_part, max_num_part=cfg.data.max_num_part,
                                          shuffle_parts=train and cfg.data.get("shuffle_parts", False), seed=seed,
                                          device=device)


def configure(args):
    """The preset's configuration with the command line's overrides applied."""
    from multi_part_assembly_amd import config

    cfg = getattr(config, args.preset)()
    if args.epochs > 0:
        cfg.exp.num_epochs = args.epochs
    if args.batch_size > 0:
        cfg.exp.batch_size = args.batch_size
    if cfg.data.dataset != "geometry":
        cfg.loss.match_sample = "device"  # the matching's point sample drawn by a kernel: no host copy in the step
    if args.lstm_draws is not None:
        cfg.model.lstm_draws = args.lstm_draws
    if args.encoder is not None:
        cfg.model.encoder = args.encoder
    if args.pointnet2_eval is not None:
        cfg.model.pointnet2_eval = args.pointnet2_eval  # (the validation passes; training is the library chain either way)
    if args.repulsion is not None:
        cfg.loss.use_repulsion_loss = True
        cfg.loss.repulsion_thre, cfg.loss.repulsion_loss_w = args.repulsion
    if args.skip_nonfinite:
        cfg.optimizer.skip_nonfinite = True
    if args.rollback_buffers:
        cfg.optimizer.skip_rollback_buffers = True
    if args.ema is not None:
        cfg.optimizer.ema_decay = args.ema
        if args.no_ema_warmup:
            cfg.optimizer.ema_warmup = False
    if args.accumulate is not None:
        cfg.optimizer.accumulate_grad_batches = args.accumulate
    return cfg


def main(argv=None):
    args = parse_args(argv)
    import torch
    import torch.distributed as dist

    from multi_part_assembly_amd.pn_transformer import build_model
    from multi_part_assembly_amd.sampler import EpochSampler
    from multi_part_assembly_amd.trainer import Trainer

    cfg = configure(args)
    world, rank, local = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", 1), ("RANK", 0), ("LOCAL_RANK", 0)))
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    if world > 1:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
    torch.manual_seed(args.seed)
    train_store, val_store = stores(cfg, args)
    train = producer(cfg, train_store, device, args.seed, train=True)
    batch = min(cfg.exp.batch_size, -(-len(train) // world))
    sampler = EpochSampler(len(train), batch, seed=args.seed, world=world, rank=rank, device=device)
    val_batches = None
    if val_store is not None:
        val = producer(cfg, val_store, device, args.seed + 1, train=False)
        val_sampler = EpochSampler(len(val), cfg.exp.batch_size, world=world, rank=rank, shuffle=False,
                                   drop_last=False, device=device)

        def val_batches():  # the same streams in every pass: validation results are comparable across epochs
            val_sampler.set_epoch(0)
            for k, idx in enumerate(val_sampler):
                yield val.batch(idx, batch_counter=k)

    trainer = Trainer(build_model(cfg).to(device), cfg, use_graph=args.graph)
    log = (lambda rec: print("; ".join(f"{k}: {v:.6g}" if isinstance(v, float) else f"{k}: {v}"
                                       for k, v in rec.items()), flush=True)) if rank == 0 else None
    if args.resume:
        start = trainer.resume(args.ckpt_dir)
        if rank == 0:
            print(f"resuming at epoch {start}", flush=True)
    history = trainer.fit(train, sampler, val_batches=val_batches, val_every=args.val_every if args.val_every > 0 else None,
                          ckpt_dir=args.ckpt_dir or None, monitor=args.monitor, log_every=args.log_every, on_log=log,
                          max_steps=args.max_steps if args.max_steps > 0 else None,
                          skip_limit=args.skip_limit if args.skip_limit > 0 else None)
    if rank == 0:
        steps = f"; {trainer.micro_batches} micro-batches in {trainer.optimizer.step_count} optimiser steps" \
            if trainer.accumulate > 1 else ""
        print(f"done: {len(history)} epochs in the history{steps}", flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
