"""Export the best assemblies of a model as meshes and point clouds — the counterpart of the reference's scripts/vis.py,
a thin caller of `multi_part_assembly_amd.assemble`.

  python tools/visualize.py --preset pn_transformer_everyday --weight ckpt.pt --data-dir data/breaking_bad \\
      --data-fn everyday.val.txt --vis 20 --out vis [--category Bottle] [--min-num-part 2] [--max-num-part 20]

Arguments and presets as tools/evaluate.py.  The fractures of the data list are ranked by `rot_pt_l2_loss + trans_mae`
(`rank_assemblies`); for the `--vis` best of them the original meshes are posed with the ground-truth and the
predicted transforms (`pose_meshes`) and the sampled clouds with `assemble_clouds`.  Written below
`<out>/<category or all>/rank<r>-<p>pcs-<shape>/`: per part `<part>.obj` (as stored), `input_<part>.obj` (as the
network sees it), `pred_<part>.obj`, `input_<part>.ply`, `pred_<part>.ply`, and one `assembly.ply` per shape: ground
truth and prediction side by side (`assembly_figure`), the parts coloured by `cfg.data.colors`."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multi_part_assembly_amd import assemble, config, datasets  # noqa: E402
from multi_part_assembly_amd.pn_transformer import build_model  # noqa: E402
from multi_part_assembly_amd.trainer import Trainer  # noqa: E402


def load_checkpoint(model, cfg, path, device, weights="live"):
    """`Trainer.load_state_dict` on what `torch.save` wrote: `Trainer.state_dict()`, a Lightning-style `{"state_dict":
    ...}`, or a bare model state dict.  `weights="ema"`: the checkpoint's weight average (`ckpt["ema"]["model"]`, written
    by a run with tools/train.py --ema) goes into the model instead; SystemExit if the checkpoint has none."""
    # (weights_only=False: a checkpoint of `Trainer.fit` also holds the run's generator states, numpy's among them)
    state = torch.load(path, map_location=device, weights_only=False)
    if weights == "ema":
        ema = state.get("ema") if isinstance(state, dict) else None
        if not (isinstance(ema, dict) and isinstance(ema.get("model"), dict)):
            raise SystemExit(f"--weights ema: {path} holds no weight average (no \"ema\" entry: it was written by a run "
                             "without tools/train.py --ema, or is not a Trainer.state_dict() checkpoint)")
        state = ema["model"]
    if not (isinstance(state, dict) and ("model" in state or "state_dict" in state)):
        state = {"state_dict": state}
    Trainer(model, cfg).load_state_dict(state)


def export(model, cfg, data_dir, folders, out_dir, vis, device):
    """Rank the fractures `folders` (relative to `data_dir`) and write the `vis` best below `out_dir`; returns the
    directories written, best first."""
    store = datasets.MeshStore.from_folders(data_dir, folders, cfg.data.min_num_part, cfg.data.max_num_part)
    producer = datasets.DeviceGeometryProducer(store, num_points=cfg.data.num_pc_points,
                                               min_num_part=cfg.data.min_num_part, max_num_part=cfg.data.max_num_part,
                                               data_keys=cfg.data.data_keys, device=device)
    size = cfg.exp.batch_size
    # batch_counter = the batch's first shape: the clouds of a shape are the same whenever it is sampled again below
    batches = (producer.batch(list(range(a, min(a + size, len(producer)))), batch_counter=a)
               for a in range(0, len(producer), size))
    records = assemble.rank_assemblies(model, batches, top=vis)
    if not records:
        return []
    colors = torch.tensor(cfg.data.colors, dtype=torch.float32, device=device)
    P, N = cfg.data.max_num_part, cfg.data.num_pc_points
    ids = [int(r["data_id"]) for r in records]
    stack = lambda key: np.stack([r[key] for r in records])
    slots = producer.slot_parts(ids)
    meshes = assemble.pose_meshes(store, slots, stack("gt_quat"), stack("gt_trans"), stack("pred_quat"),
                                  stack("pred_trans"), rot_type="quat")
    tri = meshes.to_host()
    # the clouds the ranking saw: the batches that hold a picked shape, sampled again on their own random streams (once each)
    again = {a: producer.batch(list(range(a, min(a + size, len(producer)))), batch_counter=a)["part_pcs"]
             for a in sorted({i - i % size for i in ids})}
    pcs = torch.stack([again[i - i % size][i % size] for i in ids])
    dev = lambda key: torch.from_numpy(stack(key)).to(device)
    clouds = assemble.assemble_clouds(pcs, dev("part_valids").float(), dev("pred_quat"), dev("pred_trans"),
                                      dev("gt_quat"), dev("gt_trans"), colors, rot_type="quat")
    rows, off = clouds.to_host(rows=N * sum(int(r["part_valids"].sum()) for r in records))  # the records know the count
    figures = assemble.assembly_figure(*assemble.rows_to_lists(rows, off))
    sampled = pcs.cpu().numpy()  # the parts as the network sees them
    written = []
    for rank, (rec, i) in enumerate(zip(records, ids)):
        folder = folders[i]
        names = sorted(os.listdir(os.path.join(data_dir, folder)))
        assert len(names) == int(rec["part_valids"].sum())
        shape = "-".join(folder.replace("\\", "/").split("/")[-2:])
        target = os.path.join(out_dir, f"rank{rank}-{len(names)}pcs-{shape}")
        os.makedirs(target, exist_ok=True)
        for k, name in enumerate(names):
            stem = os.path.splitext(name)[0]
            orig, inp, pred = meshes.slot(tri, rank * P + k)
            assemble.write_obj(os.path.join(target, f"{stem}.obj"), orig)
            assemble.write_obj(os.path.join(target, f"input_{stem}.obj"), inp)
            assemble.write_obj(os.path.join(target, f"pred_{stem}.obj"), pred)
            a = off[rank] + k * N
            assemble.write_ply(os.path.join(target, f"input_{stem}.ply"), sampled[rank, k])
            assemble.write_ply(os.path.join(target, f"pred_{stem}.ply"), rows[0, a:a + N, :3])
        fig = figures[rank]
        assemble.write_ply(os.path.join(target, "assembly.ply"), fig[:, :3], fig[:, 3:])
        written.append(target)
    return written


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--preset", required=True)
    ap.add_argument("--weight", default="")
    ap.add_argument("--weights", choices=("live", "ema"), default="live",
                    help="which weights of the checkpoint to export with: the trained ones, or the exponential moving "
                         "average a run with tools/train.py --ema keeps beside them")
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--data-fn", required=True)
    ap.add_argument("--category", default="")
    ap.add_argument("--min-num-part", type=int, default=-1)
    ap.add_argument("--max-num-part", type=int, default=-1)
    ap.add_argument("--num-points", type=int, default=-1, help="points sampled per part (default: the preset's)")
    ap.add_argument("--vis", type=int, default=-1, help="how many of the best assemblies to write (default: all)")
    ap.add_argument("--out", required=True, help="directory to write below")
    ap.add_argument("--encoder", choices=("pointnet", "dgcnn", "pointnet2_ssg"), default=None,
                    help="cfg.model.encoder: the part encoder the weights were trained with (default: the preset's)")
    ap.add_argument("--pointnet2-eval", choices=("library", "fused"), default=None,
                    help="cfg.model.pointnet2_eval: how a pointnet2_ssg encoder evaluates — its library Conv2d / BatchNorm2d "
                         "chain (default) or the fused set-abstraction kernel; other encoders ignore it")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    cfg = getattr(config, args.preset)()
    if cfg.data.dataset != "geometry":
        raise SystemExit("tools/visualize.py reads the Breaking-Bad folder layout (part meshes); semantic presets have none")
    if args.min_num_part > 0:
        cfg.data.min_num_part = args.min_num_part
    if args.max_num_part > 0:
        cfg.data.max_num_part = args.max_num_part
    if args.num_points > 0:
        cfg.data.num_pc_points = args.num_points
    if args.encoder is not None:
        cfg.model.encoder = args.encoder
    if args.pointnet2_eval is not None:
        cfg.model.pointnet2_eval = args.pointnet2_eval
    device = torch.device("cuda:0")
    model = build_model(cfg).to(device)
    if args.weight:
        load_checkpoint(model, cfg, args.weight, device, args.weights)
    elif cfg.model.name != "identity":
        raise SystemExit("please provide --weight (only the identity baseline needs none)")
    folders = datasets.read_fracture_list(args.data_dir, args.data_fn, args.category, cfg.data.min_num_part,
                                          cfg.data.max_num_part)
    if not folders:
        raise SystemExit(f"{args.data_fn}: no fracture of category '{args.category}' with {cfg.data.min_num_part} to "
                         f"{cfg.data.max_num_part} parts under {args.data_dir}")
    written = export(model, cfg, args.data_dir, folders, os.path.join(args.out, args.category or "all"), args.vis, device)
    print(f"Saving {len(written)} predictions for visualization below {os.path.join(args.out, args.category or 'all')}")
    return written


if __name__ == "__main__":
    main()
