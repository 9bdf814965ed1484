#!/usr/bin/env python3
"""Generate tests/golden/sample_assembly.npz by RUNNING THE REFERENCE's `BaseModel.sample_assembly`
(models/modules/base_model.py:427-460, with `colorize_part_pc`, utils/utils.py:49-64) on a PNTransformer.
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_assembly.py

Same setup as make_golden.py / make_golden_rmat.py (which, with _reference_shim.py, are left as they are).  One record
per rot_type ('quat', 'rmat'), B = 3, P = 5, N = 37, part counts [2, 5, 3], sample_iter = 3 with the stochastic pose
regressor switched on (noise_dim = 32) so that the three forwards differ.  Recorded, as plain arrays:
  data.*                the batch (shared by both records)
  colors                the reference's colour table (cfg.data.colors) as data
  sd0.*                 the 'quat' model's parameters and buffers (param_fill.fill_parameters, keyed by name)
  rmat.sd0.*            those of the 'rmat' model that differ from them (the rotation head); the others are equal
  <rt>.pred_rot/_trans  the poses each of the three forwards returned, [3, B, P, 4 | 3, 3] and [3, B, P, 3]
  <rt>.gt_rot           the ground-truth rotation sample_assembly posed with, [B, P, 4 | 3, 3]
  <rt>.gt_pcs.<b>       gt_pcs_lst[b], float64 [p N, 6]
  <rt>.pred_pcs.<b>.<s> pred_pcs_lst[b][s], float64 [p N, 6]
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import _reference_shim as shim  # noqa: E402
import make_golden as mg  # noqa: E402
import make_golden_rmat as mgr  # noqa: E402

B, P, N, SAMPLES, SEED = 3, 5, 37, 3, 3001


def record(rot_type, data):
    from multi_part_assembly.models import build_model
    import param_fill

    cfg = mg._load_cfg("configs/pn_transformer/pn_transformer", "pn_transformer-32x1-cosine_400e-everyday")
    cfg.model.rot_type = rot_type
    cfg.model.pc_feat_dim, cfg.model.transformer_feat_dim = 32, 64
    cfg.model.transformer_heads, cfg.model.transformer_layers = 2, 1
    cfg.data.max_num_part = P
    cfg.loss.sample_iter, cfg.loss.noise_dim = SAMPLES, 32
    torch.manual_seed(SEED)
    model = build_model(cfg)
    param_fill.fill_parameters(model, SEED)
    mg.zero_dropout(model)
    model.eval()
    out = {f"{rot_type}.sd0.{k}": mg.npy(v) for k, v in model.state_dict().items()}
    poses = []
    forward = model.forward

    def watched(data_dict):
        res = forward(data_dict)
        poses.append((mg.npy(res["rot"]), mg.npy(res["trans"])))
        return res

    model.forward = watched
    batch = {k: v.clone() for k, v in data.items()}
    torch.manual_seed(SEED + 1)
    gt_pcs, pred_pcs = model.sample_assembly(batch)
    assert len(poses) == SAMPLES and len(gt_pcs) == B and all(len(p) == SAMPLES for p in pred_pcs)
    assert not np.array_equal(poses[0][0], poses[1][0])  # the forwards are stochastic
    out[f"{rot_type}.pred_rot"] = np.stack([r for r, _ in poses])
    out[f"{rot_type}.pred_trans"] = np.stack([t for _, t in poses])
    out[f"{rot_type}.gt_rot"] = mg.npy(batch["part_rot"])
    for b in range(B):
        out[f"{rot_type}.gt_pcs.{b}"] = gt_pcs[b]
        for s in range(SAMPLES):
            out[f"{rot_type}.pred_pcs.{b}.{s}"] = pred_pcs[b][s]
    return out, np.array(cfg.data.colors)


def main():
    mgr._cross_check_with_scipy()
    shim._install_pytorch3d = mgr._install_with_rmat(shim._install_pytorch3d)
    shim.import_reference()
    g = torch.Generator().manual_seed(SEED)
    data = mg.synthetic_batch(g, B, P, N, [2, 5, 3])
    out = {f"data.{k}": mg.npy(v) for k, v in data.items()}
    for rot_type in ("quat", "rmat"):
        rec, colors = record(rot_type, data)
        for k, v in rec.items():
            if k.startswith("quat.sd0."):
                out[k[len("quat."):]] = v
            elif k.startswith("rmat.sd0.") and np.array_equal(out.get(k[len("rmat."):]), v):
                continue
            else:
                out[k] = v
    out["colors"] = colors
    out["seed"] = np.array([SEED])
    mg.save("sample_assembly", **out)


if __name__ == "__main__":
    main()
