#!/usr/bin/env python3
"""Generate the semantic graph-network fixtures under tests/golden/ by RUNNING THE REFERENCE on its PartNet configs.
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_semantic_gnn.py [--only dgl,rgl_net]

Same setup as make_golden.py (which, with _reference_shim.py, is left as it is): one training-mode `forward_pass` +
backward of the model `build_model(cfg)` returns, weights from `param_fill.fill_parameters`, recorded in float32 and once
more in float64 (the anchor of the gradient bar in tests/test_callers_gpu.py).  Outputs are plain .npz files of inputs and
the reference's outputs.

Fixture -> reference entry points exercised
  dgl_partnet_step.npz      configs/dgl/dgl-32x1-cosine_300e-partnet_chair.py: models/dgl/network.py with
                            `_gather_same_class` / `_merge_nodes` at the odd GNN iteration (:75-119), the second relation
                            net, base_model.py's matching inside groups of identical parts and min-of-5 sampling
  rgl_net_partnet_step.npz  configs/rgl_net/rgl_net-32x1-cosine_300e-partnet_chair.py: the same with the GRU node update

Shape: B = 2, max_num_part = 8, N = 128, pc_feat_dim shrunk to 64.  Per shape one group of 3 identical parts, one group of
2, one unique part and two padded slots (in another slot order in the second shape).
"""
from __future__ import annotations

import argparse
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

B, P, N = 2, 8, 128
PART_IDS = [[1, 1, 1, 2, 2, 3, 0, 0], [1, 2, 2, 3, 3, 3, 0, 0]]  # geo_part_ids, padded (partnet_data.py:190-192)


def semantic_batch(g):
    """The data_dict of PartNetPartDataset.__getitem__ (partnet_data.py:133-232) for the ids above, on synthetic clouds."""
    ids = torch.tensor(PART_IDS)
    data = mg.synthetic_batch(g, B, P, N, [int((row > 0).sum()) for row in ids])
    match = torch.zeros_like(ids)
    inst = torch.zeros(B, P, P)
    for b in range(B):
        label = 1
        for v in range(1, int(ids[b].max()) + 1):  # partnet_data.py:195-208
            members = torch.nonzero(ids[b] == v).flatten().tolist()
            if len(members) >= 2:
                match[b, members] = label
                label += 1
                for m in members[1:]:  # geometrically equivalent parts share one point cloud
                    data["part_pcs"][b, m] = data["part_pcs"][b, members[0]]
        seen = {}
        for p in range(P):  # partnet_data.py:163-173
            if ids[b, p] > 0:
                k = seen.get(int(ids[b, p]), 0)
                inst[b, p, k] = 1.0
                seen[int(ids[b, p])] = k + 1
    data["part_ids"] = ids
    data["match_ids"] = match
    data["instance_label"] = inst
    return data


def gen(name, rel_dir, module_name, seed):
    cfg = mg._load_cfg(rel_dir, module_name)
    assert cfg.data.dataset == "partnet" and cfg.model.merge_node and cfg.loss.sample_iter == 5
    cfg.model.pc_feat_dim = 64
    cfg.data.max_num_part = P
    g = torch.Generator().manual_seed(seed)
    mg._model_step(name, cfg, semantic_batch(g), seed, {"cfg": np.array([64, cfg.model.gnn_iter])})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    only = set(filter(None, ap.parse_args().only.split(",")))
    shim.import_reference()
    todo = {"dgl": lambda: gen("dgl_partnet_step", "configs/dgl", "dgl-32x1-cosine_300e-partnet_chair", 3001),
            "rgl_net": lambda: gen("rgl_net_partnet_step", "configs/rgl_net", "rgl_net-32x1-cosine_300e-partnet_chair",
                                   3002)}
    for name, fn in todo.items():
        if not only or name in only:
            fn()


if __name__ == "__main__":
    main()
