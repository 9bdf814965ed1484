#!/usr/bin/env python3
"""Generate tests/golden/pointnet2_ssg.npz by RUNNING THE REFERENCE's `PointNet2SSG`
(models/modules/encoder/pointnet2/pointnet2_ssg.py over pointnet2_ops/pointnet2_modules.py), in this container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pointnet2.py

The reference's two Python files are loaded from their paths with `pointnet2_ops.pointnet2_utils` bound to this
package's `pointnet2_utils` on its CPU path (the numpy restatement `pointnet2_ref`): the reference's CUDA extension cannot
be built here.  The fixture therefore pins the WIRING of the set-abstraction modules (sampling -> gather -> ball query ->
grouping -> centre subtraction -> [xyz ; features] -> shared MLP -> max, three levels) to the reference's own Python; it
cannot pin the operators, which tests/test_pointnet2_ops*.py hold to the restatement.

`PointNet2SSG(128)`, parameters from `param_fill.fill_parameters(module, SEED)`, 3 clouds of 600 points: one whose last 150
rows are zero (B-Global's padding), one with 40 duplicated points, one plain.  Two passes, float32 and float64, from the
same float32 values; in the float64 pass the indices still come from the float32 restatement (the copies are exact, so
they are the same indices) and only the two copy operators are replaced by dtype-preserving `torch.gather`s.

Recorded, each under `f32.` and `f64.` through `param_fill.compact`: `new_xyz.{0,1}` and `features.{0,1,2}` after each
level, `out.train`, `out.eval` (after the training forward), `stat.<buffer>` (the updated running statistics) and
`grad.<parameter>` of sum(out.train * w).  Plain: `points`, `w`, `names`, `shapes`, `seed`.

SEED = 12 (7, 1, 2, 3 and 11 each flip a selection between the two passes).  It may change for one reason only: a max /
ReLU selection at a near tie that puts the float32 pass outside the float64-anchored bars of tests/anchored.py (the generator asserts that it is inside: every e32 below the ceiling; a bias
gradient that is structurally zero in float64 — the last BatchNorm bias of a level whose every maximum is positive, in front
of the next level's normalisation — is held to anchored's absolute rule instead).
"""
from __future__ import annotations

import importlib.util
import os
import sys
from pathlib import Path

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))
import _reference_shim as shim  # noqa: E402
import param_fill  # noqa: E402
sys.path.insert(0, str(HERE.parent))
import anchored  # noqa: E402

SEED = 12
FEAT_DIM = 128
N_POINTS = 600
CEIL = anchored.CEIL


def make_points():
    g = torch.Generator().manual_seed(SEED)
    pts = torch.rand(3, N_POINTS, 3, generator=g) - 0.5
    pts[0, N_POINTS - 150:] = 0.0                                  # zero padding, never sampled
    src = torch.randperm(N_POINTS - 40, generator=g)[:40]
    pts[1, N_POINTS - 40:] = pts[1, src]                           # 40 exact duplicates
    w = torch.randn(3, FEAT_DIM, generator=g)
    return pts, w


def load_reference_encoder():
    """The reference's PointNet2SSG class, its modules file bound to this package's operator module."""
    shim.import_reference()
    from multi_part_assembly_amd import pointnet2_utils as pu
    base = Path(shim.REFERENCE_ROOT) / "multi_part_assembly/models/modules/encoder/pointnet2"
    ops = sys.modules["pointnet2_ops"]
    ops.pointnet2_utils = pu
    sys.modules["pointnet2_ops.pointnet2_utils"] = pu

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    mods = load("pointnet2_ops.pointnet2_modules", base / "pointnet2_ops_lib/pointnet2_ops/pointnet2_modules.py")
    ops.pointnet2_modules = mods
    ssg = load("_reference_pointnet2_ssg", base / "pointnet2_ssg.py")
    return ssg.PointNet2SSG, pu


def _gather64(features, idx):
    M, C, _ = features.shape
    flat = idx.long().reshape(M, 1, -1).expand(-1, C, -1)
    return features.gather(2, flat).reshape(M, C, *idx.shape[1:])


def run(cls, pu, pts, w, dtype):
    torch.manual_seed(SEED)
    enc = cls(FEAT_DIM)
    param_fill.fill_parameters(enc, SEED)
    enc = enc.to(dtype).train()
    levels = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: levels.append(out)) for m in enc.SA_modules]
    saved = pu.grouping_operation, pu.gather_operation
    if dtype == torch.float64:
        pu.grouping_operation, pu.gather_operation = _gather64, _gather64
    try:
        out = enc(pts.to(dtype))
        (out * w.to(dtype)).sum().backward()
        for h in hooks:
            h.remove()
        enc.eval()
        with torch.no_grad():
            out_eval = enc(pts.to(dtype))
    finally:
        pu.grouping_operation, pu.gather_operation = saved
    rec = {"out.train": out, "out.eval": out_eval}
    for i, (new_xyz, feats) in enumerate(levels):
        if new_xyz is not None:
            rec[f"new_xyz.{i}"] = new_xyz
        rec[f"features.{i}"] = feats
    sd = enc.state_dict()
    rec.update({f"stat.{k}": v for k, v in sd.items() if "running_" in k})
    rec.update({f"grad.{k}": p.grad for k, p in enc.named_parameters()})
    names = list(sd)
    shapes = [tuple(v.shape) for v in sd.values()]
    return {k: v.detach().double().numpy() for k, v in rec.items()}, names, shapes


def main():
    torch.set_num_threads(4)
    cls, pu = load_reference_encoder()
    pts, w = make_points()
    r32, names, shapes = run(cls, pu, pts, w, torch.float32)
    r64, _, _ = run(cls, pu, pts, w, torch.float64)
    worst = 0.0
    t64 = {k: torch.from_numpy(v) for k, v in r64.items()}
    for k in r64:
        ws = anchored._zero_scale(k, t64)
        if ws is not None:
            assert np.abs(r32[k]).max() <= anchored.ZERO_ABS * ws, f"{k}: structurally zero in float64, not in float32"
            continue
        e = anchored.err(r32[k], r64[k])
        worst = max(worst, e)
        assert e < CEIL, f"{k}: the float32 pass is {e:.2e} from the float64 pass — a selection flipped; change SEED"
    print(f"float32 pass within {worst:.2e} of the float64 pass on every record")
    arrays = {"points": pts.numpy(), "w": w.numpy(), "seed": np.int64(SEED), "names": np.array(names),
              "shapes": np.array([",".join(map(str, s)) for s in shapes])}
    for prefix, rec in (("f32.", r32), ("f64.", r64)):
        for k, v in rec.items():
            arrays.update(param_fill.compact(prefix, k, v))
    path = HERE / "pointnet2_ssg.npz"
    np.savez_compressed(path, **arrays)
    print(f"wrote {path.name}: {len(arrays)} arrays, {path.stat().st_size / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
