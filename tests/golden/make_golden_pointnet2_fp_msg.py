#!/usr/bin/env python3
"""Generate tests/golden/pointnet2_fp_msg.npz by RUNNING THE REFERENCE's `PointnetFPModule`, `PointnetSAModuleMSG` and
`PointNet2MSG` (pointnet2_ops/pointnet2_modules.py, models/modules/encoder/pointnet2/pointnet2_msg.py), in this container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pointnet2_fp_msg.py

As in make_golden_pointnet2.py the reference's Python files are loaded from their paths with `pointnet2_ops.pointnet2_utils`
bound to this package's `pointnet2_utils` on its CPU path (the numpy restatement `pointnet2_ref`).  The fixture pins the
WIRING of the modules to the reference's own Python; the operators are held to the restatement by
tests/test_pointnet2_interp*.py.  Two passes each, float32 and float64, from the same float32 values; in the float64 pass
the indices still come from the float32 restatement and the copy / interpolation operators are replaced by
dtype-preserving torch expressions (the three distances are recomputed in float64 at those indices).

FP case (`fp.` records): `PointnetFPModule([32, 32, 16])`, M = 3 clouds, n = 40 unknown and m = 12 known points, 24 known and
8 unknown feature channels; cloud 1's unknown points contain its known points (zero distances).  Recorded under `fp.f32.` /
`fp.f64.`: `out.dist`, `out.interp` (the input of the shared MLP), `out.pre.{1,4}` (the values in front of the ReLUs),
`out.train`, `out.eval`, `stat.<buffer>`, `grad.<parameter>`, `gin.{unknow_feats,known_feats}` of sum(out.train * w).  Plain:
`fp.unknown`, `fp.known`, `fp.unknow_feats`, `fp.known_feats`, `fp.w`, `fp.idx`, `fp.sd.<state_dict entry>` (the module's
state_dict before the step), `fp.names`, `fp.shapes`.

MSG case (`msg.` records): `PointNet2MSG(64)`, parameters from `param_fill.fill_parameters(module, MSG_SEED)`, 2 clouds of 96
points (the 512 and 128 centres repeat points, as the sampling allows).  Under `msg.f32.` / `msg.f64.` through
`param_fill.compact`: `new_xyz.{0,1}`, `features.{0,1,2}` (level 0 is the record of `PointnetSAModuleMSG` alone), `out.train`,
`out.eval`, `stat.<buffer>`, `grad.<parameter>`, `gin.points`.  Plain: `msg.points`, `msg.w`, `msg.names`, `msg.shapes`.

FP_SEED is the first seed from 0 at which, in float64, no pre-activation of the module's two ReLUs lies within
100 x anchored.FLIP_PREACT of zero relative to its channel's largest, so that no ReLU decision is a coin toss for a
float32-grade evaluation (the generator asserts it, and tests/test_pointnet2_interp.py asserts it on the record), and at
which the float32 pass is inside the float64-anchored bars of tests/anchored.py.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types
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

FP_SEED = 686
MSG_SEED = 5
FP_SHAPE = dict(M=3, n=40, m=12, C1=8, C2=24, mlp=[32, 32, 16])
MSG_FEAT_DIM = 64
MSG_CLOUDS, MSG_POINTS = 2, 96
PREACT_MARGIN = 100 * anchored.FLIP_PREACT


def load_reference_modules():
    """The reference's pointnet2_modules and PointNet2MSG, bound to this package's operator module."""
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
    pkg = types.ModuleType("_reference_pointnet2")            # pointnet2_msg.py imports its neighbour relatively
    pkg.__path__ = [str(base)]
    sys.modules["_reference_pointnet2"] = pkg
    load("_reference_pointnet2.pointnet2_ssg", base / "pointnet2_ssg.py")
    msg = load("_reference_pointnet2.pointnet2_msg", base / "pointnet2_msg.py")
    return mods, msg.PointNet2MSG, pu


def _gather64(features, idx):
    M, C, _ = features.shape
    flat = idx.long().reshape(M, 1, -1).expand(-1, C, -1)
    return features.gather(2, flat).reshape(M, C, *idx.shape[1:])


def _three_nn64(pu_three_nn):
    def three_nn(unknown, known):
        with torch.no_grad():
            _, idx = pu_three_nn(unknown, known)                                  # the float32 restatement's choice
            near = known[torch.arange(known.shape[0])[:, None, None], idx.long()]   # [M, n, 3, 3]
            d = unknown[:, :, None, :] - near
            d = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            return torch.sqrt(d), idx
    return three_nn


def _interpolate64(features, idx, weight):
    return (_gather64(features, idx) * weight[:, None]).sum(-1)


class swapped:
    """The float64 pass: the operator module's copies and interpolation replaced by dtype-preserving expressions."""

    def __init__(self, pu, dtype):
        self.pu, self.on = pu, dtype == torch.float64

    def __enter__(self):
        pu = self.pu
        self.saved = {k: getattr(pu, k) for k in ("grouping_operation", "gather_operation", "three_nn", "three_interpolate")}
        if self.on:
            pu.grouping_operation, pu.gather_operation = _gather64, _gather64
            pu.three_nn, pu.three_interpolate = _three_nn64(self.saved["three_nn"]), _interpolate64

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            setattr(self.pu, k, v)


def _np64(rec):
    return {k: v.detach().double().numpy() for k, v in rec.items()}


# ---- FP ----------------------------------------------------------------------------------------------------------------
def fp_inputs(seed):
    s = FP_SHAPE
    g = torch.Generator().manual_seed(seed)
    known = torch.rand(s["M"], s["m"], 3, generator=g) - 0.5
    unknown = torch.rand(s["M"], s["n"], 3, generator=g) - 0.5
    unknown[1, :s["m"]] = known[1]                                          # zero distances: weights of 1e8 before the norm
    return {"unknown": unknown, "known": known,
            "unknow_feats": torch.randn(s["M"], s["C1"], s["n"], generator=g),
            "known_feats": torch.randn(s["M"], s["C2"], s["m"], generator=g),
            "w": torch.randn(s["M"], s["mlp"][-1], s["n"], generator=g)}


def fp_run(mods, pu, inp, seed, dtype):
    torch.manual_seed(seed)
    fp = mods.PointnetFPModule(list(FP_SHAPE["mlp"]))
    param_fill.fill_parameters(fp, seed)
    sd0 = {k: v.clone() for k, v in fp.state_dict().items()}
    fp = fp.to(dtype).train()
    x = {k: v.detach().clone().to(dtype) for k, v in inp.items()}
    uf, kf = x["unknow_feats"].requires_grad_(), x["known_feats"].requires_grad_()
    rec = {}
    hooks = [fp.mlp[0].register_forward_hook(lambda m, i, o: rec.__setitem__("out.interp", i[0].squeeze(-1)))]
    hooks += [fp.mlp[j].register_forward_hook(                                 # (a copy: the ReLU behind it works in place)
        lambda m, i, o, j=j: rec.__setitem__(f"out.pre.{j}", o.detach().squeeze(-1).clone())) for j in (1, 4)]
    with swapped(pu, dtype):
        dist, idx = pu.three_nn(x["unknown"], x["known"])
        out = fp(x["unknown"], x["known"], uf, kf)
        (out * x["w"]).sum().backward()
        for h in hooks:
            h.remove()
        fp.eval()
        with torch.no_grad():
            out_eval = fp(x["unknown"], x["known"], uf, kf)
    rec.update({"out.dist": dist, "out.train": out, "out.eval": out_eval, "gin.unknow_feats": uf.grad,
                "gin.known_feats": kf.grad})
    sd = fp.state_dict()
    rec.update({f"stat.{k}": v for k, v in sd.items() if "running_" in k})
    rec.update({f"grad.{k}": p.grad for k, p in fp.named_parameters()})
    return _np64(rec), idx.numpy(), sd0


def preact_margin(rec):
    """Smallest |pre-activation| / (its channel's largest) over the module's two ReLUs ([M, C, n] records)."""
    worst = np.inf
    for j in (1, 4):
        pre = np.abs(rec[f"out.pre.{j}"])
        worst = min(worst, float((pre / pre.max(axis=(0, 2), keepdims=True)).min()))
    return worst


def fp_case(mods, pu):
    inp = fp_inputs(FP_SEED)
    r32, idx, sd0 = fp_run(mods, pu, inp, FP_SEED, torch.float32)
    r64, idx64, _ = fp_run(mods, pu, inp, FP_SEED, torch.float64)
    assert np.array_equal(idx, idx64)
    margin = preact_margin(r64)
    assert margin >= PREACT_MARGIN, f"FP_SEED {FP_SEED}: a pre-activation at {margin:.2e} of its channel's largest; change FP_SEED"
    t32, t64 = ({k: torch.from_numpy(v) for k, v in r.items()} for r in (r32, r64))
    e32, _, _ = anchored.bars(t32, t64)
    assert max(e32.values()) < anchored.CEIL, f"FP_SEED {FP_SEED}: float32 pass {max(e32.values()):.2e} from the float64 pass"
    print(f"fp: smallest relative pre-activation {margin:.2e}, float32 pass within {max(e32.values()):.2e} of float64")
    arrays = {f"fp.{k}": v.numpy() for k, v in inp.items()}
    arrays["fp.idx"] = idx
    arrays["fp.seed"] = np.int64(FP_SEED)
    arrays.update({f"fp.sd.{k}": v.numpy() for k, v in sd0.items()})
    arrays["fp.names"] = np.array(list(sd0))
    arrays["fp.shapes"] = np.array([",".join(map(str, v.shape)) for v in sd0.values()])
    for prefix, rec in (("fp.f32.", r32), ("fp.f64.", r64)):
        arrays.update({prefix + k: (v.astype(np.float32) if prefix == "fp.f32." else v) for k, v in rec.items()})
    return arrays


# ---- MSG ---------------------------------------------------------------------------------------------------------------
def msg_inputs():
    g = torch.Generator().manual_seed(MSG_SEED)
    pts = torch.rand(MSG_CLOUDS, MSG_POINTS, 3, generator=g) - 0.5
    return pts, torch.randn(MSG_CLOUDS, MSG_FEAT_DIM, generator=g)


def msg_run(cls, pu, pts, w, dtype):
    torch.manual_seed(MSG_SEED)
    enc = cls(MSG_FEAT_DIM)
    param_fill.fill_parameters(enc, MSG_SEED)
    enc = enc.to(dtype).train()
    levels = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: levels.append(out)) for m in enc.SA_modules]
    x = pts.detach().clone().to(dtype).requires_grad_()
    with swapped(pu, dtype):
        out = enc(x)
        (out * w.to(dtype)).sum().backward()
        for h in hooks:
            h.remove()
        enc.eval()
        with torch.no_grad():
            out_eval = enc(x.detach())
    rec = {"out.train": out, "out.eval": out_eval, "gin.points": x.grad}
    for i, (new_xyz, feats) in enumerate(levels):
        if new_xyz is not None:
            rec[f"new_xyz.{i}"] = new_xyz
        rec[f"features.{i}"] = feats
    sd = enc.state_dict()
    rec.update({f"stat.{k}": v for k, v in sd.items() if "running_" in k})
    rec.update({f"grad.{k}": p.grad for k, p in enc.named_parameters()})
    return _np64(rec), list(sd), [tuple(v.shape) for v in sd.values()]


def msg_case(cls, pu):
    pts, w = msg_inputs()
    r32, names, shapes = msg_run(cls, pu, pts, w, torch.float32)
    r64, _, _ = msg_run(cls, pu, pts, w, torch.float64)
    worst = max(anchored.err(r32[k], r64[k]) for k in r64 if not k.endswith(".bias"))
    print(f"msg: float32 pass within {worst:.2e} of the float64 pass on every record but the bias gradients")
    arrays = {"msg.points": pts.numpy(), "msg.w": w.numpy(), "msg.seed": np.int64(MSG_SEED), "msg.names": np.array(names),
              "msg.shapes": np.array([",".join(map(str, s)) for s in shapes])}
    for prefix, rec in (("msg.f32.", r32), ("msg.f64.", r64)):
        for k, v in rec.items():
            arrays.update(param_fill.compact(prefix, k, v))
    return arrays


def main():
    torch.set_num_threads(4)
    mods, msg_cls, pu = load_reference_modules()
    arrays = fp_case(mods, pu)
    arrays.update(msg_case(msg_cls, pu))
    path = HERE / "pointnet2_fp_msg.npz"
    np.savez_compressed(path, **arrays)
    print(f"wrote {path.name}: {len(arrays)} arrays, {path.stat().st_size / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
