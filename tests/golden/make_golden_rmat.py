#!/usr/bin/env python3
"""Generate the rot_type='rmat' fixtures under tests/golden/ by RUNNING THE REFERENCE with `cfg.model.rot_type = 'rmat'`.
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rmat.py [--only transforms,pn_transformer,...]

Same setup as make_golden.py (which, with _reference_shim.py, is left as it is), plus the two pytorch3d functions the
matrix path calls: `rotation_6d_to_matrix` and `matrix_to_quaternion`, restated from pytorch3d's published code and
cross-checked against scipy before anything is recorded.  Outputs are plain .npz files of inputs and the reference's
outputs.

Fixture -> reference entry points exercised
  rmat_transforms.npz          utils/rotation.py:134-204 (Rotation3D 'rmat' from 6D, convert, to_euler),
                               utils/transforms.py:126-244 (rmat_rot / rmat_transform via rot_pc / transform_pc)
  pn_transformer_rmat_step.npz models/pn_transformer/network.py + base_model.py, 6D rotation head
  dgl_rmat_step.npz            models/dgl (9-wide pose fed back through the GNN iterations)
  global_rmat_semantic_step.npz models/global on semantic data (matching in matrix form, min-of-5)
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
import torch.nn.functional as F  # noqa: E402

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import _reference_shim as shim  # noqa: E402
import make_golden as mg  # noqa: E402


# ---- the two pytorch3d stand-ins (pytorch3d/transforms/rotation_conversions.py, restated) -------------------------------
def rotation_6d_to_matrix(d6):
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = F.normalize(a1, dim=-1)
    b2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = F.normalize(b2, dim=-1)
    b3 = torch.cross(b1, b2, dim=-1)
    return torch.stack((b1, b2, b3), dim=-2)


def _sqrt_positive_part(x):
    ret = torch.zeros_like(x)
    positive_mask = x > 0
    ret[positive_mask] = torch.sqrt(x[positive_mask])
    return ret


def matrix_to_quaternion(matrix):
    batch_dim = matrix.shape[:-2]
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = torch.unbind(matrix.reshape(batch_dim + (9,)), dim=-1)
    q_abs = _sqrt_positive_part(torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22,
                                             1.0 - m00 - m11 + m22], dim=-1))
    quat_by_rijk = torch.stack([
        torch.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], dim=-1),
        torch.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], dim=-1),
        torch.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], dim=-1),
        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], dim=-1),
    ], dim=-2)
    flr = torch.tensor(0.1).to(dtype=q_abs.dtype, device=q_abs.device)
    quat_candidates = quat_by_rijk / (2.0 * q_abs[..., None].max(flr))
    out = quat_candidates[F.one_hot(q_abs.argmax(dim=-1), num_classes=4) > 0.5, :].reshape(batch_dim + (4,))
    return torch.where(out[..., 0:1] < 0, -out, out)  # standardize_quaternion


def _cross_check_with_scipy():
    from scipy.spatial.transform import Rotation as R

    g = torch.Generator().manual_seed(77)
    q = F.normalize(torch.randn(256, 4, generator=g, dtype=torch.float64), dim=-1)
    sci = R.from_quat(q[:, [1, 2, 3, 0]].numpy())
    m = torch.from_numpy(sci.as_matrix())
    assert np.allclose(shim.quaternion_to_matrix(q).numpy(), m.numpy(), atol=1e-12)
    back = matrix_to_quaternion(m)
    assert np.allclose(back.numpy(), (q * torch.where(q[:, :1] < 0, -1.0, 1.0)).numpy(), atol=1e-12)
    d6 = torch.randn(256, 6, generator=g, dtype=torch.float64)
    m6 = rotation_6d_to_matrix(d6).numpy()
    assert np.allclose(m6 @ np.swapaxes(m6, -1, -2), np.eye(3), atol=1e-12) and np.allclose(np.linalg.det(m6), 1.0)
    # the first row is the normalised a1, the second lies in span(a1, a2)
    assert np.allclose(m6[:, 0], d6[:, :3].numpy() / np.linalg.norm(d6[:, :3].numpy(), axis=-1, keepdims=True))
    print("stand-ins agree with scipy")


def _install_with_rmat(orig):
    def install():
        orig()
        tr = sys.modules["pytorch3d.transforms"]
        tr.rotation_6d_to_matrix = rotation_6d_to_matrix
        tr.matrix_to_quaternion = matrix_to_quaternion
    return install


# ---- fixtures ---------------------------------------------------------------------------------------------------------
def gen_transforms():
    from multi_part_assembly.utils.rotation import Rotation3D
    from multi_part_assembly.utils.transforms import transform_pc

    g = torch.Generator().manual_seed(2001)
    quat = mg.unit_quats(g, 64) * 1.2
    d6 = torch.randn(64, 6, generator=g)
    pc = torch.randn(64, 200, 3, generator=g)
    trans = torch.randn(64, 3, generator=g)
    rq = Rotation3D(quat, "quat").convert("rmat")
    r6 = Rotation3D(d6, "rmat")
    mg.save("rmat_transforms", quat=mg.npy(quat), d6=mg.npy(d6), pc=mg.npy(pc), trans=mg.npy(trans),
            quat_rmat=mg.npy(rq.rot), d6_rmat=mg.npy(r6.rot),
            rmat_transform=mg.npy(transform_pc(trans, r6, pc)),
            to_euler=mg.npy(r6.to_euler(to_degree=True)), to_quat=mg.npy(r6.to_quat()))


def _model_step(name, cfg, data, seed, extra=None):
    """The float32 half of make_golden._model_step: the reference cannot run its rmat path in float64 (Rotation3D casts
    every rotation to float32, and `r @ v` then meets float64 points: transforms.py:171), so no `grad64` anchor is
    recorded here."""
    from multi_part_assembly.models import build_model
    import param_fill

    torch.manual_seed(seed)
    model = build_model(cfg)
    param_fill.fill_parameters(model, seed)
    mg.zero_dropout(model)
    out = {f"data.{k}": mg.npy(v) for k, v in data.items()}
    out["seed"] = np.array([seed])
    out["names"] = np.array(sorted(model.state_dict().keys()))
    out["shapes"] = np.array([str(tuple(model.state_dict()[k].shape)) for k in sorted(model.state_dict().keys())])
    out.update(extra or {})
    model.train()
    torch.manual_seed(seed + 1)
    loss_dict = model.forward_pass({k: v.clone() for k, v in data.items()}, mode="val", optimizer_idx=-1)
    loss_dict["loss"].backward()
    for k, v in loss_dict.items():
        if torch.is_tensor(v):
            out[f"loss.{k}"] = mg.npy(v)
    for k, p in model.named_parameters():
        if p.grad is not None:
            out.update(param_fill.compact("grad.", k, mg.npy(p.grad)))
    mg.save(name, **out)


def _rmat(cfg):
    cfg.model.rot_type = "rmat"
    return cfg


def gen_pn_transformer_step():
    cfg = _rmat(mg._load_cfg("configs/pn_transformer/pn_transformer", "pn_transformer-32x1-cosine_400e-everyday"))
    cfg.model.pc_feat_dim, cfg.model.transformer_feat_dim = 64, 128
    cfg.model.transformer_heads, cfg.model.transformer_layers = 4, 2
    cfg.data.max_num_part = 5
    g = torch.Generator().manual_seed(2002)
    data = mg.synthetic_batch(g, 3, 5, 64, [2, 4, 5])
    _model_step("pn_transformer_rmat_step", cfg, data, 2002, {"cfg": np.array([64, 4, 128, 2])})


def gen_dgl_step():
    cfg = _rmat(mg._load_cfg("configs/dgl", "dgl-32x1-cosine_200e-everyday"))
    cfg.model.pc_feat_dim = 64
    cfg.data.max_num_part = 5
    g = torch.Generator().manual_seed(2003)
    data = mg.synthetic_batch(g, 3, 5, 64, [2, 4, 5])
    _model_step("dgl_rmat_step", cfg, data, 2003, {"cfg": np.array([64, 3])})


def gen_global_semantic_step():
    cfg = _rmat(mg._load_cfg("configs/global", "global-32x1-cosine_200e-partnet_chair"))
    cfg.model.pc_feat_dim = 64
    cfg.data.max_num_part = 5
    g = torch.Generator().manual_seed(2004)
    B, P, N = 2, 5, 128
    data = mg.synthetic_batch(g, B, P, N, [4, 5])
    match_ids = torch.tensor([[0, 1, 1, 0, 0], [1, 1, 2, 2, 2]])
    for b in range(B):
        for gid in range(1, int(match_ids[b].max()) + 1):
            members = torch.nonzero(match_ids[b] == gid).flatten().tolist()
            for m in members[1:]:
                data["part_pcs"][b, m] = data["part_pcs"][b, members[0]]
    data["match_ids"] = match_ids
    data["instance_label"] = torch.eye(P)[None].repeat(B, 1, 1) * data["part_valids"][..., None]
    _model_step("global_rmat_semantic_step", cfg, data, 2004, {"cfg": np.array([64])})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    _cross_check_with_scipy()
    shim._install_pytorch3d = _install_with_rmat(shim._install_pytorch3d)
    shim.import_reference()
    todo = {"transforms": gen_transforms, "pn_transformer": gen_pn_transformer_step, "dgl": gen_dgl_step,
            "global": gen_global_semantic_step}
    for name, fn in todo.items():
        if not only or name in only:
            fn()


if __name__ == "__main__":
    main()
