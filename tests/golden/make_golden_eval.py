#!/usr/bin/env python3
"""Generate the evaluation fixtures under tests/golden/ by RUNNING THE REFERENCE:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eval.py

Same setup as make_golden_rmat.py (make_golden.py, _reference_shim.py and every existing fixture stay as they are).

  eval_metrics_v2.npz   utils/eval_utils.py (calc_part_acc, trans_metrics, rot_metrics, calc_connectivity_acc) for
                        quaternion poses and for rot_type='rmat', at B = 4, P = 20, N = 1000 ("big") and at a small
                        ragged shape ("small"); prediction noise scales mix exact, near and far parts; every case has
                        a contact table.  Plus the data of the identity model's evaluation record.
  state_dict_keys.json  the `state_dict` key lists of the reference's models at the presets' settings (names only) and
                        the evaluation-mode `forward_pass` results of its identity model.

A comparison at a decision threshold, or at the pole of asin, would test rounding and the intrinsic rather than the code
under test, so the generator asserts in float64 — redrawing its seed until all hold — that
  * no valid part's per-part Chamfer value lies within 1 % of 0.01,
  * no contact's distance lies within 1 % of 0.01 (for the predicted and for the zero poses),
  * every valid part of both rotation sets has |2 (w y - x z)| <= 0.99.
"""
from __future__ import annotations

import json
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
import make_golden_rmat as mr  # noqa: E402

SCALES = (0.0, 0.003, 0.02, 0.3, 1.0)  # prediction noise per part slot, cycled: exact, near, ..., far
CASES = {"big": (4, 20, 1000, [20, 9, 5, 2]), "small": (3, 5, 37, [2, 5, 3])}


def _pose64(q, t, pts):
    """Float64 posed points: quaternion_apply of the (unnormalised) quaternion, then the translation."""
    return shim.quaternion_apply(q.double()[..., None, :].expand(*pts.shape[:-1], 4), pts.double()) + t.double()[..., None, :]


def _margin(values):
    """Smallest distance of a float64 value from the 0.01 threshold, relative to the threshold."""
    return float(((values - 0.01).abs() / 0.01).min())


def _pole(q, valid):
    """Largest |2 (w y - x z)| (the argument of asin) over the valid parts, float64."""
    w, x, y, z = q.double().unbind(-1)
    return float((2 * (w * y - x * z)).abs()[valid].max())


def _conditions(d):
    """The three conditions of the module docstring on a draw's float64 figures."""
    return d["chamfer_margin"] > 0.01 and d["contact_margin"] > 0.01 and d["asin_arg_max"] <= 0.99


def _contacts64(contact, q, t):
    """Float64 minimum squared distance of every annotated contact under the poses (q, t): eval_utils.py:63-105."""
    signs = torch.tensor([[sx, sy, sz] for sx in (1.0, -1.0) for sy in (1.0, -1.0) for sz in (1.0, -1.0)], dtype=torch.float64)
    out = []
    for b, i, j in torch.nonzero(contact[..., 0] == 1).tolist():
        p1 = _pose64(q[b, i], t[b, i], contact[b, i, j, 1:].double() * signs)
        p2 = _pose64(q[b, j], t[b, j], contact[b, j, i, 1:].double() * signs)
        out.append(((p1[:, None] - p2[None]) ** 2).sum(-1).min())
    return torch.stack(out)


def _draw(seed, B, P, N, parts, U, Rotation3D):
    g = torch.Generator().manual_seed(seed)
    data = mg.synthetic_batch(g, B, P, N, parts)
    pcs, valids = data["part_pcs"], data["part_valids"]
    gt_t, gt_q = data["part_trans"], data["part_quat"]
    scale = torch.tensor([SCALES[p % len(SCALES)] for p in range(P)])[None, :, None]
    pr_t = gt_t + scale * torch.randn(B, P, 3, generator=g) * valids[..., None]
    pr_q = F.normalize(gt_q + scale * torch.randn(B, P, 4, generator=g), dim=-1) * valids[..., None]
    # the matrix form gets predictions of its own (other noise), built from unit quaternions
    pr_q2 = F.normalize(gt_q + scale * torch.randn(B, P, 4, generator=g), dim=-1) * valids[..., None]
    r_gt, r_pr = Rotation3D(gt_q.clone(), rot_type="quat"), Rotation3D(pr_q.clone(), rot_type="quat")
    m_gt, m_pr = r_gt.convert("rmat"), Rotation3D(pr_q2.clone(), rot_type="quat").convert("rmat")
    valid = valids == 1
    sets = {"quat": (r_pr, r_gt, r_pr.rot, r_gt.rot), "rmat": (m_pr, m_gt, m_pr.to_quat(), m_gt.to_quat())}
    asin_arg_max = max(_pole(q, valid) for _, _, qp, qg in sets.values() for q in (qp, qg))
    contact = torch.zeros(B, P, P, 4)
    for b, k in enumerate(parts):
        for i in range(k - 1):  # a chain of contacts; the contact point sits between the two GT centroids
            mid = 0.5 * (gt_t[b, i] + gt_t[b, i + 1])
            for a, c in ((i, i + 1), (i + 1, i)):
                contact[b, a, c, 0] = 1.0
                conj = gt_q[b, a] * torch.tensor([1.0, -1.0, -1.0, -1.0])
                contact[b, a, c, 1:] = U.qrot(conj, mid - gt_t[b, a]) + 0.004 * torch.randn(3, generator=g)
    ident = torch.tensor([1.0, 0, 0, 0]).repeat(B, P, 1)
    chamfer_margin = 1e30
    contact_margin = _margin(_contacts64(contact, ident, torch.zeros_like(pr_t)))  # the zero poses
    for kind, (_, _, qp, qg) in sets.items():
        d = torch.cdist(_pose64(qp, pr_t, pcs)[valid], _pose64(qg, gt_t, pcs)[valid]) ** 2
        cd = d.min(2)[0].mean(1) + d.min(1)[0].mean(1)  # [valid parts]
        chamfer_margin = min(chamfer_margin, _margin(cd))
        contact_margin = min(contact_margin, _margin(_contacts64(contact, qp, pr_t)))
    return dict(pcs=pcs, valids=valids, gt_t=gt_t, pr_t=pr_t, contact=contact, sets=sets, ident=ident,
                chamfer_margin=chamfer_margin, contact_margin=contact_margin, asin_arg_max=asin_arg_max)


def gen_eval_metrics(U):
    from multi_part_assembly.utils import eval_utils as E
    from multi_part_assembly.utils import Rotation3D

    out = {}
    for name, (B, P, N, parts) in CASES.items():
        seed = 3001 if name == "big" else 3501
        d = _draw(seed, B, P, N, parts, U, Rotation3D)
        while not _conditions(d):
            print(f"  {name} seed {seed}: Chamfer margin {d['chamfer_margin']:.4f}, contact margin "
                  f"{d['contact_margin']:.4f}, asin argument {d['asin_arg_max']:.4f} — redrawing")
            seed += 1
            d = _draw(seed, B, P, N, parts, U, Rotation3D)
        # the accepted draw: nothing within 1 % of the 0.01 thresholds, no rotation near the asin pole (float64)
        assert d["chamfer_margin"] > 0.01, (name, seed, d["chamfer_margin"])
        assert d["contact_margin"] > 0.01, (name, seed, d["contact_margin"])
        assert d["asin_arg_max"] <= 0.99, (name, seed, d["asin_arg_max"])
        print(f"{name}: seed {seed}, Chamfer margin {d['chamfer_margin']:.4f}, contact margin {d['contact_margin']:.4f}, "
              f"largest asin argument {d['asin_arg_max']:.4f}")
        out[f"{name}.seed"] = np.array([seed])
        out[f"{name}.margins"] = np.array([d["chamfer_margin"], d["contact_margin"], d["asin_arg_max"]])
        out.update({f"{name}.pcs": mg.npy(d["pcs"]), f"{name}.valids": mg.npy(d["valids"]), f"{name}.gt_t": mg.npy(d["gt_t"]),
                    f"{name}.pr_t": mg.npy(d["pr_t"]), f"{name}.contact_points": mg.npy(d["contact"])})
        for kind, (r_pr, r_gt, _, _) in d["sets"].items():
            pre = f"{name}.{kind}."
            out[pre + "pr_rot"], out[pre + "gt_rot"] = mg.npy(r_pr), mg.npy(r_gt)
            out[pre + "part_acc"] = mg.npy(E.calc_part_acc(d["pcs"], d["pr_t"], d["gt_t"], r_pr, r_gt, d["valids"]))
            for m in ("mse", "rmse", "mae"):
                out[pre + f"trans_{m}"] = mg.npy(E.trans_metrics(d["pr_t"], d["gt_t"], d["valids"], m))
                out[pre + f"rot_{m}"] = mg.npy(E.rot_metrics(r_pr, r_gt, d["valids"], m))
            out[pre + "connectivity_acc_pred"] = mg.npy(E.calc_connectivity_acc(d["pr_t"], r_pr, d["contact"]))
            zero_rot = Rotation3D(d["ident"].clone(), rot_type="quat")
            zero_rot = zero_rot if kind == "quat" else zero_rot.convert("rmat")
            out[pre + "connectivity_acc_zero"] = mg.npy(E.calc_connectivity_acc(torch.zeros_like(d["pr_t"]), zero_rot,
                                                                                d["contact"]))
    return out


PRESETS = {  # preset name of multi_part_assembly_amd.config -> (reference config folder, module, overrides)
    "pn_transformer_everyday": ("configs/pn_transformer/pn_transformer", "pn_transformer-32x1-cosine_400e-everyday", {}),
    "pn_transformer_refine_everyday": ("configs/pn_transformer/pn_transformer_refine",
                                       "pn_transformer_refine-32x1-cosine_400e-everyday", {}),
    "global_everyday": ("configs/global", "global-32x1-cosine_200e-everyday", {}),
    "global_partnet_chair": ("configs/global", "global-32x1-cosine_200e-partnet_chair", {}),
    "dgl_everyday": ("configs/dgl", "dgl-32x1-cosine_200e-everyday", {}),
    "dgl_dgcnn_everyday": ("configs/dgl", "dgl-32x1-cosine_200e-everyday", {"encoder": "dgcnn"}),
    "rgl_net_everyday": ("configs/rgl_net", "rgl_net-32x1-cosine_200e-everyday", {}),
    "lstm_everyday": ("configs/lstm", "lstm-32x1-cosine_200e-everyday", {}),
    "lstm_partnet_chair": ("configs/lstm", "lstm-32x1-cosine_200e-partnet_chair", {}),
    "identity_everyday": ("configs/identity", "identity-32x1-cosine_200e-everyday", {}),
}


def gen_state_dict_keys():
    from multi_part_assembly.models import build_model

    keys = {}
    for preset, (folder, module, over) in PRESETS.items():
        cfg = mg._load_cfg(folder, module)
        for k, v in over.items():
            cfg.model[k] = v
        torch.manual_seed(0)
        keys[preset] = sorted(build_model(cfg).state_dict().keys())
        print(f"{preset}: {len(keys[preset])} keys")
    return keys


def gen_identity_eval():
    """Evaluation-mode `forward_pass` of the reference's identity model (geometric data, min-of-5 over identical samples)."""
    from multi_part_assembly.models import build_model

    cfg = mg._load_cfg("configs/identity", "identity-32x1-cosine_200e-everyday")
    cfg.data.max_num_part = 5
    model = build_model(cfg)
    g = torch.Generator().manual_seed(3101)
    data = mg.synthetic_batch(g, 3, 5, 64, [2, 4, 5])
    model.eval()
    with torch.no_grad():
        res = model.forward_pass({k: v.clone() for k, v in data.items()}, mode="val", optimizer_idx=-1)
    arrays = {f"identity.data.{k}": mg.npy(v) for k, v in data.items()}
    record = {k: (float(v) if torch.is_tensor(v) else v) for k, v in res.items()}
    return arrays, record


def main():
    mr._cross_check_with_scipy()
    shim._install_pytorch3d = mr._install_with_rmat(shim._install_pytorch3d)
    shim.import_reference()
    import multi_part_assembly.utils as U

    arrays = gen_eval_metrics(U)
    ident_arrays, ident_record = gen_identity_eval()
    arrays.update(ident_arrays)
    mg.save("eval_metrics_v2", **arrays)
    doc = {"state_dict_keys": gen_state_dict_keys(),
           "identity_eval": {"preset": "identity_everyday", "max_num_part": 5, "data": "eval_metrics_v2.npz: identity.data.*",
                             "result": ident_record}}
    path = HERE / "state_dict_keys.json"
    path.write_text(json.dumps(doc, indent=1, sort_keys=True) + "\n")
    print(f"wrote {path.name}: {path.stat().st_size / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
