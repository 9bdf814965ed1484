"""Evaluation metrics of the assembly task — mirrors of the reference's utils/eval_utils.py:12-199 (`calc_part_acc`,
`calc_connectivity_acc`, `trans_metrics`, `rot_metrics`), same names, arguments and [B]
outputs.  Part accuracy runs the per-part Chamfer search on the HIP operator; the rest are small masked reductions.

`calc_connectivity_acc` gathers the contacting pairs with one `nonzero` instead of the reference's B*P*P Python loop
(eval_utils.py:84-96); the pair order — (b, i, j) ascending — is the same, and the result does not depend on it."""
from __future__ import annotations

import math
import warnings

import torch

from . import _lib
from .chamfer import chamfer_distance
from .transforms import transform_pc

METRIC_KEYS = ("part_acc", "trans_mse", "trans_rmse", "trans_mae", "rot_mse", "rot_rmse", "rot_mae")
FUSED_MAX_POINTS = 2048  # csrc/eval_metrics.hip keeps both posed clouds of a part in LDS (include/mpa_hip.h)
_warned = set()


def _warn_once(what, why):
    """The package's single warning per reason when a call leaves the fused kernels for the composition.  (Modules keep
    such a flag on themselves; these are free functions, so the flags live in one module-level set.)"""
    if what not in _warned:
        _warned.add(what)
        warnings.warn(f"{what}: {why}; composing the result from the per-function operators")


def _valid_mean(per_part, valids):
    valids = valids.float().detach()
    return (per_part * valids).sum(1) / valids.sum(1)


@torch.no_grad()
def calc_part_acc(pts, trans1, trans2, rot1, rot2, valids):
    """Fraction of valid parts whose Chamfer distance between the two posed copies is below 0.01 -> [B]."""
    B, P = pts.shape[:2]
    pts1 = transform_pc(trans1, rot1, pts).flatten(0, 1)
    pts2 = transform_pc(trans2, rot2, pts).flatten(0, 1)
    dist1, dist2 = chamfer_distance(pts1, pts2)
    per_part = (dist1.mean(dim=1) + dist2.mean(dim=1)).view(B, P).type_as(pts)
    ok = (per_part < 0.01) & (valids == 1)
    return ok.sum(-1) / (valids == 1).sum(-1)


def _symmetric_copies(points):
    """The 8 sign flips of the xyz coordinates, in the reference's order (x outermost): [n, 3] -> [n, 8, 3]."""
    signs = torch.tensor([[sx, sy, sz] for sx in (1.0, -1.0) for sy in (1.0, -1.0) for sz in (1.0, -1.0)],
                         dtype=points.dtype, device=points.device)
    return points[:, None, :] * signs[None]


@torch.no_grad()
def calc_connectivity_acc(trans, rot, contact_points, fused=False):
    """Fraction of annotated contacts (contact_points[b, i, j, 0] == 1) whose two contact points, moved by the
    predicted poses of parts i and j, come closer than 0.01 (squared distance, minimum over the 8x8 symmetric
    copies) -> the batch-wide value tiled to [B].  `fused=True`: one launch of csrc/eval_metrics.hip on CUDA tensors
    (integer counters, no gather); on the CPU the composition below, with one warning."""
    B = trans.shape[0]
    rot_type, rot = rot.rot_type, rot.rot
    if fused:
        if trans.is_cuda and trans.dtype == torch.float32 and B * trans.shape[1] ** 2 < 2 ** 31:
            return _connectivity_fused(trans, rot, rot_type, contact_points)
        _warn_once("calc_connectivity_acc", "the fused kernel takes float32 CUDA tensors")
    b, i, j = torch.nonzero(contact_points[..., 0] == 1, as_tuple=True)
    p1 = _symmetric_copies(contact_points[b, i, j, 1:])
    p2 = _symmetric_copies(contact_points[b, j, i, 1:])
    p1 = transform_pc(trans[b, i], rot[b, i], p1, rot_type=rot_type)
    p2 = transform_pc(trans[b, j], rot[b, j], p2, rot_type=rot_type)
    dist = ((p1[:, :, None] - p2[:, None, :]) ** 2).sum(-1).flatten(1).min(-1)[0]
    acc = (dist < 0.01).sum().float() / float(dist.numel())
    return torch.ones(B).type_as(trans) * acc


@torch.no_grad()
def trans_metrics(trans1, trans2, valids, metric):
    assert metric in ("mse", "rmse", "mae")
    diff = trans1 - trans2
    if metric == "mae":
        per_part = diff.abs().mean(dim=-1)
    else:
        per_part = diff.pow(2).mean(dim=-1)
        if metric == "rmse":
            per_part = per_part ** 0.5
    return _valid_mean(per_part, valids)


def quat_to_euler_zyx_deg(q):
    """Real-first unit quaternions [..., 4] -> (x, y, z) Euler angles in degrees, 'zyx' convention — the default of
    the reference's `Rotation3D.to_euler` (utils/rotation.py:35-90,201-204)."""
    w, x, y, z = q.unbind(-1)
    ex = torch.atan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y))
    ey = torch.asin(torch.clamp(2 * (w * y - x * z), -1.0, 1.0))
    ez = torch.atan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))
    return torch.stack((ex, ey, ez), dim=-1) * 180.0 / math.pi


@torch.no_grad()
def rot_metrics(rot1, rot2, valids, metric):
    """Euler-angle (degree) error with the wrap at 180 handled -> [B]."""
    assert metric in ("mse", "rmse", "mae")
    d = (quat_to_euler_zyx_deg(rot1.to_quat()) - quat_to_euler_zyx_deg(rot2.to_quat())).abs()
    d = torch.minimum(d, 360.0 - d)
    if metric == "mae":
        per_part = d.abs().mean(dim=-1)
    else:
        per_part = d.pow(2).mean(dim=-1)
        if metric == "rmse":
            per_part = per_part ** 0.5
    return _valid_mean(per_part, valids)


def _connectivity_fused(trans, rot, rot_type, contact_points):
    B, P = trans.shape[:2]
    dev = trans.device
    out = torch.empty(B, dtype=torch.float32, device=dev)
    contact = contact_points.to(torch.float32).contiguous()
    trans, rot = trans.contiguous(), rot.to(torch.float32).contiguous()
    _lib.launch("mpa_connectivity_acc", dev, contact, trans, rot, int(rot_type == "rmat"), B, P, out)
    return out


def fused_metrics_supported(pts):
    """The envelope of csrc/eval_metrics.hip (include/mpa_hip.h): float32 CUDA clouds of at most 2048 points per part."""
    return (pts.is_cuda and pts.dtype == torch.float32 and pts.dim() == 4 and 1 <= pts.shape[2] <= FUSED_MAX_POINTS
            and pts.shape[1] >= 1 and 7 * pts.shape[0] * pts.shape[1] < 2 ** 31)


def _assembly_metrics_composed(pts, pred_trans, gt_trans, pred_rot, gt_rot, valids):
    out = {"part_acc": calc_part_acc(pts, pred_trans, gt_trans, pred_rot, gt_rot, valids)}
    for m in ("mse", "rmse", "mae"):
        out[f"trans_{m}"] = trans_metrics(pred_trans, gt_trans, valids, metric=m)
    for m in ("mse", "rmse", "mae"):
        out[f"rot_{m}"] = rot_metrics(pred_rot, gt_rot, valids, metric=m)
    return out


@torch.no_grad()
def assembly_metrics(pts, pred_trans, gt_trans, pred_rot, gt_rot, valids, ret_per_part=False):
    """The seven per-batch-element metrics of the evaluation step in one call: {part_acc, trans_mse, trans_rmse,
    trans_mae, rot_mse, rot_rmse, rot_mae}, each [B] — `calc_part_acc`, `trans_metrics` and `rot_metrics` of the same
    arguments (pts [B,P,N,3], translations [B,P,3], rotations as Rotation3D of one kind, valids [B,P]).

    Float32 CUDA inputs inside the kernels' envelope (N <= 2048, finite values) take two launches of
    csrc/eval_metrics.hip; everything else — the CPU included — is composed from the seven functions, with one warning.
    `ret_per_part` also returns the [B,P] per-part Chamfer values behind part_acc (fused path only; None otherwise)."""
    if not fused_metrics_supported(pts) or pred_rot.rot_type != gt_rot.rot_type:
        if fused_metrics_supported(pts):
            _warn_once("assembly_metrics", f"a '{pred_rot.rot_type}' prediction against a '{gt_rot.rot_type}' ground truth: "
                       "csrc/eval_metrics.hip takes both rotations in one form")
        else:
            _warn_once("assembly_metrics", f"{tuple(pts.shape)} {pts.dtype} {pts.device.type} clouds are outside "
                       f"csrc/eval_metrics.hip (float32 CUDA, at most {FUSED_MAX_POINTS} points per part)")
        out = _assembly_metrics_composed(pts, pred_trans, gt_trans, pred_rot, gt_rot, valids)
        return (out, None) if ret_per_part else out
    B, P, N = pts.shape[:3]
    dev, f32 = pts.device, torch.float32
    rmat = pred_rot.rot_type == "rmat"
    args = [t.detach().to(f32).contiguous() for t in (pts, pred_trans, gt_trans, pred_rot.rot, gt_rot.rot, valids)]
    ws = torch.empty(max(1, _lib.query("mpa_assembly_metrics_workspace", B, P) // 8), dtype=torch.float64, device=dev)
    out = torch.empty((len(METRIC_KEYS), B), dtype=f32, device=dev)
    per_part = torch.empty((B, P), dtype=f32, device=dev) if ret_per_part else None
    _lib.launch("mpa_assembly_metrics_rmat" if rmat else "mpa_assembly_metrics", dev, *args, B, P, N, ws, out, per_part,
                timer=f"assembly_metrics[{B}x{P}x{N}]")
    res = {k: out[i] for i, k in enumerate(METRIC_KEYS)}
    return (res, per_part) if ret_per_part else res
