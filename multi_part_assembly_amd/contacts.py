"""Contact points of a batch, computed instead of loaded: the `contact_points [B, P, P, 4]` table that
`eval_utils.calc_connectivity_acc` consumes, from the canonical part clouds and the ground-truth poses, over
csrc/contact_points.hip.

The reference reads the table from the PartNet release's `contact_points/pairs_with_contact_points_*.npy` files
(datasets/partnet_data.py:210-222) and has no code that writes them, so a store without those files — and every
Breaking-Bad batch — had no connectivity accuracy.  include/mpa_hip.h defines the table; `contacts_ref.py` restates it
in numpy.  With the generation bound equal to the bound `calc_connectivity_acc` accepts (0.01 on the squared distance)
the ground-truth poses score exactly 1 on the generated table.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, contacts_ref
from .eval_utils import _warn_once
from .rotation import Rotation3D

__all__ = ["contact_points", "adjacency", "supported"]

MAX_POINTS, MAX_PARTS = contacts_ref.MAX_POINTS, contacts_ref.MAX_PARTS
_PAIR_BUDGET = 1 << 24  # distance evaluations of one step of the composition


def supported(part_pcs):
    """The envelope of csrc/contact_points.hip (include/mpa_hip.h): float32 CUDA clouds [B, P, N, 3] with 1 <= N <= 2048,
    1 <= P <= 64 and 4 B P P < 2^31."""
    return (part_pcs.is_cuda and part_pcs.dtype == torch.float32 and part_pcs.dim() == 4
            and 1 <= part_pcs.shape[2] <= MAX_POINTS and 1 <= part_pcs.shape[1] <= MAX_PARTS
            and 4 * part_pcs.shape[0] * part_pcs.shape[1] ** 2 < 2 ** 31)


def _composed(part_pcs, valids, rot, kind, trans, thre_sq):
    """The definition on library operators, for CUDA tensors outside the kernel's envelope: the pose operator, then per
    step a block of pairs i < j of every sample — the [B, K, N, N] distances with the pinned operation order and one
    arg-min over the flattened (a, c) axis, whose first minimum is the lexicographically first pair."""
    from .transforms import transform_pc
    B, P, N, _ = part_pcs.shape
    dev = part_pcs.device
    real = valids == 1
    clean = torch.where(real[..., None, None], part_pcs, torch.zeros((), device=dev))  # padded slots: read, never used
    pose_r = torch.where(real.reshape(B, P, *([1] * (rot.dim() - 2))), rot, torch.zeros((), device=dev))
    if kind == "quat":
        pose_r = Rotation3D(pose_r, "quat").rot  # the zero-quaternion rule
    posed = transform_pc(torch.where(real[..., None], trans, torch.zeros((), device=dev)), pose_r, clean, rot_type=kind)
    contact = torch.zeros((B, P, P, 4), dtype=torch.float32, device=dev)
    min_dist = torch.full((B, P, P), float(contacts_ref.FAR), dtype=torch.float32, device=dev)
    index = torch.full((B, P, P), -1, dtype=torch.int32, device=dev)
    if B == 0 or P < 2:
        return contact, min_dist, index
    I, J = torch.triu_indices(P, P, offset=1, device=dev)
    step = max(1, _PAIR_BUDGET // max(1, B * N * N))
    rows = torch.arange(B, device=dev)[:, None]
    for k0 in range(0, I.numel(), step):
        i, j = I[k0:k0 + step], J[k0:k0 + step]
        a, c = posed[:, i], posed[:, j]                                   # [B, K, N, 3]
        dx = a[:, :, :, None, 0] - c[:, :, None, :, 0]
        dy = a[:, :, :, None, 1] - c[:, :, None, :, 1]
        dz = a[:, :, :, None, 2] - c[:, :, None, :, 2]
        d = ((dx * dx + dy * dy) + dz * dz).flatten(2)                    # [B, K, N * N]
        flat = d.argmin(dim=2)
        dmin = d.gather(2, flat[..., None]).squeeze(2)
        ai, ci = flat // N, flat % N
        both = real[:, i] & real[:, j]                                    # [B, K]
        touch = both & (dmin < thre_sq)
        pa = clean[rows, i[None], ai]                                     # [B, K, 3]
        pc = clean[rows, j[None], ci]
        zero3 = torch.zeros((), device=dev)
        flag = touch.float()[..., None]
        contact[:, i, j] = torch.cat([flag, torch.where(touch[..., None], pa, zero3)], dim=-1)
        contact[:, j, i] = torch.cat([flag, torch.where(touch[..., None], pc, zero3)], dim=-1)
        far = torch.full((), float(contacts_ref.FAR), device=dev)
        min_dist[:, i, j] = min_dist[:, j, i] = torch.where(both, dmin, far)
        minus = torch.full((), -1, dtype=torch.int32, device=dev)
        index[:, i, j] = torch.where(both, ai.int(), minus)
        index[:, j, i] = torch.where(both, ci.int(), minus)
    return contact, min_dist, index


@torch.no_grad()
def contact_points(part_pcs, valids, rot, trans, thre=0.01, return_dist=False, return_index=False, out=None):
    """The contact table of a batch from its clouds and poses.

    part_pcs [B, P, N, 3] canonical clouds; valids [B, P] (a part is real iff == 1); rot a `Rotation3D` (quat or rmat) or a
    quaternion tensor [B, P, 4]; trans [B, P, 3]; `thre` bounds the SQUARED distance of a contact — the default is the
    number `calc_connectivity_acc` compares squared distances against.  For every pair i < j of real parts the closest
    pair of points between the two posed parts is found (ties: lowest point of i, then lowest point of j); closer than
    `thre`, rows [b, i, j] and [b, j, i] become (1, canonical coordinates of the two points), otherwise zeros.

    Returns contact_points [B, P, P, 4], then with `return_dist` min_dist [B, P, P] (symmetric; 1e32 on the diagonal and
    in padded slots) and with `return_index` index [B, P, P] int32 (-1 there).  `out`: a tuple of tensors to write into,
    in the order of the results (for a captured call).  One launch of csrc/contact_points.hip for float32 CUDA tensors
    inside its envelope (N <= 2048, P <= 64); everything else is composed — from library operators on the device, from
    `contacts_ref` on the host — with one warning."""
    if isinstance(rot, Rotation3D):
        kind, r = rot.rot_type, rot.rot
    else:
        kind, r = "quat", rot
    if part_pcs.dim() != 4 or part_pcs.shape[-1] != 3:
        raise ValueError(f"contact_points: part_pcs must be [B, P, N, 3], got {tuple(part_pcs.shape)}")
    B, P, N, _ = part_pcs.shape
    tail = (4,) if kind == "quat" else (3, 3)
    if (tuple(r.shape) != (B, P) + tail or tuple(valids.shape) != (B, P) or tuple(trans.shape) != (B, P, 3)):
        raise ValueError(f"contact_points: shape mismatch: part_pcs {tuple(part_pcs.shape)}, valids {tuple(valids.shape)}, "
                         f"rot {tuple(r.shape)} ({kind}), trans {tuple(trans.shape)}")
    if N < 1 or P < 1:
        raise ValueError(f"contact_points: need at least one part slot and one point per part, got P={P}, N={N}")
    thre_sq = float(np.float32(thre))
    want = [True, bool(return_dist), bool(return_index)]
    spec = [((B, P, P, 4), torch.float32), ((B, P, P), torch.float32), ((B, P, P), torch.int32)]
    dev = part_pcs.device
    if out is not None:
        out = (out,) if torch.is_tensor(out) else tuple(out)
        if len(out) != sum(want):
            raise ValueError(f"contact_points: `out` holds {len(out)} tensors, the call returns {sum(want)}")
    slots, it = [], iter(out or ())
    for wanted, (shape, dtype) in zip(want, spec):
        t = next(it) if (wanted and out is not None) else None
        if t is not None and (tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous()):
            raise ValueError(f"contact_points: an `out` tensor must be contiguous {dtype} {shape} on {dev}")
        slots.append(t)
    if supported(part_pcs):
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        for k, (shape, dtype) in enumerate(spec):
            if want[k] and slots[k] is None:
                slots[k] = torch.empty(shape, dtype=dtype, device=dev)
        _lib.launch("mpa_contact_points_rmat" if kind == "rmat" else "mpa_contact_points", dev, f32(part_pcs), f32(valids),
                    f32(r), f32(trans), thre_sq, B, P, N, slots[0], slots[1], slots[2], timer=f"contact_points[{B}x{P}x{N}]")
        res = slots
    else:
        _warn_once("contact_points", f"{tuple(part_pcs.shape)} {part_pcs.dtype} {dev.type} clouds are outside "
                   f"csrc/contact_points.hip (float32 CUDA, at most {MAX_POINTS} points per part and {MAX_PARTS} part slots)")
        if part_pcs.is_cuda:
            res = _composed(part_pcs.detach().float(), valids.detach().float(), r.detach().float(), kind,
                            trans.detach().float(), thre_sq)
        else:
            res = [torch.from_numpy(x) for x in contacts_ref.contact_points(
                part_pcs.detach().numpy(), valids.detach().numpy(), r.detach().numpy(), trans.detach().numpy(), thre_sq)]
        for k in range(3):
            if slots[k] is not None:
                slots[k].copy_(res[k])
        res = [slots[k] if slots[k] is not None else res[k] for k in range(3)]
    picked = [res[k] for k in range(3) if want[k]]
    return picked[0] if len(picked) == 1 else tuple(picked)


def adjacency(contact_points):
    """The [B, P, P] 0/1 matrix of the pairs a contact table flags (its first channel == 1), in the table's dtype."""
    return (contact_points[..., 0] == 1).to(contact_points.dtype)
