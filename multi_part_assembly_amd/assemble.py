"""Assembled shapes for export: posed, coloured part clouds and posed part meshes from predictions — the counterpart
of the reference's `BaseModel.sample_assembly` (models/modules/base_model.py:427-460), of the callback that draws it
(utils/callback.py:19-35) and of scripts/vis.py, over csrc/assemble.hip.

The reference gathers `pred_pcs[j][valid]` per sample and per shape, copies each piece to the host and colours it in a
Python loop: `sample_iter x B` device synchronisations for one figure.  Here `assemble_clouds` is two launches for the
whole batch (no host synchronisation: it can be captured) and `AssembledClouds.to_lists()` one pinned device-to-host
copy; `pose_meshes` poses the triangles of any selection of `MeshStore` parts in one launch.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .rotation import Rotation3D, quat_to_matrix

__all__ = ["AssembledClouds", "assemble_clouds", "rows_to_lists", "assembly_figure", "rank_order", "rank_assemblies", "PosedMeshes",
           "pose_meshes", "write_ply", "write_obj"]

_HEADER_ALIGN = 256  # the clouds start on this boundary behind the offsets of the packed buffer


class AssembledClouds:
    """What `assemble_clouds` wrote: `clouds` fp32 [S + 1, B P N, 6] (slab s < S = prediction s, slab S = ground truth;
    rows (x, y, z, r, g, b); only the first `offsets[B]` rows of a slab are defined), `offsets` int64 [B + 1] (shape b owns
    the rows `offsets[b]:offsets[b + 1]` of every slab) and `num_samples` = S.  Both tensors are views of one device
    buffer, `packed`, so that the host gets everything in one copy."""

    def __init__(self, packed, batch, slots, points, num_samples):
        self.packed, self.num_samples = packed, num_samples
        self.shape = (batch, slots, points)
        head = self.header_bytes(batch)
        self.offsets = packed[: 8 * (batch + 1)].view(torch.int64)
        self.clouds = packed[head:].view(torch.float32).view(num_samples + 1, batch * slots * points, 6)

    @staticmethod
    def header_bytes(batch):
        return -(-8 * (batch + 1) // _HEADER_ALIGN) * _HEADER_ALIGN

    @classmethod
    def empty(cls, batch, slots, points, num_samples, device):
        nbytes = cls.header_bytes(batch) + 24 * (num_samples + 1) * batch * slots * points
        return cls(torch.empty(nbytes, dtype=torch.uint8, device=device), batch, slots, points, num_samples)

    def to_host(self, rows=None):
        """(clouds [S + 1, rows, 6] float32, offsets [B + 1] int64) as numpy views of ONE pinned device-to-host copy.
        The offsets and the slabs travel together.  Without `rows` the copy carries the capacity B P N rows of every
        slab, not only the `offsets[B]` in use: that count is known on the device only, and learning it first would be a
        second copy and a second synchronisation.  A caller that knows a bound on the host (the batch's number of valid
        parts times N, e.g. from its loader) passes it as `rows`; the slabs are then cut to it on the device first."""
        B, cap = self.shape[0], self.clouds.shape[1]
        head = self.header_bytes(B)
        rows = cap if rows is None else max(0, min(int(rows), cap))
        packed = self.packed
        if rows < cap:
            cut = self.clouds[:, :rows].contiguous().view(-1).view(torch.uint8)
            packed = torch.cat([packed[:head], cut])
        host = torch.empty(packed.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(packed, non_blocking=True)
        torch.cuda.current_stream(packed.device).synchronize()
        offsets = host[: 8 * (B + 1)].view(torch.int64).numpy()
        clouds = host[head:].view(torch.float32).view(self.num_samples + 1, rows, 6).numpy()
        if rows < cap and offsets[-1] > rows:
            raise ValueError(f"AssembledClouds.to_host: rows={rows} is no bound, {int(offsets[-1])} rows are in use")
        return clouds, offsets

    def to_lists(self, rows=None):
        """`(gt_pcs_lst, pred_pcs_lst)` in the structure the reference's `sample_assembly` returns: `gt_pcs_lst[b]` and
        `pred_pcs_lst[b][s]` are numpy float64 [p N, 6] holding the float32 values (`np.zeros` upstream).  One
        device-to-host copy; `rows` as in `to_host`."""
        return rows_to_lists(*self.to_host(rows))


def rows_to_lists(clouds, offsets):
    """The host arrays of `AssembledClouds.to_host()` cut into `(gt_pcs_lst, pred_pcs_lst)`."""
    S, B = len(clouds) - 1, len(offsets) - 1
    gt = [clouds[S, offsets[b]:offsets[b + 1]].astype(np.float64) for b in range(B)]
    pred = [[clouds[s, offsets[b]:offsets[b + 1]].astype(np.float64) for s in range(S)] for b in range(B)]
    return gt, pred


def _rot_tensor(rot, rot_type):
    if rot_type is None:
        if not isinstance(rot, Rotation3D):
            raise TypeError("assemble_clouds: pass Rotation3D values, or raw tensors with `rot_type`")
        return rot.rot, rot.rot_type
    return (rot.rot if isinstance(rot, Rotation3D) else rot), rot_type


def assemble_clouds(part_pcs, valids, rot, trans, gt_rot, gt_trans, colors, rot_type=None, out=None):
    """Pose the parts of a batch with S predictions and with the ground truth and lay them out as coloured clouds.

    part_pcs [B, P, N, 3]; valids [B, P] (real iff == 1); rot [S, B, P, 4 | 3, 3] with trans [S, B, P, 3], or one
    prediction [B, P, ...] (S = 1); gt_rot [B, P, 4 | 3, 3], gt_trans [B, P, 3]; colors [C, 3] with C >= P.  Rotations
    are `Rotation3D` values or, with `rot_type`, raw tensors — as in `transform_pc`.  `out`: an `AssembledClouds` of the
    same sizes to write into (a captured call keeps its buffers).  Two launches, nothing read on the host."""
    r, kind = _rot_tensor(rot, rot_type)
    g, gkind = _rot_tensor(gt_rot, rot_type)
    if kind != gkind or kind not in ("quat", "rmat"):
        raise NotImplementedError(f"assemble_clouds: rotations {kind!r} / {gkind!r} are not supported together")
    _lib.require_hip("assemble_clouds", part_pcs, valids, r, trans, g, gt_trans, colors)
    if part_pcs.dim() != 4 or part_pcs.shape[-1] != 3:
        raise RuntimeError(f"assemble_clouds: part_pcs must be [B, P, N, 3], got {tuple(part_pcs.shape)}")
    B, P, N, _ = part_pcs.shape
    tail = (4,) if kind == "quat" else (3, 3)
    if r.dim() == 2 + len(tail):
        r, trans = r[None], trans[None]
    S = r.shape[0]
    if (tuple(r.shape) != (S, B, P) + tail or tuple(trans.shape) != (S, B, P, 3) or tuple(g.shape) != (B, P) + tail
            or tuple(gt_trans.shape) != (B, P, 3) or tuple(valids.shape) != (B, P) or colors.dim() != 2
            or colors.shape[1] != 3):
        raise RuntimeError(f"assemble_clouds: shape mismatch: part_pcs {tuple(part_pcs.shape)}, valids "
                           f"{tuple(valids.shape)}, rot {tuple(r.shape)}, trans {tuple(trans.shape)}, gt_rot "
                           f"{tuple(g.shape)}, gt_trans {tuple(gt_trans.shape)}, colors {tuple(colors.shape)}")
    dev = part_pcs.device
    if out is None:
        out = AssembledClouds.empty(B, P, N, S, dev)
    elif out.shape != (B, P, N) or out.num_samples != S or out.packed.device != dev:
        raise RuntimeError(f"assemble_clouds: `out` holds {out.num_samples} samples of {out.shape}, the call needs {S} of "
                           f"{(B, P, N)}")
    f32 = lambda t: t.detach().to(torch.float32).contiguous()
    _lib.launch("mpa_assemble_clouds" if kind == "quat" else "mpa_assemble_clouds_rmat", dev, f32(part_pcs), f32(valids),
                f32(r), f32(trans), f32(g), f32(gt_trans), f32(colors), S, B, P, N, colors.shape[0], out.offsets,
                out.clouds)
    return out


def assembly_figure(gt, preds):
    """The layout the reference's callback draws (utils/callback.py:26-33): per shape the ground truth shifted by +1.5 in
    x and sample j by -1.5 j, concatenated into one [., 6] array.  `gt` and `preds` as `to_lists()` returns them; the
    inputs are left as they are."""
    figures = []
    for g, samples in zip(gt, preds):
        pieces = [np.array(g, copy=True)]
        pieces[0][:, 0] = pieces[0][:, 0] + 1.5
        for j, p in enumerate(samples):
            p = np.array(p, copy=True)
            p[:, 0] = p[:, 0] - 1.5 * j
            pieces.append(p)
        figures.append(np.concatenate(pieces, axis=0))
    return figures


# ---- ranking (scripts/vis.py:33-58) ---------------------------------------------------------------------------------------
def rank_order(criterion, top=None):
    """Indices of `criterion` [K] in ascending order, equal values in their original order, the first `top` of them."""
    order = torch.sort(criterion, stable=True).indices
    return order if top is None or top < 0 else order[:top]


_RECORD_FIELDS = ("data_id", "criterion", "pred_trans", "pred_quat", "gt_trans", "gt_quat", "part_valids")


@torch.no_grad()
def rank_assemblies(model, batches, top=None):
    """Rank the shapes of `batches` by how well `model` assembles them, best first (scripts/vis.py:33-58): per batch one
    forward in eval mode and `_calc_loss`; the criterion of a shape is `rot_pt_l2_loss + trans_mae`.  Criteria and poses
    stay on the device until every batch is done; then one stable sort, one gather of the first `top` shapes and one
    device-to-host copy.  Returns a list of records {data_id, criterion, pred_trans [P, 3], pred_quat [P, 4] (through
    `to_quat()`), gt_trans, gt_quat, part_valids [P] int64} of numpy values."""
    modes = [(m, m.training) for m in model.modules()]
    model.eval()
    cols = {k: [] for k in _RECORD_FIELDS}
    try:
        for batch in batches:
            batch = model._with_part_rot(batch)
            out = model.forward(batch)
            loss, _ = model._calc_loss(out, batch)
            if "rot_pt_l2_loss" not in loss or "trans_mae" not in loss:
                raise RuntimeError("rank_assemblies: the criterion rot_pt_l2_loss + trans_mae needs geometric data with "
                                   "cfg.loss.use_rot_pt_l2_loss")
            dev = batch["part_pcs"].device
            cols["criterion"].append((loss["rot_pt_l2_loss"] + loss["trans_mae"]).float())
            cols["data_id"].append(torch.as_tensor(batch["data_id"]).to(dev).long())
            cols["pred_trans"].append(out["trans"].float())
            cols["pred_quat"].append(out["rot"].to_quat().float())
            cols["gt_trans"].append(batch["part_trans"].float())
            cols["gt_quat"].append(batch["part_rot"].to_quat().float())
            cols["part_valids"].append(batch["part_valids"].long())
    finally:
        for m, mode in modes:
            m.training = mode
    if not cols["criterion"]:
        return []
    cols = {k: torch.cat(v, dim=0) for k, v in cols.items()}
    order = rank_order(cols["criterion"], top)
    picked = {k: v[order].contiguous() for k, v in cols.items()}
    K = order.shape[0]
    if K == 0:
        return []
    rows = torch.cat([picked[k].view(torch.uint8).reshape(K, -1) for k in _RECORD_FIELDS], dim=1)
    host = torch.empty(rows.shape, dtype=torch.uint8, pin_memory=True)
    host.copy_(rows, non_blocking=True)  # the ranking's one device-to-host copy
    torch.cuda.current_stream(rows.device).synchronize()
    host = host.numpy()
    fields, at = {}, 0
    for k in _RECORD_FIELDS:
        t = picked[k]
        width = t[0].numel() * t.element_size() if K else 0
        dtype = np.int64 if t.dtype == torch.int64 else np.float32
        fields[k] = np.ascontiguousarray(host[:, at:at + width]).view(dtype).reshape((K,) + tuple(t.shape[1:]))
        at += width
    return [{k: (fields[k][i].item() if fields[k][i].ndim == 0 else fields[k][i]) for k in _RECORD_FIELDS}
            for i in range(K)]


# ---- meshes (scripts/vis.py:75-96) ----------------------------------------------------------------------------------------
class PosedMeshes:
    """Triangles of the selected parts, fp32 [F_sel, 3, 3] (vertex triples per face) on the device: `orig` as stored,
    `input` = R_gt^T (v - T_gt) (the part as the network sees it), `pred` = R_pred input + T_pred; slot m owns the rows
    `face_off[m]:face_off[m + 1]` (numpy int64 [M + 1]; empty for a slot without a part)."""

    def __init__(self, orig, input, pred, face_off):
        self.orig, self.input, self.pred, self.face_off = orig, input, pred, face_off

    def to_host(self):
        """The three arrays as numpy float32 [F_sel, 3, 3], in one device-to-host copy."""
        both = torch.stack([self.orig, self.input, self.pred])
        host = torch.empty(both.shape, dtype=both.dtype, pin_memory=True)
        host.copy_(both, non_blocking=True)
        torch.cuda.current_stream(both.device).synchronize()
        return tuple(host.numpy())

    def slot(self, arrays, m):
        """The rows of slot m of every array of `arrays` (as `to_host()` returns them)."""
        a, b = self.face_off[m], self.face_off[m + 1]
        return tuple(x[a:b] for x in arrays)


def _dev_f32(x, dev):
    if isinstance(x, Rotation3D):
        x = x.rot
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x.detach().to(dev, torch.float32).contiguous()


def pose_meshes(store, slot_part, gt_quat, gt_trans, pred_rot, pred_trans, rot_type="quat", out=None):
    """Pose the meshes of `store` (a `datasets.MeshStore`) parts `slot_part` (int64 [...]: store part ids, < 0 = no part)
    in one launch.  gt_quat [..., 4] / gt_trans [..., 3]: the ground-truth poses of the slots (those of slots without a
    part are never read, whatever they hold); pred_rot [..., 4] or [..., 3, 3] by `rot_type`, pred_trans [..., 3].  Arrays or
    tensors, on any device; the leading shapes are flattened.  `out`: a `PosedMeshes` of the same selection to write into.
    Returns `PosedMeshes`."""
    dev = None
    for x in (pred_trans, pred_rot, gt_trans, gt_quat):
        x = x.rot if isinstance(x, Rotation3D) else x
        if torch.is_tensor(x) and x.is_cuda:
            dev = x.device
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError("pose_meshes: runs on the HIP device only (there is no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device())
    slots = (slot_part.detach().cpu().numpy() if torch.is_tensor(slot_part) else np.asarray(slot_part))
    slots = slots.astype(np.int64).reshape(-1)
    M = len(slots)
    if (slots >= store.num_parts).any():
        raise IndexError(f"pose_meshes: part id outside the store's {store.num_parts} parts")
    pf = store.part_face_off
    safe = np.clip(slots, 0, None)
    count = np.where(slots >= 0, pf[safe + 1] - pf[safe], 0)
    face_off = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    F_sel, max_faces = int(face_off[-1]), int(count.max()) if M else 0
    with torch.cuda.device(dev):
        tri, _, d_pf = store.device_arrays(dev)
        host = torch.empty(2 * M + 1, dtype=torch.int64, pin_memory=True)
        host[:M] = torch.from_numpy(slots)
        host[M:] = torch.from_numpy(face_off)
        table = host.to(dev, non_blocking=True)
        gq, gt = _dev_f32(gt_quat, dev).reshape(-1, 4), _dev_f32(gt_trans, dev).reshape(-1, 3)
        pt = _dev_f32(pred_trans, dev).reshape(-1, 3)
        pr = _dev_f32(pred_rot, dev)
        g_rmat = Rotation3D(gq, "quat").to_rmat().reshape(-1, 9)
        if rot_type == "quat":
            p_rmat = quat_to_matrix(pr.reshape(-1, 4)).reshape(-1, 9)
        elif rot_type == "rmat":
            p_rmat = pr.reshape(-1, 9)
        else:
            raise NotImplementedError(f"pose_meshes: rotation {rot_type!r} is not supported")
        if not (len(g_rmat) == len(gt) == len(p_rmat) == len(pt) == M):
            raise RuntimeError(f"pose_meshes: {M} slots, but {len(g_rmat)} / {len(gt)} ground-truth and {len(p_rmat)} / "
                               f"{len(pt)} predicted poses")
        if out is None:
            o, i, p = (torch.empty((F_sel, 3, 3), dtype=torch.float32, device=dev) for _ in range(3))
        else:
            o, i, p = out.orig, out.input, out.pred
            if any(tuple(x.shape) != (F_sel, 3, 3) or x.device != dev or x.dtype != torch.float32 for x in (o, i, p)):
                raise RuntimeError(f"pose_meshes: `out` does not hold [{F_sel}, 3, 3] float32 arrays on {dev}")
        _lib.launch("mpa_mesh_pose_parts", dev, tri, d_pf, store.num_parts, table[:M], table[M:], M, F_sel, max_faces,
                    g_rmat.contiguous(), gt, p_rmat.contiguous(), pt, o, i, p)
    return PosedMeshes(o, i, p, face_off)


# ---- writers ----------------------------------------------------------------------------------------------------------------
def write_ply(path, xyz, rgb=None):
    """Binary little-endian PLY: `x y z` float32 per vertex and, with `rgb` ([n, 3], values 0-255), `red green blue`
    uchar."""
    xyz = np.asarray(xyz, dtype="<f4").reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    props = ["property float x", "property float y", "property float z"]
    if rgb is not None:
        rgb = np.clip(np.rint(np.asarray(rgb, dtype=np.float64).reshape(-1, 3)), 0, 255).astype(np.uint8)
        if len(rgb) != len(xyz):
            raise ValueError(f"write_ply: {len(xyz)} points, {len(rgb)} colours")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        props += ["property uchar red", "property uchar green", "property uchar blue"]
    rows = np.empty(len(xyz), dtype=np.dtype(fields))
    rows["x"], rows["y"], rows["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if rgb is not None:
        rows["red"], rows["green"], rows["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    header = "\n".join(["ply", "format binary_little_endian 1.0", f"element vertex {len(xyz)}", *props, "end_header"]) + "\n"
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(rows.tobytes())


def write_obj(path, triangles):
    """Wavefront .obj of `triangles` [F, 3, 3]: one `v` line per vertex (three per face, not welded; written with the
    shortest text that reads back to the same value) and one `f` line per face."""
    tri = np.asarray(triangles)
    tri = tri.reshape(-1, 3, 3)
    lines = [f"v {float(x)!r} {float(y)!r} {float(z)!r}" for x, y, z in tri.reshape(-1, 3).tolist()]
    lines += [f"f {3 * k + 1} {3 * k + 2} {3 * k + 3}" for k in range(len(tri))]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + ("\n" if lines else ""))
