"""Batch producers: the `data_dict` contract at the entry of the hot path.

Mirrors `GeometryPartDataset` (multi_part_assembly/datasets/geometry_data.py:11-207) and
`PartNetPartDataset` (multi_part_assembly/datasets/partnet_data.py:7-243) plus torch's default collate:
the same keys, shapes and dtypes, batched `[B, ...]` and already on the device.

* Breaking-Bad-style geometry data: the per-part numpy work of `__getitem__` (centroid, recentre, random
  rotation, point shuffle, zero padding, float32 cast) runs for the whole batch in ONE HIP launch
  (`mpa_part_batch_transform`, csrc/batch.hip) on the raw sampled points; the host only draws the random
  rotations and point orders — with the reference's own RNG calls, in its order, so a seeded run reproduces
  the reference's batches — and converts the 3x3 matrices to scalar-first quaternions with scipy exactly as
  the reference does.  Mesh loading + surface sampling (`trimesh`, geometry_data.py:109-131) is a pluggable
  `sampler`: `ObjSurfaceSampler` reads the fracture folders' Wavefront .obj meshes itself and samples them with the
  algorithm trimesh publishes for `trimesh.sample.sample_surface` (area-weighted face pick, folded uniform barycentric
  coordinates, numpy's global RNG in the same call order).  trimesh is a third-party dependency that is neither vendored
  by the reference nor present in this image, so that piece is PARITY UNPINNED (its statistical properties are tested);
  without a sampler the producer raises.
* Device-resident meshes: `MeshStore` parses every part mesh once and packs per-triangle (origin, e1, e2) and per-part
  cumulative areas as float64 device arrays; `DeviceGeometryProducer.batch` then samples, recentres, rotates and casts a
  whole batch in ONE launch (`mpa_mesh_sample_batch`, csrc/mesh_sample.hip) with counter-based Philox randomness on the
  device — the host builds a few [B, P] integer tables per batch and nothing per part.  Same `data_dict`.
* PartNet-style semantic data: the on-disk format is plain numpy (`{category}.{split}.npy` id lists,
  `shape_data/{id}_level3.npy` pickled dicts, `contact_points/pairs_with_contact_points_{id}_level3.npy`);
  the label derivations (`instance_label`, `match_ids`, one-hot `part_label`) are host integer logic.
* Device-resident PartNet data: `PartNetStore` reads a split once and packs it into flat arrays; `DevicePartNetProducer.batch`
  gathers a batch from them and derives every label in ONE launch (`mpa_partnet_gather_batch`, csrc/partnet_gather.hip).
  Same `data_dict` as `PartNetBatchProducer`, which stays the yardstick.

What the four producers and the two stores have in common is written once, ahead of them: `_hip_device` (the "HIP device
only" refusal and the resolved device index), `_check_data_keys`, `_geometry_batch` (the geometry `data_dict` and its key
order, for all three geometry paths), `_StatusWord` (the device word behind `.check()`) and `_ResidentStore` (`.npz`
writer and reader, byte limit, one upload per array and device); `read_partnet_split` is the one reader of a PartNet
split.  `DeviceGeometryProducer` has one launch path (`_run`) fed by a host and a device builder of its slot tables.
"""
from __future__ import annotations

import os
import random
from typing import Callable, Iterable, Sequence

import numpy as np
import torch
from scipy.spatial.transform import Rotation as R

from . import _lib


def _no_sampler(folder):
    raise RuntimeError(
        "GeometryBatchProducer: no mesh sampler configured (trimesh is not available in this image); pass "
        "`sampler=folder -> float64 [p, N, 3]` or call produce() with already sampled part clouds")


def load_obj(path):
    """Wavefront .obj -> (vertices float64 [V, 3], triangles int64 [F, 3]); polygons are fan-triangulated, texture /
    normal indices (`v/vt/vn`) and negative (relative) indices are understood, everything else is ignored."""
    verts, faces = [], []
    with open(path) as f:
        for line in f:
            if line.startswith("v "):
                verts.append([float(t) for t in line.split()[1:4]])
            elif line.startswith("f "):
                idx = []
                for tok in line.split()[1:]:
                    i = int(tok.split("/")[0])
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                for k in range(1, len(idx) - 1):
                    faces.append([idx[0], idx[k], idx[k + 1]])
    return np.asarray(verts, dtype=np.float64).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3)


def triangle_table(vertices, faces):
    """Per triangle: origin = v0, e1 = v1 - v0, e2 = v2 - v0 (float64 [F, 3] each) and area [F] — the quantities the
    surface sampler works on.  `MeshStore` packs exactly these arrays, so a face pick on the device is bit-reproducible
    against `sample_surface_from_uniforms`."""
    tri = np.asarray(vertices, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]   # [F, 3, 3]
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    area = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)
    return tri[:, 0], e1, e2, area


def sample_surface_from_uniforms(vertices, faces, u):
    """The surface sampling of `sample_surface` as a function of its uniforms `u` float64 [count, 3] in [0, 1): column 0
    picks the face — `searchsorted(cumsum(area), u0 * total_area)`, probability proportional to area — and columns 1, 2
    are the lengths (a, b) along the triangle's two edge vectors, reflected to (|a - 1|, |b - 1|) where a + b > 1; the
    point is `(e1 * a + e2 * b) + origin`.  -> float64 [count, 3].  This is the yardstick of the device sampler
    (csrc/mesh_sample.hip), which repeats these float64 operations one by one."""
    u = np.asarray(u, dtype=np.float64)
    if u.ndim != 2 or u.shape[1] != 3:
        raise ValueError(f"sample_surface_from_uniforms: u must be [count, 3], got {u.shape}")
    origin, e1, e2, area = triangle_table(vertices, faces)
    weight_cum = np.cumsum(area)
    face_pick = u[:, 0] * weight_cum[-1]
    face_index = np.searchsorted(weight_cum, face_pick)
    origins = origin[face_index]
    vectors = np.stack([e1[face_index], e2[face_index]], axis=1)   # [count, 2, 3]
    lengths = u[:, 1:, None].copy()                                # [count, 2, 1]
    outside = lengths.sum(axis=1).reshape(-1) > 1.0
    lengths[outside] -= 1.0
    lengths = np.abs(lengths)
    return (vectors * lengths).sum(axis=1) + origins


def sample_surface(vertices, faces, count):
    """`trimesh.sample.sample_surface(mesh, count)[0]` restated from trimesh's published algorithm (trimesh is not in this
    image: parity unpinned): faces are picked with probability proportional to their area by inverting the cumulative
    area with `np.random.random(count)`, and a point inside the picked triangle is `origin + a * e1 + b * e2` with (a, b)
    = `np.random.random((count, 2, 1))`, reflected into the triangle where a + b > 1.  Uses numpy's GLOBAL generator,
    like trimesh, so that `np.random.seed` in the caller governs it."""
    face_pick = np.random.random(count)
    lengths = np.random.random((count, 2, 1))
    return sample_surface_from_uniforms(vertices, faces, np.concatenate([face_pick[:, None], lengths[:, :, 0]], axis=1))


class ObjSurfaceSampler:
    """`GeometryPartDataset._get_pcs` (geometry_data.py:109-131): the sorted mesh files of a fracture folder (shuffled
    with `random.shuffle` if `shuffle_parts`), `num_points` surface samples each -> float64 [p, num_points, 3]."""

    def __init__(self, data_dir, num_points=1000, min_num_part=2, max_num_part=20, shuffle_parts=False):
        self.data_dir, self.num_points = data_dir, num_points
        self.min_num_part, self.max_num_part, self.shuffle_parts = min_num_part, max_num_part, shuffle_parts

    def __call__(self, data_folder):
        folder = os.path.join(self.data_dir, data_folder)
        mesh_files = sorted(os.listdir(folder))
        if not self.min_num_part <= len(mesh_files) <= self.max_num_part:
            raise ValueError(f"{folder}: {len(mesh_files)} parts outside [{self.min_num_part}, {self.max_num_part}]")
        if self.shuffle_parts:
            random.shuffle(mesh_files)
        pcs = []
        for name in mesh_files:
            v, f = load_obj(os.path.join(folder, name))
            pcs.append(sample_surface(v, f, self.num_points))
        return np.stack(pcs, axis=0)


def read_fracture_list(data_dir, data_fn, category="", min_num_part=2, max_num_part=20):
    """`GeometryPartDataset._read_data` (geometry_data.py:48-71): the lines of `data_dir/data_fn` name SHAPE folders
    (`everyday/Bottle/<id>`); each is expanded into its `fractured_*` / `mode_*` sub-folders, and a fracture is kept
    when its number of entries lies in [min_num_part, max_num_part] — the others are skipped, not an error.
    `category` ('' or 'all': every shape) must be one path component of the line.  Returns fracture folders relative
    to `data_dir`, in the reference's order (the list's, then `os.listdir`'s)."""
    wanted = "" if category.lower() == "all" else category
    with open(os.path.join(data_dir, data_fn)) as fh:
        shapes = [line.strip() for line in fh]
    fractures = []
    for shape in shapes:
        if not shape or (wanted and wanted not in shape.split("/")):
            continue
        if not os.path.isdir(os.path.join(data_dir, shape)):
            print(f"{shape} does not exist")
            continue
        for sub in os.listdir(os.path.join(data_dir, shape)):
            if "fractured" in sub or "mode" in sub:
                count = len(os.listdir(os.path.join(data_dir, shape, sub)))
                if min_num_part <= count <= max_num_part:
                    fractures.append(os.path.join(shape, sub))
    return fractures


def _to_device(arr: np.ndarray, device) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(arr))
    if device is not None and torch.device(device).type == "cuda":
        return t.pin_memory().to(device, non_blocking=True)
    return t


# ---- what the producers and the stores share ----------------------------------------------------------------------
def _hip_device(device, who):
    """`device` with its index resolved; RuntimeError, in the name of `who` (the caller and what it runs there: "MeshStore:
    the mesh sampler"), unless it is a HIP device."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{who} runs on the HIP device only (there is no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _check_data_keys(allowed, data_keys):
    """The reference's refusal of a data key it does not know (geometry_data.py:189-201, partnet_data.py:210-241)."""
    for key in data_keys:
        if key not in allowed:
            raise ValueError(f"ERROR: unknown data {key}")


def _geometry_batch(part_pcs, part_quat, part_trans, part_valids, part_ids, data_id, data_keys, contact_thre=0.01):
    """The geometry `data_dict` from its device tensors, in the one key order every geometry producer returns.
    `part_ids` may be None where `data_keys` does not ask for it."""
    (B, P), dev = part_valids.shape, part_valids.device
    out = {
        "part_pcs": part_pcs,
        "part_quat": part_quat,
        "part_trans": part_trans,
        "part_valids": part_valids,
        "data_id": data_id,
        # zero-width labels keep the semantic models' concatenations valid (geometry_data.py:181-187)
        "instance_label": torch.zeros((B, P, 0), dtype=torch.float32, device=dev),
        "part_label": torch.zeros((B, P, 0), dtype=torch.float32, device=dev),
    }
    if "part_ids" in data_keys:
        out["part_ids"] = part_ids
    if "valid_matrix" in data_keys:
        out["valid_matrix"] = part_valids[:, :, None] * part_valids[:, None, :]
    if "contact_points" in data_keys:  # the table of the batch's own clouds and ground-truth poses
        from .contacts import contact_points
        out["contact_points"] = contact_points(part_pcs, part_valids, part_quat, part_trans, thre=contact_thre)
    return out


class _StatusWord:
    """The int32 device word through which a kernel reports what it could not read.  It is allocated at the first launch
    that needs it — outside a graph capture, hence the rule to call `.batch()` once before capturing — and `check` reads
    it, clears it and raises."""

    def __init__(self):
        self.word = None

    def on(self, device):
        if self.word is None:
            self.word = torch.zeros(1, dtype=torch.int32, device=device)
        return self.word

    def check(self, template, what):
        """RuntimeError `template.format(what[code])` if the word holds a code; synchronises."""
        if self.word is None:
            return
        code = int(self.word.item())
        if code:
            self.word.zero_()
            raise RuntimeError(template.format(what.get(code, f"status {code}")))


def _check_store_bytes(nbytes, max_bytes, who, noun):
    if max_bytes is not None and nbytes > max_bytes:
        raise ValueError(f"{who}: {nbytes} bytes of {noun} data exceed max_bytes={max_bytes}")


class _ResidentStore:
    """What `MeshStore` and `PartNetStore` share.  A store names its host arrays in `ARRAYS` (`shape_part_off` among them)
    and those that may be None in `OPTIONAL`; `_meta` / `_from_meta` carry whatever else its .npz holds."""

    ARRAYS, OPTIONAL = (), ()

    def _names(self):
        return self.ARRAYS + tuple(n for n in self.OPTIONAL if getattr(self, n) is not None)

    @property
    def nbytes(self):
        return sum(getattr(self, n).nbytes for n in self._names())

    @property
    def num_shapes(self):
        return len(self.shape_part_off) - 1

    def __len__(self):
        return self.num_shapes

    def _meta(self):
        return {}

    @staticmethod
    def _from_meta(z):
        return {}

    def save(self, path):
        """One .npz of plain arrays (no pickle): the per-file parse is paid once per dataset."""
        with open(path, "wb") as fh:
            np.savez(fh, **{n: getattr(self, n) for n in self._names()}, **self._meta())

    @classmethod
    def load(cls, path, max_bytes=None):
        with np.load(path, allow_pickle=False) as z:
            arrays = [z[n] for n in cls.ARRAYS] + [z[n] if n in z.files else None for n in cls.OPTIONAL]
            return cls(*arrays, **cls._from_meta(z), max_bytes=max_bytes)

    def _on_device(self, device, names):
        """The arrays `names` as tensors on `device` (resolved by `_hip_device`), each uploaded at its first use there;
        None for an optional array the store does not hold."""
        cache = self._device.setdefault(device, {})  # `_device`: {} from the store's __init__
        if names not in cache:  # the first call for this tuple of names: later ones are this one lookup
            for n in names:
                if n not in cache:
                    a = getattr(self, n)
                    cache[n] = None if a is None else torch.from_numpy(a).to(device)
            cache[names] = tuple(cache[n] for n in names)
        return cache[names]


class GeometryBatchProducer:
    """`GeometryPartDataset` + default collate, one HIP launch per batch for the per-part transforms."""

    def __init__(self, num_points=1000, min_num_part=2, max_num_part=20, rot_range=-1, data_keys=("part_ids",),
                 device="cuda", sampler: Callable | None = None, data_list: Sequence[str] = ()):
        self.num_points = num_points
        self.min_num_part = min_num_part
        self.max_num_part = max_num_part
        self.rot_range = rot_range
        self.data_keys = tuple(data_keys)
        _check_data_keys(("part_ids", "valid_matrix"), self.data_keys)
        self.device = torch.device(device)
        self.sampler = sampler or _no_sampler
        self.data_list = list(data_list)

    def __len__(self):
        return len(self.data_list)

    # -- host randomness, in the reference's call order (geometry_data.py:80-100) --------------------------
    def _draw_rotation(self):
        if self.rot_range > 0.0:
            rot_euler = (np.random.rand(3) - 0.5) * 2.0 * self.rot_range
            rot_mat = R.from_euler("xyz", rot_euler, degrees=True).as_matrix()
        else:
            rot_mat = R.random().as_matrix()
        quat = R.from_matrix(rot_mat.T).as_quat()[[3, 0, 1, 2]]  # scalar-first, the inverse rotation
        return rot_mat, quat

    def _draw_order(self, n):
        order = np.arange(n)
        random.shuffle(order)
        return order

    def produce(self, items: Iterable[np.ndarray], data_ids: Sequence[int] | None = None) -> dict:
        """items: per sample a float64 array [p, N, 3] of sampled part points (what `_get_pcs` returns).
        Returns the collated `data_dict` on `self.device`."""
        items = [np.asarray(x, dtype=np.float64) for x in items]
        B, P, N = len(items), self.max_num_part, self.num_points
        raw = np.zeros((B, P, N, 3), dtype=np.float64)
        rot = np.zeros((B, P, 9), dtype=np.float64)
        perm = np.zeros((B, P, N), dtype=np.int32)
        quat = np.zeros((B, P, 4), dtype=np.float32)
        valids = np.zeros((B, P), dtype=np.float32)
        for b, pcs in enumerate(items):
            p = pcs.shape[0]
            if not self.min_num_part <= p <= self.max_num_part or pcs.shape[1:] != (N, 3):
                raise ValueError(f"sample {b}: expected [{self.min_num_part}..{P}, {N}, 3], got {pcs.shape}")
            raw[b, :p] = pcs
            valids[b, :p] = 1.0
            for i in range(p):  # per part: rotation first, then the point order — as __getitem__ does
                rot_mat, q = self._draw_rotation()
                rot[b, i] = rot_mat.reshape(9)
                quat[b, i] = q
                perm[b, i] = self._draw_order(N)
        dev = _hip_device(self.device, "GeometryBatchProducer: the transform")
        with torch.cuda.device(dev):
            d_raw, d_rot, d_perm, d_val = (_to_device(a, dev) for a in (raw, rot, perm, valids))
            part_pcs = torch.empty((B, P, N, 3), dtype=torch.float32, device=dev)
            part_trans = torch.empty((B, P, 3), dtype=torch.float32, device=dev)
            _lib.launch("mpa_part_batch_transform", dev, d_raw, d_rot, d_perm, d_val, B * P, N, part_pcs, part_trans)
        part_ids = None
        if "part_ids" in self.data_keys:
            part_ids = _to_device(np.arange(P, dtype=np.float32)[None] * valids, dev)  # 0..p-1, 0 in padded slots
        data_id = torch.as_tensor(list(range(B)) if data_ids is None else list(data_ids), dtype=torch.int64)
        return _geometry_batch(part_pcs, _to_device(quat, dev), part_trans, d_val, part_ids, data_id, self.data_keys)

    def batch(self, indices: Sequence[int]) -> dict:
        """Sample the fracture folders `data_list[i]` with the configured sampler and produce the batch."""
        return self.produce([self.sampler(self.data_list[i]) for i in indices], data_ids=indices)


# ---- device-resident meshes ---------------------------------------------------------------------------------------
class MeshStore(_ResidentStore):
    """Every part mesh of a list of shapes, parsed once and packed into four flat arrays the device sampler reads
    (csrc/mesh_sample.hip):

    * `tri` float64 [F_total, 9]: per triangle (origin, e1, e2) of `triangle_table`;
    * `cum_area` float64 [F_total]: per part, `np.cumsum` of that part's triangle areas;
    * `part_face_off` int64 [parts_total + 1]: part k owns the faces `part_face_off[k]:part_face_off[k + 1]`;
    * `shape_part_off` int64 [shapes + 1]: shape s owns the parts `shape_part_off[s]:shape_part_off[s + 1]`.

    float64 like the reference pipeline up to its final cast: 80 B per face, `nbytes` in total; with `max_bytes` a store
    that would be larger raises instead of exhausting device memory (stores larger than the device are out of scope).
    Zero-area faces inside a part stay and are never picked (`searchsorted`), except a degenerate FIRST face at a pick of
    exactly 0.  The arrays live on the host; each is uploaded once per device, when a batch first needs it there."""

    ARRAYS = ("tri", "cum_area", "part_face_off", "shape_part_off")

    def __init__(self, tri, cum_area, part_face_off, shape_part_off, max_bytes=None):
        self.tri = np.ascontiguousarray(tri, dtype=np.float64).reshape(-1, 9)
        self.cum_area = np.ascontiguousarray(cum_area, dtype=np.float64).reshape(-1)
        self.part_face_off = np.ascontiguousarray(part_face_off, dtype=np.int64).reshape(-1)
        self.shape_part_off = np.ascontiguousarray(shape_part_off, dtype=np.int64).reshape(-1)
        pf, sp = self.part_face_off, self.shape_part_off
        if (len(pf) < 1 or len(sp) < 1 or pf[0] != 0 or sp[0] != 0 or pf[-1] != len(self.tri)
                or len(self.cum_area) != len(self.tri) or sp[-1] != len(pf) - 1
                or (np.diff(pf) < 1).any() or (np.diff(sp) < 1).any()):
            raise ValueError("MeshStore: inconsistent offsets (every part needs a face, every shape a part)")
        last = self.cum_area[pf[1:] - 1]
        if not (np.isfinite(last) & (last > 0.0)).all():
            raise ValueError("MeshStore: a part with zero (or non-finite) total area cannot be sampled")
        _check_store_bytes(self.nbytes, max_bytes, "MeshStore", "mesh")
        self._device = {}

    @property
    def num_parts(self):
        return len(self.part_face_off) - 1

    @classmethod
    def from_arrays(cls, shapes, min_num_part=2, max_num_part=20, max_bytes=None):
        """shapes: per shape a list of `(vertices [V, 3], triangles [F, 3])`, one per part, in part order."""
        shapes = [list(parts) for parts in shapes]
        faces_total = sum(len(f) for parts in shapes for _, f in parts)
        parts_total = sum(len(parts) for parts in shapes)
        _check_store_bytes(80 * faces_total + 8 * (parts_total + 1) + 8 * (len(shapes) + 1), max_bytes, "MeshStore", "mesh")
        tri, cum, pf, sp = [], [], [0], [0]
        for s, parts in enumerate(shapes):
            if not min_num_part <= len(parts) <= max_num_part:
                raise ValueError(f"shape {s}: {len(parts)} parts outside [{min_num_part}, {max_num_part}]")
            for k, (v, f) in enumerate(parts):
                v, f = np.asarray(v, dtype=np.float64).reshape(-1, 3), np.asarray(f, dtype=np.int64).reshape(-1, 3)
                if len(f) == 0:
                    raise ValueError(f"shape {s} part {k}: a mesh without faces cannot be sampled")
                if f.min() < 0 or f.max() >= len(v):
                    raise ValueError(f"shape {s} part {k}: face index outside the {len(v)} vertices")
                origin, e1, e2, area = triangle_table(v, f)
                c = np.cumsum(area)
                if not (np.isfinite(c[-1]) and c[-1] > 0.0):
                    raise ValueError(f"shape {s} part {k}: zero (or non-finite) total area cannot be sampled")
                tri.append(np.concatenate([origin, e1, e2], axis=1))
                cum.append(c)
                pf.append(pf[-1] + len(f))
            sp.append(sp[-1] + len(parts))
        if not shapes:
            raise ValueError("MeshStore: no shapes")
        return cls(np.concatenate(tri), np.concatenate(cum), pf, sp, max_bytes=max_bytes)

    @classmethod
    def from_folders(cls, data_dir, data_list, min_num_part=2, max_num_part=20, max_bytes=None):
        """The fracture folders `data_dir/data_list[i]`, each holding one .obj per part: sorted file names and part-count
        limits as `ObjSurfaceSampler`, every mesh parsed once with `load_obj`."""
        shapes = []
        for rel in data_list:
            folder = os.path.join(data_dir, rel)
            mesh_files = sorted(os.listdir(folder))
            if not min_num_part <= len(mesh_files) <= max_num_part:
                raise ValueError(f"{folder}: {len(mesh_files)} parts outside [{min_num_part}, {max_num_part}]")
            shapes.append([load_obj(os.path.join(folder, name)) for name in mesh_files])
        return cls.from_arrays(shapes, min_num_part, max_num_part, max_bytes)

    def device_arrays(self, device):
        """(tri, cum_area, part_face_off) as tensors on `device`, uploaded at the first call."""
        device = _hip_device(device, "MeshStore: the mesh sampler")
        return self._on_device(device, ("tri", "cum_area", "part_face_off"))

    def device_shape_part_off(self, device):
        """`shape_part_off` on `device`, uploaded at the first call: what builds a batch's slot table from device indices."""
        return self._on_device(_hip_device(device, "MeshStore: the mesh sampler"), ("shape_part_off",))[0]


MAX_DEVICE_SAMPLE_POINTS = 2048  # the sampled float64 cloud of a part lives in LDS (csrc/mesh_sample.hip)


class DeviceGeometryProducer:
    """`GeometryBatchProducer.batch` + `ObjSurfaceSampler` with the per-part work on the device: the meshes sit in a
    `MeshStore`, and ONE HIP launch per batch (`mpa_mesh_sample_batch`) samples every part's surface, recentres, rotates
    and casts.  `.batch()` returns the `data_dict` of `GeometryBatchProducer.produce` — same keys, shapes and dtypes.
    The host only builds the [B, P] integer tables from the store's offsets and sends them in one pinned copy.

    Randomness (`.batch`) is Philox4x32-10 on the device, stateless: key = `seed`, and slot m of a batch uses the
    64-bit stream `batch_counter * B * P + m` (include/mpa_hip.h has the counter layout), so the same (seed,
    batch_counter, slot) gives the same bits in every run, whichever other shapes share the batch.  It reproduces the
    reference's DISTRIBUTION, not numpy's streams.  The points of a part are NOT shuffled: the N samples are independent
    and identically distributed, so a random permutation of them changes nothing a model can see.  `rot_range <= 0`: a
    uniformly random rotation; `> 0`: Euler angles uniform in [-rot_range, rot_range] degrees, as the reference.
    `shuffle_parts` permutes the parts of each shape with `random.shuffle`, like the reference.

    `.replay` feeds host-drawn uniforms / rotations / point orders through the same kernel, for parity tests.

    The data key `"contact_points"` (not one of the reference's geometry keys: its fracture data carries no contact
    annotation) adds the table `contacts.contact_points` computes from the batch's own sampled clouds and ground-truth
    poses, with `contact_thre` as its bound on the squared distance — one more launch (csrc/contact_points.hip); every
    other entry of the batch is what it is without the key."""

    def __init__(self, store: MeshStore, num_points=1000, min_num_part=2, max_num_part=20, rot_range=-1,
                 data_keys=("part_ids",), seed=0, device="cuda", shuffle_parts=False, contact_thre=0.01):
        if not 1 <= num_points <= MAX_DEVICE_SAMPLE_POINTS:
            raise ValueError(f"DeviceGeometryProducer: num_points={num_points} outside [1, {MAX_DEVICE_SAMPLE_POINTS}]")
        self.store = store
        self.num_points, self.min_num_part, self.max_num_part = num_points, min_num_part, max_num_part
        self.rot_range = float(rot_range)
        self.data_keys = tuple(data_keys)
        _check_data_keys(("part_ids", "valid_matrix", "contact_points"), self.data_keys)
        self.contact_thre = float(contact_thre)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.device = torch.device(device)
        self.shuffle_parts = shuffle_parts
        self.batch_counter = 0  # the default `batch_counter` of the next batch() call
        self._status = _StatusWord()  # of the device-index path (csrc/mesh_sample.hip, mesh_slot_table)

    def __len__(self):
        return self.store.num_shapes

    def _slots(self, indices):
        """indices -> slot_part int64 [B, P] (store part id, -1 in padded slots) and the valid mask [B, P]."""
        off = self.store.shape_part_off
        idx = np.asarray(list(indices), dtype=np.int64).reshape(-1)
        if ((idx < 0) | (idx >= len(off) - 1)).any():
            raise IndexError(f"DeviceGeometryProducer: shape index outside [0, {len(off) - 1})")
        start, count = off[idx], off[idx + 1] - off[idx]
        if ((count < self.min_num_part) | (count > self.max_num_part)).any():
            raise ValueError(f"DeviceGeometryProducer: a shape has a part count outside "
                             f"[{self.min_num_part}, {self.max_num_part}]")
        ar = np.arange(self.max_num_part, dtype=np.int64)[None]
        valid = ar < count[:, None]
        slot = np.where(valid, start[:, None] + ar, -1)
        if self.shuffle_parts:
            for b, p in enumerate(count):
                order = list(range(p))
                random.shuffle(order)
                slot[b, :p] = slot[b, order]
        return slot, valid

    def slot_parts(self, indices):
        """The store part id behind every slot of the batch `indices`: numpy int64 [B, P], -1 in padded slots — what
        `assemble.pose_meshes` needs to find the meshes of a batch's parts.  Refused with `shuffle_parts`: the order
        of a batch already drawn is not kept (evaluation never shuffles)."""
        if self.shuffle_parts:
            raise RuntimeError("DeviceGeometryProducer.slot_parts: with shuffle_parts the slots of a batch are drawn anew "
                               "in every call, so the table would not describe any batch")
        return self._slots(indices)[0]

    def _host_tables(self, dev, indices, stream_ids):
        """The [2, B, P] int64 (slot_part, stream) and float32 (valids, part ids) tables of the host sequence `indices`,
        filled on the host in one pinned buffer and sent in one asynchronous copy."""
        slot, valid = self._slots(indices)
        B, P = len(indices), self.max_num_part
        M = B * P
        host = torch.empty(24 * M, dtype=torch.uint8, pin_memory=True)
        h64 = host[: 16 * M].view(torch.int64).view(2, B, P).numpy()
        h32 = host[16 * M:].view(torch.float32).view(2, B, P).numpy()
        h64[0] = slot
        h64[1] = stream_ids
        h32[0] = valid
        h32[1] = np.arange(P)[None] * valid
        buf = host.to(dev, non_blocking=True)
        return buf[: 16 * M].view(torch.int64).view(2, B, P), buf[16 * M:].view(torch.float32).view(2, B, P)

    def _device_tables(self, dev, indices, batch_counter):
        """The same tables for a device index vector, built by `mpa_mesh_slot_table` from the store's `shape_part_off`;
        what the host builder refuses with an exception is left in the status word here."""
        if indices.dtype != torch.int64 or indices.dim() != 1 or not indices.is_contiguous():
            raise ValueError("DeviceGeometryProducer: device indices must be a contiguous int64 vector")
        if self.shuffle_parts:
            raise ValueError("DeviceGeometryProducer: shuffle_parts draws its part orders on the host (random.shuffle) "
                             "and is not available with device indices")
        B, P = indices.numel(), self.max_num_part
        off, = self.store._on_device(dev, ("shape_part_off",))
        d64 = torch.empty((2, B, P), dtype=torch.int64, device=dev)
        d32 = torch.empty((2, B, P), dtype=torch.float32, device=dev)
        _lib.launch("mpa_mesh_slot_table", dev, off, self.store.num_shapes, indices, B, P, self.min_num_part,
                    self.max_num_part, (int(batch_counter) * B * P) & 0xFFFFFFFFFFFFFFFF, d64[0], d64[1], d32[0], d32[1],
                    self._status.on(dev))
        return d64, d32

    def _run(self, indices, batch_counter=None, replay=None, return_raw=False):
        """One batch: the tables of `indices`, the sampler launch, the `data_dict`.  `replay`: the caller's (uniforms,
        rot, perm, quat) instead of the device's draws."""
        dev = _hip_device(self.device, "DeviceGeometryProducer: the mesh sampler")
        with torch.cuda.device(dev):
            if isinstance(indices, torch.Tensor) and indices.device.type == "cuda":
                data_id = indices
                d64, d32 = self._device_tables(dev, indices, batch_counter)
            else:
                indices = list(indices)
                data_id = torch.as_tensor(indices, dtype=torch.int64)
                B, P = len(indices), self.max_num_part
                streams = 0 if replay else (int(batch_counter) * B * P + np.arange(B * P, dtype=np.int64)).reshape(B, P)
                d64, d32 = self._host_tables(dev, indices, streams)
            (_, B, P), N = d64.shape, self.num_points
            tri, cum, pf = self.store._on_device(dev, ("tri", "cum_area", "part_face_off"))
            part_pcs = torch.empty((B, P, N, 3), dtype=torch.float32, device=dev)
            part_trans = torch.empty((B, P, 3), dtype=torch.float32, device=dev)
            raw = torch.empty((B, P, N, 3), dtype=torch.float64, device=dev) if return_raw else None
            if replay:
                d_uni, d_rot, d_perm, part_quat = (_to_device(a, dev) for a in replay)
                args = (d_uni, d_rot, d_perm, 0, None, 0.0, part_pcs, part_trans, None)
            else:
                part_quat = torch.empty((B, P, 4), dtype=torch.float32, device=dev)
                args = (None, None, None, self.seed, d64[1], self.rot_range, part_pcs, part_trans, part_quat)
            _lib.launch("mpa_mesh_sample_batch", dev, tri, cum, pf, self.store.num_parts, d64[0], B * P, N, *args, raw)
        out = _geometry_batch(part_pcs, part_quat, part_trans, d32[0], d32[1], data_id, self.data_keys, self.contact_thre)
        return (out, raw) if return_raw else out

    def check(self):
        """RuntimeError if a device-index batch since the last check held a shape index outside the store or a shape whose
        part count is outside [min_num_part, max_num_part]; synchronises.  The word is cleared as it is reported."""
        self._status.check("DeviceGeometryProducer: a batch met {}; that shape was written as padding",
                           {1: "a shape index outside the store",
                            2: f"a shape with a part count outside [{self.min_num_part}, {self.max_num_part}]"})

    def batch(self, indices: Sequence[int], batch_counter: int | None = None, return_raw=False):
        """The `data_dict` of the shapes `indices`, sampled, rotated and cast on the device.  `batch_counter` selects the
        random streams (default: the number of batches drawn so far); with `return_raw` also the sampled float64 cloud
        [B, P, N, 3] before the transform, as a second result.

        `indices`: a host sequence, or a device int64 vector (for instance a batch of `sampler.EpochSampler`): then the
        slot table is built on the device too, `data_id` is that vector, the bits are those of the host sequence with
        the same values, and a bad index is reported by `check()` instead of an exception here (the host never sees
        the values).  `shuffle_parts` is refused with device indices."""
        if batch_counter is None:
            batch_counter = self.batch_counter
            self.batch_counter += 1
        return self._run(indices, batch_counter, return_raw=return_raw)

    def replay(self, indices: Sequence[int], uniforms, rot, perm, quat, return_raw=False):
        """Replay mode: uniforms float64 [B, P, N, 3], rot float64 [B, P, 9], perm int32 [B, P, N] and quat float32
        [B, P, 4] drawn by the caller (as `GeometryBatchProducer` draws rot / perm / quat).  `part_pcs` and `part_trans`
        are bit-equal to `GeometryBatchProducer.produce` on the clouds `sample_surface_from_uniforms` computes."""
        indices = list(indices)
        B, P, N = len(indices), self.max_num_part, self.num_points
        uniforms = np.ascontiguousarray(uniforms, dtype=np.float64)
        rot = np.ascontiguousarray(rot, dtype=np.float64)
        perm = np.ascontiguousarray(perm, dtype=np.int32)
        quat = np.ascontiguousarray(quat, dtype=np.float32)
        for name, arr, shape in (("uniforms", uniforms, (B, P, N, 3)), ("rot", rot, (B, P, 9)),
                                 ("perm", perm, (B, P, N)), ("quat", quat, (B, P, 4))):
            if arr.shape != shape:
                raise ValueError(f"replay: {name} must be {shape}, got {arr.shape}")
        if perm.size and (perm.min() < 0 or perm.max() >= N):
            raise ValueError(f"replay: perm entries outside [0, {N})")
        return self._run(indices, replay=(uniforms, rot, perm, quat), return_raw=return_raw)


# ---- PartNet ---------------------------------------------------------------------------------------------------
def instance_labels(geo_part_ids: np.ndarray, max_num_part: int) -> np.ndarray:
    """One-hot rank of every part among the geometrically equivalent parts before it (partnet_data.py:160-170):
    `[0,4,4,4,1]` -> ranks `[0,0,1,2,0]`."""
    ids = np.asarray(geo_part_ids).astype(np.int64)
    p = ids.shape[0]
    same_before = (ids[None, :] == ids[:, None]) & (np.arange(p)[None, :] < np.arange(p)[:, None])
    out = np.zeros((max_num_part, max_num_part), dtype=np.float32)
    out[np.arange(p), same_before.sum(1)] = 1.0
    return out


def match_ids(geo_part_ids: np.ndarray, max_num_part: int) -> np.ndarray:
    """Groups of >= 2 equivalent parts numbered 1, 2, ... in increasing id order; everything else (unique ids,
    id 0, padding) is 0 (partnet_data.py:194-208).  The device-side matching draw (`cfg.loss.match_sample = "device"`,
    `matching.static_groups`) runs a static max_num_part // 2 group slots and would leave a larger id unmatched: every
    group has two members or more, so none can occur — checked here, on the host, not inside the step."""
    ids = np.zeros(max_num_part, dtype=np.float32)
    ids[: len(geo_part_ids)] = geo_part_ids
    out = np.zeros_like(ids)
    values, counts = np.unique(ids[ids >= 1], return_counts=True)  # ascending, like the reference's range(1, max+1)
    for label, v in enumerate(values[counts >= 2], start=1):
        out[ids == v] = label
    if out.max() > max(1, max_num_part // 2):
        raise ValueError(f"match_ids: group id {int(out.max())} exceeds max_num_part // 2 = {max_num_part // 2}")
    return out


PARTNET_KEYS = ("part_label", "part_ids", "match_ids", "contact_points", "sym", "valid_matrix")


def _load_partnet(data_dir, shape_id, contacts=False):
    """A shape's `shape_data` dict, or with `contacts` its [p, p, 4] contact table, from the reference's files."""
    level = PartNetBatchProducer.LEVEL
    if contacts:
        fn = os.path.join(data_dir, "contact_points", f"pairs_with_contact_points_{shape_id}_level{level}.npy")
        return np.load(fn, allow_pickle=True)
    return np.load(os.path.join(data_dir, "shape_data", f"{shape_id}_level{level}.npy"), allow_pickle=True).item()


def read_partnet_split(data_dir, data_fn, min_num_part=2, max_num_part=20, overfit=-1):
    """`PartNetPartDataset._read_data` and the `overfit` cut (partnet_data.py:36-54): yields (shape id, `shape_data`
    dict) of the split `data_dir/data_fn` in its order, for the shapes with a part count in [min_num_part, max_num_part]
    — the others are skipped, not an error — and with `overfit > 0` the first `overfit` of them only."""
    kept = 0
    for shape_id in np.load(os.path.join(data_dir, data_fn)):
        cur = _load_partnet(data_dir, shape_id)
        if min_num_part <= np.asarray(cur["part_pcs"]).shape[0] <= max_num_part:
            yield shape_id, cur
            kept += 1
            if kept == overfit:
                return


class PartNetBatchProducer:
    """`PartNetPartDataset` + default collate; reads the reference's on-disk format."""

    LEVEL = 3  # fixed in the paper (partnet_data.py:33)

    def __init__(self, data_dir, data_fn, data_keys, num_part_category=20, min_num_part=2, max_num_part=20,
                 shuffle_parts=False, overfit=-1, device="cuda"):
        self.data_dir = data_dir
        self.num_part_category = num_part_category
        self.min_num_part = min_num_part
        self.max_num_part = max_num_part
        self.shuffle_parts = shuffle_parts
        self.data_keys = tuple(data_keys)
        self.device = torch.device(device)
        # only the ids are kept: `item` reads a shape's file again, as the reference does
        self.shape_ids = [s for s, _ in read_partnet_split(data_dir, data_fn, min_num_part, max_num_part, overfit)]

    def __len__(self):
        return len(self.shape_ids)

    def _load(self, shape_id) -> dict:
        return _load_partnet(self.data_dir, shape_id)

    def _pad(self, data) -> np.ndarray:
        data = np.asarray(data)
        out = np.zeros((self.max_num_part,) + data.shape[1:], dtype=np.float32)
        out[: data.shape[0]] = data
        return out

    def item(self, index) -> dict:
        """One sample as host arrays — the dict `PartNetPartDataset.__getitem__` returns."""
        shape_id = self.shape_ids[index]
        cur = self._load(shape_id)
        p = cur["part_pcs"].shape[0]
        if self.shuffle_parts:
            order = np.random.permutation(p)
            cur = {k: np.array(v)[order] for k, v in cur.items()}
        P = self.max_num_part
        pose = self._pad(cur["part_poses"])
        valids = np.zeros(P, dtype=np.float32)
        valids[:p] = 1.0
        geo = np.asarray(cur["geo_part_ids"])
        d = {
            "part_pcs": self._pad(cur["part_pcs"]),
            "part_trans": pose[:, :3],
            "part_quat": pose[:, 3:],
            "part_valids": valids,
            "data_id": index,
            "shape_id": int(shape_id),
            "instance_label": instance_labels(geo, P),
        }
        if "part_label" in self.data_keys:  # labels in the files start from 1
            one_hot = np.zeros((p, self.num_part_category), dtype=np.float32)
            one_hot[np.arange(p), np.asarray(cur["part_ids"]) - 1] = 1.0
            d["part_label"] = self._pad(one_hot)
        else:
            d["part_label"] = np.zeros((P, 0), dtype=np.float32)
        _check_data_keys(PARTNET_KEYS, self.data_keys)  # raised per item, as the reference does
        for key in self.data_keys:
            if key == "part_ids":
                d[key] = self._pad(geo)
            elif key == "match_ids":
                d[key] = match_ids(geo, P)
            elif key == "contact_points":
                out = np.zeros((P, P, 4), dtype=np.float32)
                out[:p, :p] = _load_partnet(self.data_dir, shape_id, contacts=True)
                d[key] = out
            elif key == "sym":
                d[key] = self._pad(cur["sym"])
            elif key == "valid_matrix":
                d[key] = valids[:, None] * valids[None, :]
        return d

    def batch(self, indices: Sequence[int]) -> dict:
        """Default collate of `item(i)` for i in indices, moved to the device."""
        items = [self.item(i) for i in indices]
        out = {}
        for k in items[0]:
            vals = [it[k] for it in items]
            if isinstance(vals[0], np.ndarray):
                out[k] = _to_device(np.stack(vals), self.device)
            else:
                out[k] = torch.as_tensor(vals, dtype=torch.int64)
        return out


# ---- device-resident PartNet data ---------------------------------------------------------------------------------
MAX_DEVICE_PARTS = 64        # one lane per part in csrc/partnet_gather.hip
_MAX_EXACT_ID = 1 << 24      # `part_ids` travels as float32: every id below 2^24 survives the cast


class PartNetStore(_ResidentStore):
    """Every shape of a PartNet split, read once and packed into flat arrays the gather kernel reads
    (csrc/partnet_gather.hip) — the `MeshStore` of the semantic data:

    * `pcs` float32 [parts_total, N, 3], `poses` float32 [parts_total, 7], `sym` float32 [parts_total, 3]: the float32
      cast `PartNetBatchProducer._pad` applies per batch, done once;
    * `geo_ids` int32 [parts_total] (`geo_part_ids`), `sem_ids` int32 [parts_total] (the files' 1-based `part_ids`);
    * `shape_part_off` int64 [S + 1]: shape s owns the parts `shape_part_off[s]:shape_part_off[s + 1]`;
    * `shape_ids` int64 [S];
    * optional `contacts` float32 [sum_s p_s^2, 4] with `contact_off` int64 [S + 1]: per shape its p x p x 4 block.

    Everything the kernel relies on is checked here, once: consistent offsets, `min_num_part <= p <= max_num_part`,
    `sem_ids >= 1`, `0 <= geo_ids < 2^24`, and the group-count check of `match_ids`.  `nbytes` / `max_bytes` as
    `MeshStore`.  The arrays live on the host; `device_arrays(device)` uploads them once per device."""

    ARRAYS = ("pcs", "poses", "sym", "geo_ids", "sem_ids", "shape_part_off", "shape_ids")
    OPTIONAL = ("contacts", "contact_off")
    EVERY = ARRAYS + OPTIONAL

    def __init__(self, pcs, poses, sym, geo_ids, sem_ids, shape_part_off, shape_ids, contacts=None, contact_off=None,
                 min_num_part=2, max_num_part=20, max_bytes=None):
        pcs = np.asarray(pcs)
        if pcs.ndim != 3 or pcs.shape[2] != 3:
            raise ValueError(f"PartNetStore: pcs must be [parts_total, N, 3], got {pcs.shape}")
        self.pcs = np.ascontiguousarray(pcs, dtype=np.float32)
        self.poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 7)
        self.sym = np.ascontiguousarray(sym, dtype=np.float32).reshape(-1, 3)
        geo, sem = np.asarray(geo_ids).reshape(-1), np.asarray(sem_ids).reshape(-1)
        self.shape_part_off = np.ascontiguousarray(shape_part_off, dtype=np.int64).reshape(-1)
        self.shape_ids = np.ascontiguousarray(shape_ids, dtype=np.int64).reshape(-1)
        self.min_num_part, self.max_num_part = int(min_num_part), int(max_num_part)
        off, total = self.shape_part_off, len(self.pcs)
        if (len(off) < 2 or off[0] != 0 or off[-1] != total or len(self.shape_ids) != len(off) - 1
                or any(len(a) != total for a in (self.poses, self.sym, geo, sem))):
            raise ValueError("PartNetStore: inconsistent offsets (shape_part_off must run from 0 to the number of parts, "
                             "with one entry per shape and one more, and every per-part array must have that many rows)")
        count = np.diff(off)
        if (count < self.min_num_part).any() or (count > self.max_num_part).any():
            raise ValueError(f"PartNetStore: a shape has a part count outside [{self.min_num_part}, {self.max_num_part}]")
        if (sem < 1).any() or (sem >= _MAX_EXACT_ID).any():
            raise ValueError("PartNetStore: sem_ids (the files' part_ids) start from 1")
        if (geo < 0).any() or (geo >= _MAX_EXACT_ID).any():
            raise ValueError(f"PartNetStore: geo_ids must lie in [0, {_MAX_EXACT_ID})")
        self.geo_ids = np.ascontiguousarray(geo, dtype=np.int32)
        self.sem_ids = np.ascontiguousarray(sem, dtype=np.int32)
        for s in range(len(count)):  # the static group slots of the device-side matching draw (see `match_ids`)
            try:
                match_ids(self.geo_ids[off[s]:off[s + 1]], self.max_num_part)
            except ValueError as e:
                raise ValueError(f"PartNetStore: shape {s} (id {self.shape_ids[s]}): {e}") from None
        if (contacts is None) != (contact_off is None):
            raise ValueError("PartNetStore: contacts and contact_off come together")
        self.contacts = self.contact_off = None
        if contacts is not None:
            self.contacts = np.ascontiguousarray(contacts, dtype=np.float32).reshape(-1, 4)
            self.contact_off = np.ascontiguousarray(contact_off, dtype=np.int64).reshape(-1)
            want = np.concatenate([[0], np.cumsum(count * count)])
            if len(self.contact_off) != len(want) or (self.contact_off != want).any() or len(self.contacts) != want[-1]:
                raise ValueError("PartNetStore: inconsistent offsets (contact_off must be the running sum of p * p)")
        _check_store_bytes(self.nbytes, max_bytes, "PartNetStore", "part")
        self._device = {}

    @property
    def num_parts(self):
        return len(self.pcs)

    @property
    def num_points(self):
        return self.pcs.shape[1]

    @property
    def has_contacts(self):
        return self.contacts is not None

    @classmethod
    def from_arrays(cls, shapes, shape_ids=None, contacts=None, min_num_part=2, max_num_part=20, max_bytes=None):
        """shapes: per shape a dict with the entries of a `shape_data` file (`part_pcs` [p, N, 3], `part_poses` [p, 7],
        `sym` [p, 3], `geo_part_ids` [p], `part_ids` [p]); `shape_ids` defaults to 0, 1, ...; `contacts`: per shape a
        [p, p, 4] array, or None for a store without contact points."""
        shapes = list(shapes)
        if not shapes:
            raise ValueError("PartNetStore: no shapes")
        pcs = [np.asarray(d["part_pcs"]) for d in shapes]
        if any(a.ndim != 3 or a.shape[2] != 3 for a in pcs) or len({a.shape[1] for a in pcs}) != 1:
            raise ValueError(f"PartNetStore: every shape must hold [p, N, 3] clouds of one N, got "
                             f"{sorted({a.shape[1:] for a in pcs})}")
        count = np.array([len(a) for a in pcs], dtype=np.int64)
        if (count < min_num_part).any() or (count > max_num_part).any():
            raise ValueError(f"PartNetStore: a shape has a part count outside [{min_num_part}, {max_num_part}]")
        _check_store_bytes(int(count.sum()) * (12 * pcs[0].shape[1] + 48), max_bytes, "PartNetStore", "part")
        cat = lambda key, width: np.concatenate(
            [np.asarray(d[key]).reshape((len(a),) + width) for d, a in zip(shapes, pcs)])
        c = co = None
        if contacts is not None:
            contacts = [np.asarray(x) for x in contacts]
            if len(contacts) != len(shapes) or any(x.shape != (p, p, 4) for x, p in zip(contacts, count)):
                raise ValueError("PartNetStore: contacts must hold one [p, p, 4] array per shape")
            c = np.concatenate([x.reshape(-1, 4) for x in contacts])
            co = np.concatenate([[0], np.cumsum(count * count)])
        return cls(np.concatenate(pcs), cat("part_poses", (7,)), cat("sym", (3,)), cat("geo_part_ids", ()),
                   cat("part_ids", ()), np.concatenate([[0], np.cumsum(count)]),
                   np.arange(len(shapes)) if shape_ids is None else shape_ids, c, co,
                   min_num_part=min_num_part, max_num_part=max_num_part, max_bytes=max_bytes)

    @classmethod
    def from_folder(cls, data_dir, data_fn, min_num_part=2, max_num_part=20, overfit=-1, with_contacts=None,
                    max_bytes=None):
        """The split `data_dir/data_fn` in the reference's on-disk format, with the shape filter, the order and the
        `overfit` cut of `PartNetBatchProducer.__init__`; every file is read once.  `with_contacts`: None reads the
        contact files when the `contact_points` folder exists, True requires them, False leaves them out."""
        ids, shapes = [], []
        for s, cur in read_partnet_split(data_dir, data_fn, min_num_part, max_num_part, overfit):
            ids.append(int(s))
            shapes.append(cur)
        if with_contacts is None:
            with_contacts = os.path.isdir(os.path.join(data_dir, "contact_points"))
        contacts = [_load_partnet(data_dir, s, contacts=True) for s in ids] if with_contacts else None
        return cls.from_arrays(shapes, ids, contacts, min_num_part, max_num_part, max_bytes)

    def with_computed_contacts(self, device="cuda", thre=0.01, batch=64):
        """A store of the same shapes whose `contacts` / `contact_off` are computed from its own clouds and poses instead of
        read from the release's contact files: `batch` shapes at a time, padded to `max_num_part`, go through
        `contacts.contact_points` (csrc/contact_points.hip) with `thre` as the bound on the squared distance, and the
        p x p x 4 block of every shape is kept.  Contacts the store already holds are replaced.  `save`, `load` and
        `DevicePartNetProducer` then work as they do for file-borne contacts."""
        device = _hip_device(device, "PartNetStore: the contact search")
        if batch < 1:
            raise ValueError(f"PartNetStore.with_computed_contacts: batch={batch} must be positive")
        from .contacts import contact_points
        off, P, N = self.shape_part_off, self.max_num_part, self.num_points
        count = np.diff(off)
        blocks = []
        for s0 in range(0, self.num_shapes, int(batch)):
            s1 = min(s0 + int(batch), self.num_shapes)
            pcs = np.zeros((s1 - s0, P, N, 3), dtype=np.float32)
            poses = np.zeros((s1 - s0, P, 7), dtype=np.float32)
            valids = np.zeros((s1 - s0, P), dtype=np.float32)
            for b, s in enumerate(range(s0, s1)):
                pcs[b, :count[s]] = self.pcs[off[s]:off[s + 1]]
                poses[b, :count[s]] = self.poses[off[s]:off[s + 1]]
                valids[b, :count[s]] = 1.0
            d_pcs, d_poses, d_val = (_to_device(a, device) for a in (pcs, poses, valids))
            table = contact_points(d_pcs, d_val, d_poses[..., 3:].contiguous(), d_poses[..., :3].contiguous(),
                                   thre=thre).cpu().numpy()
            blocks += [table[b, :count[s], :count[s]].reshape(-1, 4) for b, s in enumerate(range(s0, s1))]
        return PartNetStore(self.pcs, self.poses, self.sym, self.geo_ids, self.sem_ids, off, self.shape_ids,
                            np.concatenate(blocks), np.concatenate([[0], np.cumsum(count * count)]),
                            min_num_part=self.min_num_part, max_num_part=self.max_num_part)

    def _meta(self):
        return {"part_limits": np.array([self.min_num_part, self.max_num_part], dtype=np.int64)}

    @staticmethod
    def _from_meta(z):
        lo, hi = (int(x) for x in z["part_limits"])
        return {"min_num_part": lo, "max_num_part": hi}

    def device_arrays(self, device):
        """name -> tensor on `device` for every array of the store (`contacts` / `contact_off`: None without contact
        points), uploaded at the first call."""
        return dict(zip(self.EVERY, self._on_device(_hip_device(device, "PartNetStore: the gather"), self.EVERY)))


class DevicePartNetProducer:
    """`PartNetBatchProducer.batch` with the data resident on the device: the split sits in a `PartNetStore`, and ONE HIP
    launch per batch (`mpa_partnet_gather_batch`, csrc/partnet_gather.hip) gathers the clouds, poses and symmetries of
    the chosen shapes and derives every label (`part_valids`, `part_ids`, `instance_label`, `match_ids`, `part_label`,
    `valid_matrix`, `shape_id`) on the device.  `.batch()` returns the `data_dict` of the host producer — same keys,
    shapes, dtypes and values; the tensors of the kernel's outputs (`shape_id` among them) are on the device.

    `shuffle_parts` permutes the parts of every shape on the device: a Fisher-Yates shuffle on Philox4x32-10 keyed by
    `seed`, with the batch counter and the sample's position in the batch as the stream (include/mpa_hip.h fixes the
    layout) — the reference's DISTRIBUTION (`np.random.permutation`), not numpy's stream.  `contact_points` stays in
    stored part order under a shuffle, as in the reference, which reads the contact file after its shuffle.
    `.replay` feeds host-drawn orders through the same kernel, for parity tests.

    A shape index the kernel finds outside the store (it can only come from a device tensor: host sequences are checked
    before the launch) reads nothing, yields an all-padding sample and sets a device status word; `.check()` turns it
    into a RuntimeError.  Call `.batch()` once outside a graph capture first: it allocates that word."""

    def __init__(self, store: PartNetStore, data_keys, num_part_category=20, min_num_part=2, max_num_part=20,
                 shuffle_parts=False, seed=0, device="cuda"):
        self.store = store
        self.data_keys = tuple(data_keys)
        _check_data_keys(PARTNET_KEYS, self.data_keys)
        self.num_part_category = int(num_part_category)
        self.min_num_part, self.max_num_part = int(min_num_part), int(max_num_part)
        if not 1 <= self.max_num_part <= MAX_DEVICE_PARTS:
            raise ValueError(f"DevicePartNetProducer: max_num_part={max_num_part} outside [1, {MAX_DEVICE_PARTS}]")
        count = np.diff(store.shape_part_off)
        if (count < self.min_num_part).any() or (count > self.max_num_part).any():
            raise ValueError(f"DevicePartNetProducer: the store holds a shape with a part count outside "
                             f"[{self.min_num_part}, {self.max_num_part}]")
        if "part_label" in self.data_keys and (self.num_part_category < 1
                                               or int(store.sem_ids.max()) > self.num_part_category):
            raise ValueError(f"DevicePartNetProducer: the store holds part label {int(store.sem_ids.max())}, "
                             f"num_part_category is {self.num_part_category}")
        if "contact_points" in self.data_keys and not store.has_contacts:
            raise ValueError("DevicePartNetProducer: contact_points requested from a store without contacts")
        self.shuffle_parts = bool(shuffle_parts)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.device = torch.device(device)
        self.batch_counter = 0  # the default `batch_counter` of the next batch() call
        self._status = _StatusWord()

    def __len__(self):
        return self.store.num_shapes

    def _spec(self, B):
        """key -> (shape, dtype) of every tensor the kernel writes, in the host producer's key order."""
        P, N = self.max_num_part, self.store.num_points
        C = self.num_part_category if "part_label" in self.data_keys else 0
        f32 = torch.float32
        spec = {"part_pcs": ((B, P, N, 3), f32), "part_trans": ((B, P, 3), f32), "part_quat": ((B, P, 4), f32),
                "part_valids": ((B, P), f32), "shape_id": ((B,), torch.int64), "instance_label": ((B, P, P), f32),
                "part_label": ((B, P, C), f32)}
        extra = {"part_ids": (B, P), "match_ids": (B, P), "contact_points": (B, P, P, 4), "sym": (B, P, 3),
                 "valid_matrix": (B, P, P)}
        for key in self.data_keys:
            if key != "part_label":
                spec[key] = (extra[key], f32)
        return spec

    def _indices(self, dev, indices):
        """(the index vector on the device, the batch's `data_id`, the host's copy of the values): a device vector is
        used as it is, and the host never sees its values (None); a host sequence is checked and sent in one pinned copy."""
        if isinstance(indices, torch.Tensor) and indices.device.type == "cuda":
            if indices.dtype != torch.int64 or indices.dim() != 1 or not indices.is_contiguous():
                raise ValueError("DevicePartNetProducer: device indices must be a contiguous int64 vector")
            return indices, indices, None
        host_idx = np.asarray(indices.numpy() if isinstance(indices, torch.Tensor) else list(indices),
                              dtype=np.int64).reshape(-1)
        S = self.store.num_shapes
        if ((host_idx < 0) | (host_idx >= S)).any():
            raise IndexError(f"DevicePartNetProducer: shape index outside [0, {S})")
        pinned = torch.empty(len(host_idx), dtype=torch.int64, pin_memory=True)
        pinned.numpy()[:] = host_idx
        return pinned.to(dev, non_blocking=True), torch.as_tensor(host_idx, dtype=torch.int64), host_idx

    def _replayed_order(self, dev, perm, B, host_idx):
        """The caller's part orders as the int32 [B, P] device table the kernel replays."""
        P = self.max_num_part
        if isinstance(perm, torch.Tensor) and perm.device.type == "cuda":
            if perm.dtype != torch.int32 or tuple(perm.shape) != (B, P) or not perm.is_contiguous():
                raise ValueError(f"replay: a device perm must be contiguous int32 [{B}, {P}]")
            return perm
        h_perm = np.ascontiguousarray(perm, dtype=np.int32)
        if h_perm.shape != (B, P):
            raise ValueError(f"replay: perm must be ({B}, {P}), got {h_perm.shape}")
        if host_idx is not None:  # what the wrapper can see: every row permutes 0..p-1
            count = np.diff(self.store.shape_part_off)[host_idx]
            for b, p in enumerate(count):
                if not np.array_equal(np.sort(h_perm[b, :p]), np.arange(p)):
                    raise ValueError(f"replay: perm[{b}, :{p}] is not a permutation of 0..{p - 1}")
        return _to_device(h_perm, dev)

    def _output_slots(self, dev, B, out):
        """(key -> tensor of the batch, key -> what the kernel writes: None for an empty entry, passed as NULL).  The
        device tensors of `out` that fit are taken as they are, the others are allocated."""
        result, slots = {}, {}
        for key, (shape, dtype) in self._spec(B).items():
            t = None if out is None else out.get(key)
            if t is not None and t.device.type != "cuda":
                t = None  # (a host tensor of a host-built batch, `shape_id`: the kernel cannot write it)
            if t is None:
                t = torch.empty(shape, dtype=dtype, device=dev)
            elif tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"DevicePartNetProducer: out[{key!r}] must be a contiguous {dtype} tensor of shape "
                                 f"{shape} on {dev}")
            result[key] = t
            slots[key] = t if t.numel() else None
        return result, slots

    def _run(self, indices, perm=None, counter=None, out=None, return_order=False):
        """One batch: the indices, the replayed order if there is one, the output slots, the launch."""
        dev = _hip_device(self.device, "DevicePartNetProducer: the gather")
        P = self.max_num_part
        with torch.cuda.device(dev):
            d_idx, data_id, host_idx = self._indices(dev, indices)
            B = d_idx.numel()
            d_perm = None if perm is None else self._replayed_order(dev, perm, B, host_idx)
            counter_val, counter_dev = 0, None
            if isinstance(counter, torch.Tensor):
                if counter.dtype != torch.int64 or counter.numel() != 1 or counter.device.type != "cuda":
                    raise ValueError("DevicePartNetProducer: a device batch_counter must be one int64 word on the device")
                counter_dev = counter
            elif counter is not None:
                counter_val = int(counter) & 0xFFFFFFFFFFFFFFFF
            result, slots = self._output_slots(dev, B, out)
            order = torch.empty((B, P), dtype=torch.int32, device=dev) if return_order else None
            _lib.launch(  # the store's arrays lead the kernel's arguments, in the order of `EVERY`
                "mpa_partnet_gather_batch", dev, *self.store._on_device(dev, PartNetStore.EVERY), self.store.num_shapes,
                d_idx, B, P, self.store.num_points, result["part_label"].shape[2], d_perm,
                1 if (self.shuffle_parts and perm is None) else 0, self.seed, counter_val, counter_dev,
                slots["part_pcs"], slots["part_trans"], slots["part_quat"], slots["part_valids"], slots.get("part_ids"),
                slots["instance_label"], slots.get("match_ids"), slots["part_label"], slots.get("contact_points"),
                slots.get("sym"), slots.get("valid_matrix"), slots["shape_id"], order, self._status.on(dev))
        if out is not None and host_idx is not None:  # the host-side entries of a host-built batch, filled in place
            for key, val in (("data_id", data_id), ("shape_id", self.store.shape_ids[host_idx])):
                t = out.get(key)
                if t is not None and t.device.type == "cpu" and t.dtype == torch.int64 and tuple(t.shape) == (B,):
                    t.copy_(torch.as_tensor(val))
                    if key == "data_id":
                        data_id = t
                    else:
                        result[key] = t
        batch = {}
        for key in ("part_pcs", "part_trans", "part_quat", "part_valids"):
            batch[key] = result.pop(key)
        batch["data_id"] = data_id
        batch.update(result)
        return (batch, order) if return_order else batch

    def batch(self, indices, batch_counter=None, out=None, return_order=False):
        """The `data_dict` of the shapes `indices`, gathered and labelled on the device.

        `indices`: a host sequence (one pinned asynchronous copy; `data_id` is a host tensor, as the host producer's) or a
        device int64 tensor (no host work at all; `data_id` is that tensor).  `batch_counter` selects the random streams
        of `shuffle_parts` (default: the number of batches drawn so far); an int64 device word instead of a number is
        read by the kernel at run time, so that a captured launch draws afresh after the host rewrites it.  `out`: a dict
        of preallocated tensors (for instance `Trainer.static_batch`) — the kernel writes into those of its keys that
        are device tensors, so their data pointers stay, and `Trainer._graph_step` has nothing to copy.  With
        `return_order` also the part order used, int32 [B, P] (-1 in padded slots), as a second result."""
        if batch_counter is None and self.shuffle_parts:
            batch_counter = self.batch_counter
            self.batch_counter += 1
        return self._run(indices, counter=batch_counter, out=out, return_order=return_order)

    def replay(self, indices, perm, out=None):
        """Replay mode: `perm` int32 [B, P], row b holding in its first p entries the order `np.random.permutation(p)`
        gave the caller.  Bit-equal to `PartNetBatchProducer(shuffle_parts=True).batch` under the same draws."""
        return self._run(indices, perm=perm, out=out)

    def check(self):
        """RuntimeError if a launch since the last check met a shape index outside the store (or a replayed order that
        is no permutation); synchronises.  The word is cleared as it is reported."""
        self._status.check("DevicePartNetProducer: a gather launch met {}; that sample was written as padding",
                           {1: "a shape index outside the store", 2: "a replayed part order that is no permutation"})
