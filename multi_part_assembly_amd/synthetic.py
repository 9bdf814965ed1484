"""On-device synthetic batches with the reference's data_dict contract
(multi_part_assembly/datasets/geometry_data.py:133-207), for benchmarks and tests — the Breaking-Bad
meshes are not available, and the metric is defined on synthetic B x P x 1000 x 3 part clouds.

Per sample: num_parts ~ U{min..max}; every valid part is N points uniform in an axis-aligned box
(half-extents ~ U(lo, hi)^3) around its centroid c ~ U(-0.4, 0.4)^3.  As in `__getitem__`
(:133-146) the part is re-centred (part_trans = c), rotated by a Haar-random rotation R
(part_pcs = R (x - c)) and part_quat is the inverse rotation, real part first, so that
transform_pc(part_trans, part_quat, part_pcs) re-assembles the shape.  Padded slots are all-zero
and valid parts come first (:121-126,175-177).
"""
from __future__ import annotations

import numpy as np
import torch

from .transforms import pose_apply

PRESETS = {
    "everyday": dict(min_parts=2, max_parts=20, half_extent=(0.02, 0.3)),   # breaking_bad/everyday.py:13-14
    "artifact": dict(min_parts=12, max_parts=20, half_extent=(0.01, 0.1)),  # many small parts
}


def make_batch(batch_size, max_parts=20, num_points=1000, preset="everyday", seed=1234,
               device="cuda", num_parts=None):
    """Returns a data_dict of float32 CUDA tensors (+ `num_parts` as a host list).

    `seed` should differ per rank (1234 + rank)."""
    cfg = PRESETS[preset]
    dev = torch.device(device)
    g = torch.Generator(device="cpu").manual_seed(seed)
    B, P, N = batch_size, max_parts, num_points
    if num_parts is None:
        num_parts = torch.randint(cfg["min_parts"], min(cfg["max_parts"], P) + 1, (B,), generator=g).tolist()
    valids = torch.zeros(B, P)
    for b, k in enumerate(num_parts):
        valids[b, :k] = 1.0
    lo, hi = cfg["half_extent"]
    half = torch.rand(B, P, 1, 3, generator=g) * (hi - lo) + lo
    local = (torch.rand(B, P, N, 3, generator=g) * 2 - 1) * half
    local = local - local.mean(dim=2, keepdim=True)
    centroid = torch.rand(B, P, 3, generator=g) * 0.8 - 0.4
    q_rot = torch.nn.functional.normalize(torch.randn(B, P, 4, generator=g), dim=-1)  # Haar on S^3
    v = valids.to(dev)
    local = local.to(dev) * v[..., None, None]
    q_rot = q_rot.to(dev)
    part_pcs = pose_apply(local, q_rot) * v[..., None, None]
    part_quat = q_rot * q_rot.new_tensor([1.0, -1.0, -1.0, -1.0]) * v[..., None]
    ids = torch.arange(P, device=dev, dtype=torch.float32)[None].expand(B, P) * v
    return {
        "part_pcs": part_pcs.contiguous(),
        "part_trans": (centroid.to(dev) * v[..., None]).contiguous(),
        "part_quat": part_quat.contiguous(),
        "part_valids": v,
        "instance_label": torch.zeros(B, P, 0, device=dev),
        "part_label": torch.zeros(B, P, 0, device=dev),
        "part_ids": ids,
        "valid_matrix": v[:, :, None] * v[:, None, :],
        "num_parts": num_parts,
    }


def make_semantic_batch(batch_size, max_parts=2, num_points=1000, seed=1234, device="cuda", num_part_category=57):
    """Semantic-dataset (PartNet-like) stand-in for the plumbing configuration (P = 2, B = 4,
    `match_ids = [1, 1]`): every shape has `max_parts` geometrically identical parts (one cloud, different poses), so
    the GT <-> prediction matching has a real group to permute; `instance_label` is the one-hot part slot
    (partnet_data.py:163-208), `part_label` zero-width (not in the shipped `data_keys`)."""
    batch = make_batch(batch_size, max_parts, num_points, preset="everyday", seed=seed, device=device,
                       num_parts=[max_parts] * batch_size)
    dev = batch["part_pcs"].device
    B, P = batch_size, max_parts
    batch["part_pcs"] = batch["part_pcs"][:, :1].expand(B, P, num_points, 3).contiguous()
    batch["match_ids"] = torch.ones(B, P, dtype=torch.int64, device=dev)
    batch["instance_label"] = torch.eye(P, device=dev)[None].repeat(B, 1, 1)
    return batch


def make_partnet_like_batch(batch_size, max_parts=20, num_points=1000, seed=1234, device="cuda"):
    """Semantic-dataset stand-in at PartNet's shape statistics, with everything the `*_partnet_chair` presets' `data_keys`
    ask for.  Per shape (P = `max_parts` slots, P >= 2), valid parts first:
      * 1 .. min(3, P // 4) groups (at least one) of 2-4 geometrically identical parts — one cloud per group, different
        poses — with `match_ids` 1, 2, ... in slot order and one shared `part_ids` value per group;
      * 0-3 unique parts (`match_ids` 0, a `part_ids` value of their own), as far as the slots allow;
      * padding behind them (all-zero, `part_ids` / `match_ids` 0).
    `instance_label` [B, P, P] is the one-hot rank of a part inside its class (partnet_data.py:163-173), `part_label`
    zero-width, `valid_matrix` the outer product of the validity vector, `contact_points` [B, P, P, 4] a symmetric
    contact flag between consecutive valid parts with the midpoint of their centroids.  A function of the arguments only
    (a private CPU generator)."""
    B, P, N = batch_size, max_parts, num_points
    if P < 2:
        raise ValueError("make_partnet_like_batch: needs at least two part slots")
    g = torch.Generator(device="cpu").manual_seed(seed)
    draw = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
    part_ids = np.zeros((B, P), dtype=np.int64)
    match = np.zeros((B, P), dtype=np.int64)
    source = np.tile(np.arange(P), (B, 1))   # slot whose cloud a slot shares
    num_parts = []
    for b in range(B):
        slot, label = 0, 0
        for group in range(draw(1, max(1, min(3, P // 4)))):
            size = min(draw(2, 4), P - slot)
            if size < 2:
                break
            label += 1
            part_ids[b, slot:slot + size], match[b, slot:slot + size] = label, group + 1
            source[b, slot:slot + size] = slot
            slot += size
        for _ in range(min(draw(0, 3), P - slot)):
            label += 1
            part_ids[b, slot] = label
            slot += 1
        num_parts.append(slot)
    batch = make_batch(B, P, N, preset="everyday", seed=seed, device=device, num_parts=num_parts)
    dev = batch["part_pcs"].device
    src = torch.from_numpy(source).to(dev)
    batch["part_pcs"] = torch.gather(batch["part_pcs"], 1, src[:, :, None, None].expand(B, P, N, 3)).contiguous()
    v = batch["part_valids"]
    batch["part_ids"] = torch.from_numpy(part_ids).to(dev)
    batch["match_ids"] = torch.from_numpy(match).to(dev)
    inst = np.zeros((B, P, P), dtype=np.float32)
    contact = np.zeros((B, P, P, 4), dtype=np.float32)
    centre = batch["part_trans"].cpu().numpy()
    for b in range(B):
        seen = {}
        for p in range(num_parts[b]):
            k = seen.get(part_ids[b, p], 0)
            inst[b, p, k] = 1.0
            seen[part_ids[b, p]] = k + 1
            if p + 1 < num_parts[b]:
                mid = 0.5 * (centre[b, p] + centre[b, p + 1])
                contact[b, p, p + 1] = contact[b, p + 1, p] = (1.0, *mid)
    batch["instance_label"] = torch.from_numpy(inst).to(dev)
    batch["contact_points"] = torch.from_numpy(contact).to(dev)
    batch["valid_matrix"] = v[:, :, None] * v[:, None, :]
    return batch


def make_partnet_like_store(num_shapes, max_parts=20, num_points=1000, seed=1234, num_part_category=20,
                            with_contacts=True, min_parts=2, device="cuda", thre=0.01):
    """A `datasets.PartNetStore` of `num_shapes` shapes at the statistics of `make_partnet_like_batch`, on the host and
    without a dataset: per shape 1 .. min(3, P // 4) groups of 2-4 geometrically identical parts (one centred cloud per
    group, different poses, one shared `geo_part_ids` value >= 1) and 0-3 unique parts, the first of them with
    `geo_part_ids` 0 as in the PartNet files; `part_ids` (semantic labels) uniform in 1 .. `num_part_category`; `sym`
    a 0/1 flag per axis; with `with_contacts` a symmetric contact flag between consecutive parts with the midpoint of
    their translations.  The parts of a shape are NOT sorted by group: their order is shuffled, so equal ids are
    scattered as in the files.  `with_contacts="computed"`: the table `PartNetStore.with_computed_contacts(device, thre)`
    derives from the clouds and poses instead (needs the HIP device).  A function of the arguments only (a private
    generator)."""
    from .datasets import PartNetStore
    if with_contacts not in (True, False, "computed"):
        raise ValueError(f"make_partnet_like_store: with_contacts={with_contacts!r} is not True, False or 'computed'")
    P, N = max_parts, num_points
    if P < 2:
        raise ValueError("make_partnet_like_store: needs at least two part slots")
    rng = np.random.RandomState(seed)
    lo, hi = PRESETS["everyday"]["half_extent"]
    shapes, contacts = [], []
    for _ in range(num_shapes):
        geo, label = [], 0
        for _ in range(rng.randint(1, max(1, min(3, P // 4)) + 1)):
            size = min(rng.randint(2, 5), P - len(geo))
            if size < 2:
                break
            label += 1
            geo += [label] * size
        for k in range(min(rng.randint(0, 4), P - len(geo))):
            label += 1
            geo.append(0 if k == 0 else label)
        geo = np.array(geo, dtype=np.int64)
        while len(geo) < min_parts:
            label += 1
            geo = np.append(geo, label)
        geo = geo[rng.permutation(len(geo))]
        p = len(geo)
        clouds = {}
        for g in np.unique(geo):
            pts = (2.0 * rng.random_sample((N, 3)) - 1.0) * (lo + (hi - lo) * rng.random_sample(3))
            clouds[g] = (pts - pts.mean(0)).astype(np.float32)
        quat = rng.standard_normal((p, 4))
        quat /= np.linalg.norm(quat, axis=1, keepdims=True)
        trans = 0.8 * rng.random_sample((p, 3)) - 0.4
        shapes.append({"part_pcs": np.stack([clouds[g] for g in geo]),
                       "part_poses": np.concatenate([trans, quat], axis=1).astype(np.float32),
                       "part_ids": rng.randint(1, num_part_category + 1, size=p).astype(np.int64),
                       "geo_part_ids": geo,
                       "sym": rng.randint(0, 2, size=(p, 3)).astype(np.float32)})
        c = np.zeros((p, p, 4), dtype=np.float32)
        for i in range(p - 1):
            c[i, i + 1] = c[i + 1, i] = (1.0, *(0.5 * (trans[i] + trans[i + 1])))
        contacts.append(c)
    store = PartNetStore.from_arrays(shapes, shape_ids=1000 + np.arange(num_shapes),
                                     contacts=contacts if with_contacts is True else None, min_num_part=min_parts,
                                     max_num_part=P)
    return store.with_computed_contacts(device=device, thre=thre) if with_contacts == "computed" else store


def write_partnet_folder(store, data_dir, data_fn="Chair.train.npy", level=3):
    """Write a `PartNetStore` as a split in the reference's on-disk format (`data_fn` id list, `shape_data/{id}_level3.npy`
    pickled dicts, `contact_points/pairs_with_contact_points_{id}_level3.npy`), so that `datasets.PartNetBatchProducer`
    really loads files of the same data."""
    import os
    os.makedirs(os.path.join(data_dir, "shape_data"), exist_ok=True)
    np.save(os.path.join(data_dir, data_fn), store.shape_ids)
    if store.has_contacts:
        os.makedirs(os.path.join(data_dir, "contact_points"), exist_ok=True)
    for s, sid in enumerate(store.shape_ids):
        a, b = store.shape_part_off[s], store.shape_part_off[s + 1]
        np.save(os.path.join(data_dir, "shape_data", f"{sid}_level{level}.npy"),
                {"part_pcs": store.pcs[a:b], "part_poses": store.poses[a:b], "part_ids": store.sem_ids[a:b].astype(np.int64),
                 "geo_part_ids": store.geo_ids[a:b].astype(np.int64), "sym": store.sym[a:b]}, allow_pickle=True)
        if store.has_contacts:
            c = store.contacts[store.contact_off[s]:store.contact_off[s + 1]].reshape(b - a, b - a, 4)
            np.save(os.path.join(data_dir, "contact_points", f"pairs_with_contact_points_{sid}_level{level}.npy"), c)


def _uv_sphere(segments, rings):
    """Closed latitude / longitude triangulation of the unit sphere: `segments * (rings - 1) + 2` vertices,
    `2 * segments * (rings - 1)` triangles, outward orientation."""
    theta = np.pi * np.arange(1, rings) / rings
    phi = 2.0 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.sin(theta)[:, None] * np.cos(phi)[None], np.sin(theta)[:, None] * np.sin(phi)[None],
                     np.broadcast_to(np.cos(theta)[:, None], (rings - 1, segments))], axis=-1).reshape(-1, 3)
    verts = np.concatenate([[[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]]])
    j = np.arange(segments)
    jn = (j + 1) % segments
    faces = [np.stack([np.zeros_like(j), 1 + j, 1 + jn], axis=1)]
    for r in range(rings - 2):
        a, b = 1 + r * segments, 1 + (r + 1) * segments
        faces += [np.stack([a + j, b + j, b + jn], axis=1), np.stack([a + j, b + jn, a + jn], axis=1)]
    last, south = 1 + (rings - 2) * segments, len(verts) - 1
    faces.append(np.stack([last + j, np.full_like(j, south), last + jn], axis=1))
    return verts, np.concatenate(faces).astype(np.int64)


def make_fracture_meshes(seed, shapes, parts_per_shape, faces):
    """Seeded stand-ins for the Breaking-Bad part meshes, without files: `shapes` lists of `(vertices float64 [V, 3],
    triangles int64 [F, 3])`, one entry per part.  `parts_per_shape` is one count for every shape or one per shape.
    Every part is a closed mesh of about `faces` triangles (`2 * s * max(1, faces // (2 * s))` with s = max(3,
    round(sqrt(faces / 2))): 5000 -> exactly 5000): a sphere whose radius is perturbed per vertex by up to +-30 %,
    scaled to the 'everyday' half-extents U(0.02, 0.3)^3 and moved to a centre ~ U(-0.4, 0.4)^3.  Uses a private
    generator: numpy's global state is untouched."""
    rng = np.random.RandomState(seed)
    counts = [parts_per_shape] * shapes if np.isscalar(parts_per_shape) else list(parts_per_shape)
    if len(counts) != shapes:
        raise ValueError(f"make_fracture_meshes: {len(counts)} part counts for {shapes} shapes")
    segments = max(3, int(round(np.sqrt(faces / 2.0))))
    rings = max(1, faces // (2 * segments)) + 1
    unit, tri = _uv_sphere(segments, rings)
    lo, hi = PRESETS["everyday"]["half_extent"]
    out = []
    for count in counts:
        parts = []
        for _ in range(int(count)):
            radius = 1.0 + 0.3 * (2.0 * rng.random_sample(len(unit)) - 1.0)
            half = lo + (hi - lo) * rng.random_sample(3)
            centre = 0.8 * rng.random_sample(3) - 0.4
            parts.append((unit * radius[:, None] * half[None] + centre[None], tri.copy()))
        out.append(parts)
    return out
