"""Plain numpy restatement of csrc/assemble.hip, the yardstick of tests/test_assemble*.py.

Clouds: float32, every operation rounded once, in the reference's order — pytorch3d's `quaternion_apply` (two raw
Hamilton products, sums left to right) or `r @ v` ((r0 x + r1 y) + r2 z), then `+ t` — the boolean-mask gather of
`sample_assembly` and `colorize_part_pc` (colour k for the k-th valid part).  Meshes: float64 on the float32 poses
widened, results left in float64 (the kernel rounds them to float32 once).
"""
import struct

import numpy as np

f32 = np.float32


def _raw_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (aw * bw - ax * bx - ay * by - az * bz,
            aw * bx + ax * bw + ay * bz - az * by,
            aw * by - ax * bz + ay * bw + az * bx,
            aw * bz + ax * by - ay * bx + az * bw)


def pose_quat(pc, quat, trans):
    """pc [..., N, 3], quat [..., 4], trans [..., 3] float32 -> quaternion_apply(q, p) + t, float32 [..., N, 3]."""
    pc, quat, trans = (np.asarray(a, dtype=f32) for a in (pc, quat, trans))
    q = tuple(quat[..., None, k] for k in range(4))
    p = (np.zeros_like(pc[..., 0]), pc[..., 0], pc[..., 1], pc[..., 2])
    conj = (q[0] * f32(1), q[1] * f32(-1), q[2] * f32(-1), q[3] * f32(-1))
    r = _raw_mul(_raw_mul(q, p), conj)
    out = np.stack([r[1] + trans[..., None, 0], r[2] + trans[..., None, 1], r[3] + trans[..., None, 2]], axis=-1)
    assert out.dtype == f32
    return out


def pose_rmat(pc, rmat, trans):
    """pc [..., N, 3], rmat [..., 3, 3], trans [..., 3] float32 -> r @ p + t, float32 [..., N, 3]."""
    pc, rmat, trans = (np.asarray(a, dtype=f32) for a in (pc, rmat, trans))
    x, y, z = pc[..., 0], pc[..., 1], pc[..., 2]
    rows = []
    for i in range(3):
        r = rmat[..., None, i, :]
        rows.append(((r[..., 0] * x + r[..., 1] * y) + r[..., 2] * z) + trans[..., None, i])
    out = np.stack(rows, axis=-1)
    assert out.dtype == f32
    return out


def assemble_clouds(part_pcs, valids, rot, trans, gt_rot, gt_trans, colors, rot_type):
    """-> (clouds float32 [S + 1, rows, 6] with rows = offsets[B], offsets int64 [B + 1]); slab S is the ground truth."""
    part_pcs, valids = np.asarray(part_pcs, dtype=f32), np.asarray(valids)
    pose = pose_quat if rot_type == "quat" else pose_rmat
    rot, trans = np.asarray(rot, dtype=f32), np.asarray(trans, dtype=f32)
    B, P, N, _ = part_pcs.shape
    S = rot.shape[0]
    valid = valids == 1
    count = valid.sum(axis=1)
    offsets = np.concatenate([[0], np.cumsum(count) * N]).astype(np.int64)
    colors = np.asarray(colors, dtype=f32)
    safe = np.where(valid[..., None, None], part_pcs, f32(0))  # padded slots are never read: any value will do
    slabs = []
    for s in range(S + 1):
        r, t = (rot[s], trans[s]) if s < S else (np.asarray(gt_rot, dtype=f32), np.asarray(gt_trans, dtype=f32))
        keep = valid.reshape(valid.shape + (1,) * (r.ndim - 2))
        ident = np.array([1, 0, 0, 0], dtype=f32) if rot_type == "quat" else np.eye(3, dtype=f32)
        with np.errstate(all="ignore"):
            posed = pose(safe, np.where(keep, r, ident), np.where(valid[..., None], t, f32(0)))
        rows = []
        for b in range(B):
            part = posed[b][valid[b]]                          # [p, N, 3]: the reference's boolean-mask gather
            col = np.zeros((len(part), N, 6), dtype=f32)
            col[:, :, :3] = part
            for k in range(len(part)):
                col[k, :, 3:] = colors[k]
            rows.append(col.reshape(-1, 6))
        slabs.append(np.concatenate(rows, axis=0) if rows else np.zeros((0, 6), dtype=f32))
    return np.stack(slabs), offsets


def to_lists(clouds, offsets):
    """The reference's result structure from `assemble_clouds`' arrays: float64 copies of the float32 rows."""
    S = len(clouds) - 1
    B = len(offsets) - 1
    gt = [clouds[S, offsets[b]:offsets[b + 1]].astype(np.float64) for b in range(B)]
    pred = [[clouds[s, offsets[b]:offsets[b + 1]].astype(np.float64) for s in range(S)] for b in range(B)]
    return gt, pred


def quat_to_rmat(quat):
    """pytorch3d quaternion_to_matrix in float32, |q|^2 summed left to right (csrc/rmat.hip) -> [..., 9]."""
    q = np.asarray(quat, dtype=f32)
    r, i, j, k = (q[..., n] for n in range(4))
    two_s = f32(2) / (((r * r + i * i) + j * j) + k * k)
    one = f32(1)
    return np.stack([one - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), one - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), one - two_s * (i * i + j * j)], axis=-1)


def mesh_pose_parts(tri, part_face_off, slot_part, gt_rmat, gt_trans, pred_rmat, pred_trans):
    """tri float64 [F, 9] (origin, e1, e2) -> (orig, input, pred) float64 [F_sel, 3, 3] and face_off int64 [M + 1]."""
    tri = np.asarray(tri, dtype=np.float64)
    slot_part = np.asarray(slot_part, dtype=np.int64).reshape(-1)
    outs, face_off = ([], [], []), [0]
    for m, part in enumerate(slot_part):
        if part < 0:
            face_off.append(face_off[-1])
            continue
        rows = tri[part_face_off[part]:part_face_off[part + 1]]
        Rg, Rp = (np.asarray(a, dtype=f32).reshape(-1, 3, 3)[m].astype(np.float64) for a in (gt_rmat, pred_rmat))
        Tg, Tp = (np.asarray(a, dtype=f32).reshape(-1, 3)[m].astype(np.float64) for a in (gt_trans, pred_trans))
        v = np.stack([rows[:, 0:3], rows[:, 0:3] + rows[:, 3:6], rows[:, 0:3] + rows[:, 6:9]], axis=1)  # [F, 3, 3]
        d = v - Tg
        inp = np.stack([(Rg[0, k] * d[..., 0] + Rg[1, k] * d[..., 1]) + Rg[2, k] * d[..., 2] for k in range(3)], axis=-1)
        pred = np.stack([((Rp[k, 0] * inp[..., 0] + Rp[k, 1] * inp[..., 1]) + Rp[k, 2] * inp[..., 2]) + Tp[k]
                         for k in range(3)], axis=-1)
        for o, a in zip(outs, (v, inp, pred)):
            o.append(a)
        face_off.append(face_off[-1] + len(rows))
    cat = lambda xs: np.concatenate(xs, axis=0) if xs else np.zeros((0, 3, 3))
    return cat(outs[0]), cat(outs[1]), cat(outs[2]), np.asarray(face_off, dtype=np.int64)


def float32_or_adjacent(got, want64):
    """True where the float32 `got` is the float32 rounding of `want64` or one of its two float32 neighbours."""
    got = np.asarray(got, dtype=f32)
    want = np.asarray(want64, dtype=np.float64).astype(f32)
    return (got == want) | (got == np.nextafter(want, f32(np.inf))) | (got == np.nextafter(want, f32(-np.inf)))


def read_ply(path):
    """A reader for exactly what `write_ply` promises: binary little-endian, float x y z, optional uchar red green blue."""
    blob = open(path, "rb").read()
    head, body = blob.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    count = int(next(l for l in lines if l.startswith("element vertex")).split()[2])
    props = [l.split()[1:] for l in lines if l.startswith("property")]
    assert props[:3] == [["float", "x"], ["float", "y"], ["float", "z"]]
    colour = props[3:] == [["uchar", "red"], ["uchar", "green"], ["uchar", "blue"]]
    assert colour or len(props) == 3
    fmt, size = ("<fffBBB", 15) if colour else ("<fff", 12)
    assert len(body) == count * size
    rows = np.array([struct.unpack_from(fmt, body, size * i) for i in range(count)], dtype=np.float64)
    rows = rows.reshape(count, len(fmt) - 1)
    return rows[:, :3].astype(np.float32), (rows[:, 3:].astype(np.uint8) if colour else None)
