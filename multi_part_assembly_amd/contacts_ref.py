"""numpy restatement of `mpa_contact_points[_rmat]` (include/mpa_hip.h): the posing of `mpa_pose_apply[_rmat]_forward`
operation by operation in float32, the Chamfer distance form `(dx*dx + dy*dy) + dz*dz`, and an exhaustive search per pair
of real parts whose first minimiser in (a, c) order wins — no prune.  It is the specification the device kernel is held
to, and what `contacts.contact_points` runs for host tensors.  Imports nothing but numpy."""
from __future__ import annotations

import numpy as np

FAR = np.float32(1e32)   # min_dist of the diagonal and of padded slots
MAX_POINTS = 2048        # the kernel's envelope (csrc/contact_points.hip)
MAX_PARTS = 64

_f32 = np.float32


def sanitize_quat(quat):
    """Rotation3D's zero-quaternion rule as `mpa_quat_sanitize` evaluates it: sqrt(((w*w + x*x) + y*y) + z*z) > 0.5 keeps
    the quaternion, everything else becomes the identity.  [..., 4] float32."""
    q = np.asarray(quat, dtype=_f32)
    w, x, y, z = (q[..., k] for k in range(4))
    keep = np.sqrt(((w * w + x * x) + y * y) + z * z) > _f32(0.5)
    return np.where(keep[..., None], q, np.array([1, 0, 0, 0], dtype=_f32))


def _raw_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (aw * bw - ax * bx - ay * by - az * bz,
            aw * bx + ax * bw + ay * bz - az * by,
            aw * by - ax * bz + ay * bw + az * bx,
            aw * bz + ax * by - ay * bx + az * bw)


def pose_quat(pts, quat, trans):
    """`mpa_pose_apply_forward`: pts [N, 3], quat [4] (used as given), trans [3] -> [N, 3], every operation a float32 one
    in the order of csrc/quat.h (the two Hamilton products of pytorch3d's quaternion_apply, then the translation)."""
    pts, q, t = np.asarray(pts, dtype=_f32), np.asarray(quat, dtype=_f32), np.asarray(trans, dtype=_f32)
    zero = np.zeros(len(pts), dtype=_f32)
    qq = tuple(np.full(len(pts), q[k], dtype=_f32) for k in range(4))
    conj = (qq[0] * _f32(1.0), qq[1] * _f32(-1.0), qq[2] * _f32(-1.0), qq[3] * _f32(-1.0))
    r = _raw_mul(_raw_mul(qq, (zero, pts[:, 0], pts[:, 1], pts[:, 2])), conj)
    return np.stack([r[1] + t[0], r[2] + t[1], r[3] + t[2]], axis=1)


def pose_rmat(pts, rmat, trans):
    """`mpa_pose_apply_rmat_forward`: out_i = ((r_i0 x + r_i1 y) + r_i2 z) + t_i in float32 (csrc/mat3.h)."""
    pts, r, t = np.asarray(pts, dtype=_f32), np.asarray(rmat, dtype=_f32).reshape(3, 3), np.asarray(trans, dtype=_f32)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return np.stack([((r[k, 0] * x + r[k, 1] * y) + r[k, 2] * z) + t[k] for k in range(3)], axis=1)


def pair_distances(a, c):
    """d [Na, Nc] float32 between two posed clouds with the Chamfer contract: (dx*dx + dy*dy) + dz*dz, each rounded."""
    dx = a[:, None, 0] - c[None, :, 0]
    dy = a[:, None, 1] - c[None, :, 1]
    dz = a[:, None, 2] - c[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def closest_pair(a, c):
    """(dmin, a*, c*): the lexicographically first minimiser (lowest a, then lowest c) of `pair_distances`."""
    d = pair_distances(a, c)
    flat = int(np.argmin(d))  # the first occurrence in row-major order
    ai, ci = divmod(flat, d.shape[1])
    return d[ai, ci], ai, ci


def contact_points(part_pcs, valids, rot, trans, thre_sq=0.01, samples=None):
    """What `mpa_contact_points[_rmat]` writes: (contact_points [B, P, P, 4] float32, min_dist [B, P, P] float32, index
    [B, P, P] int32).  part_pcs [B, P, N, 3]; valids [B, P] (real iff == 1); rot [B, P, 4] quaternions (the zero-quaternion
    rule is applied here) or [B, P, 3, 3] matrices; trans [B, P, 3]; `thre_sq` is rounded to float32.  Padded slots are
    never read.  `samples`: only these batch rows are evaluated (the others keep the values of an all-padding sample)."""
    pcs, valids = np.asarray(part_pcs, dtype=_f32), np.asarray(valids, dtype=_f32)
    rot, trans = np.asarray(rot, dtype=_f32), np.asarray(trans, dtype=_f32)
    if pcs.ndim != 4 or pcs.shape[3] != 3:
        raise ValueError(f"contact_points: part_pcs must be [B, P, N, 3], got {pcs.shape}")
    B, P, N, _ = pcs.shape
    rmat = rot.shape == (B, P, 3, 3)
    if not rmat and rot.shape != (B, P, 4):
        raise ValueError(f"contact_points: rot must be [B, P, 4] or [B, P, 3, 3], got {rot.shape}")
    if valids.shape != (B, P) or trans.shape != (B, P, 3):
        raise ValueError(f"contact_points: valids {valids.shape} / trans {trans.shape} do not fit {pcs.shape}")
    thre_sq = _f32(thre_sq)
    contact = np.zeros((B, P, P, 4), dtype=_f32)
    min_dist = np.full((B, P, P), FAR, dtype=_f32)
    index = np.full((B, P, P), -1, dtype=np.int32)
    for b in (range(B) if samples is None else samples):
        real = [p for p in range(P) if valids[b, p] == 1]
        if rmat:
            posed = {p: pose_rmat(pcs[b, p], rot[b, p], trans[b, p]) for p in real}
        else:
            posed = {p: pose_quat(pcs[b, p], sanitize_quat(rot[b, p]), trans[b, p]) for p in real}
        for x, i in enumerate(real):
            for j in real[x + 1:]:
                d, a, c = closest_pair(posed[i], posed[j])
                min_dist[b, i, j] = min_dist[b, j, i] = d
                index[b, i, j], index[b, j, i] = a, c
                if d < thre_sq:
                    contact[b, i, j, 0] = contact[b, j, i, 0] = 1.0
                    contact[b, i, j, 1:] = pcs[b, i, a]
                    contact[b, j, i, 1:] = pcs[b, j, c]
    return contact, min_dist, index
