"""`MeshStore`, `sample_surface_from_uniforms` and the argument contract of `mpa_mesh_sample_batch`, without a GPU; and the
pure-Python restatements (Philox4x32-10, the uniform construction, the rotation formulas of include/mpa_hip.h) that
tests/test_mesh_sample_gpu.py uses as the oracle of the device-random mode."""
import ctypes

import numpy as np
import pytest

from multi_part_assembly_amd import _build, _lib, datasets, philox_ref, synthetic
from multi_part_assembly_amd.datasets import MeshStore, load_obj, sample_surface, sample_surface_from_uniforms


# ---- oracle restatements (shared with the GPU test) -----------------------------------------------------------------
def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), plain ints."""
    c, k = [int(x) for x in ctr], [int(x) for x in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


# The same rounds on numpy uint64 arrays holding 32-bit words (broadcast), fast enough for whole batches: the package's
# function, which `test_philox_restatement_reproduces_the_published_vectors` holds to the plain-int statement above.
philox4x32_10_np = philox_ref.philox4x32_10


def uniform53(hi, lo):
    """numpy's `random_sample` construction from two 32-bit words, the first one the high part; exact in float64."""
    hi, lo = np.asarray(hi, dtype=np.uint64), np.asarray(lo, dtype=np.uint64)
    return ((hi >> np.uint64(5)).astype(np.float64) * 67108864.0 + (lo >> np.uint64(6)).astype(np.float64)) \
        / 9007199254740992.0


def _words(x):
    x = int(x) & 0xFFFFFFFFFFFFFFFF
    return x & 0xFFFFFFFF, x >> 32


def point_uniforms(seed, stream, n):
    """[n, 3] float64: the (u0, u1, u2) of points 0..n-1 of a slot with the 64-bit `stream` (include/mpa_hip.h)."""
    (k0, k1), (s0, s1) = _words(seed), _words(stream)
    i = np.arange(n, dtype=np.uint64)
    a = philox4x32_10_np(i, 0, s0, s1, k0, k1)
    b = philox4x32_10_np(i, 1, s0, s1, k0, k1)
    return np.stack([uniform53(a[0], a[1]), uniform53(a[2], a[3]), uniform53(b[0], b[1])], axis=1)


def rotation_uniforms(seed, streams):
    """[n, 3] float64: the (r0, r1, r2) of the slots with the 64-bit `streams` [n]."""
    k0, k1 = _words(seed)
    streams = np.asarray(streams, dtype=np.int64).astype(np.uint64).reshape(-1)
    s0, s1 = streams & np.uint64(0xFFFFFFFF), streams >> np.uint64(32)
    a = philox4x32_10_np(0, 2, s0, s1, k0, k1)
    b = philox4x32_10_np(0, 3, s0, s1, k0, k1)
    return np.stack([uniform53(a[0], a[1]), uniform53(a[2], a[3]), uniform53(b[0], b[1])], axis=1)


def slot_rotations(seed, streams, rot_range):
    """(rot float64 [n, 3, 3] applied to the points, quat float64 [n, 4] = its inverse, scalar first) of the slots
    `streams`, from the documented formulas in float64."""
    from scipy.spatial.transform import Rotation as R
    r = rotation_uniforms(seed, streams)
    if rot_range > 0:
        x, y, z, w = R.from_euler("xyz", (r - 0.5) * 2.0 * rot_range, degrees=True).as_quat().T
    else:
        a, b = np.sqrt(1.0 - r[:, 0]), np.sqrt(r[:, 0])
        x, y, z, w = a * np.sin(2 * np.pi * r[:, 1]), a * np.cos(2 * np.pi * r[:, 1]), \
            b * np.sin(2 * np.pi * r[:, 2]), b * np.cos(2 * np.pi * r[:, 2])
    mat = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                    [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                    [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]).transpose(2, 0, 1)
    return mat, np.stack([w, -x, -y, -z], axis=1)


def write_box_obj(path, lo, hi):
    """The box of tests/test_datasets.py: six quads (fan triangulation), `v/vt/vn` index syntax on one face."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    v = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    f = [(1, 2, 3, 4), (5, 8, 7, 6), (1, 5, 6, 2), (2, 6, 7, 3), (3, 7, 8, 4), (4, 8, 5, 1)]
    with open(path, "w") as fh:
        fh.write("# box\n")
        for p in v:
            fh.write("v %r %r %r\n" % p)
        for k, q in enumerate(f):
            fh.write("f " + " ".join((f"{i}/1/1" if k == 0 else str(i)) for i in q) + "\n")


def box_mesh(tmp_path, lo=(0, 0, 0), hi=(1, 2, 4)):
    write_box_obj(tmp_path / "box.obj", lo, hi)
    return load_obj(tmp_path / "box.obj")


def reference_tables(v, f):
    """origins / vectors / cumulative area with the very expressions of the sampler before this store existed."""
    tri = v[f]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    return tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], np.cumsum(area)


@pytest.fixture(scope="module")
def built():
    return _build.build()


# ---- 1. packing -------------------------------------------------------------------------------------------------------
def test_store_packs_every_part_bit_for_bit(tmp_path):
    shapes = synthetic.make_fracture_meshes(seed=5, shapes=3, parts_per_shape=[2, 4, 3], faces=200)
    shapes.append([box_mesh(tmp_path), box_mesh(tmp_path, (-1, -1, -1), (0, 0, 0))])
    store = MeshStore.from_arrays(shapes)
    assert store.num_shapes == 4 and store.num_parts == 11 and len(store) == 4
    np.testing.assert_array_equal(store.shape_part_off, [0, 2, 6, 9, 11])
    assert store.tri.dtype == np.float64 and store.cum_area.dtype == np.float64
    assert store.part_face_off.dtype == np.int64 and store.shape_part_off.dtype == np.int64
    k = 0
    for parts in shapes:
        for v, f in parts:
            a, b = store.part_face_off[k], store.part_face_off[k + 1]
            assert b - a == len(f)
            origin, e1, e2, cum = reference_tables(v, f)
            assert np.array_equal(store.cum_area[a:b], cum)
            assert np.array_equal(store.tri[a:b], np.concatenate([origin, e1, e2], axis=1))
            k += 1
    faces = store.part_face_off[-1]
    assert faces == sum(len(f) for parts in shapes for _, f in parts) and store.tri.shape == (faces, 9)
    assert store.nbytes == 80 * faces + 8 * 12 + 8 * 5
    assert MeshStore.from_arrays(shapes, max_bytes=store.nbytes).nbytes == store.nbytes
    with pytest.raises(ValueError, match="max_bytes"):
        MeshStore.from_arrays(shapes, max_bytes=store.nbytes - 1)
    # the box: 12 triangles, total area 2 * (1*2 + 1*4 + 2*4)
    assert store.part_face_off[10] - store.part_face_off[9] == 12
    assert store.cum_area[store.part_face_off[10] - 1] == 28.0


def test_make_fracture_meshes_is_seeded_and_closed():
    a = synthetic.make_fracture_meshes(3, 2, 3, 5000)
    b = synthetic.make_fracture_meshes(3, 2, 3, 5000)
    c = synthetic.make_fracture_meshes(4, 2, 3, 5000)
    assert [len(p) for p in a] == [3, 3]
    v, f = a[1][2]
    assert v.shape == (2502, 3) and f.shape == (5000, 3) and v.dtype == np.float64 and f.dtype == np.int64
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for p, q in zip(a, b) for x, y in zip(p, q))
    assert not np.array_equal(a[0][0][0], c[0][0][0])
    edges = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    directed = set(map(tuple, edges))
    assert len(directed) == len(edges) and all((q, p) in directed for p, q in directed)  # closed, consistently oriented
    state = np.random.get_state()[1].copy()
    synthetic.make_fracture_meshes(1, 1, 2, 20)
    assert np.array_equal(np.random.get_state()[1], state)  # numpy's global generator is not touched


# ---- 2. the sampler as a function of its uniforms ---------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 3, 11])
def test_sample_surface_from_uniforms_is_sample_surface(tmp_path, seed):
    meshes = [box_mesh(tmp_path), synthetic.make_fracture_meshes(seed, 1, 2, 300)[0][1]]
    for v, f in meshes:
        count = 4000
        np.random.seed(seed)
        want = sample_surface(v, f, count)
        np.random.seed(seed)
        pick = np.random.random(count)
        lengths = np.random.random((count, 2, 1))
        got = sample_surface_from_uniforms(v, f, np.concatenate([pick[:, None], lengths[:, :, 0]], axis=1))
        assert got.dtype == np.float64 and np.array_equal(got, want)
        # ... and it restates the sampler as it was before the two were one piece of code
        origin, e1, e2, cum = reference_tables(v, f)
        face = np.searchsorted(cum, pick * cum[-1])
        ln = lengths.copy()
        ln[ln.sum(axis=1).reshape(-1) > 1.0] -= 1.0
        old = (np.stack([e1[face], e2[face]], axis=1) * np.abs(ln)).sum(axis=1) + origin[face]
        assert np.array_equal(got, old)
    with pytest.raises(ValueError):
        sample_surface_from_uniforms(v, f, np.zeros((4, 2)))


def test_zero_area_faces_follow_searchsorted():
    """A degenerate face is never picked, except a degenerate FIRST face at a pick of exactly 0."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [0, 0, 1.0]])
    f = np.array([[0, 1, 3], [0, 1, 2], [1, 1, 2], [0, 2, 4]])  # faces 0 (collinear) and 2 (repeated vertex) have no area
    store = MeshStore.from_arrays([[(v, f), (v, f[1:])]])
    np.testing.assert_array_equal(store.cum_area[:4], [0.0, 0.5, 0.5, 1.0])
    u = np.random.RandomState(0).random_sample((5000, 3))
    u[0, 0], u[1, 0] = 0.0, np.nextafter(1.0, 0.0)
    pts = sample_surface_from_uniforms(v, f, u)
    on_face1 = np.abs(pts[:, 2]) < 1e-15
    on_face3 = np.abs(pts[:, 0]) < 1e-15
    assert (on_face1 | on_face3)[1:].all() and 0.45 < on_face1.mean() < 0.55
    assert pts[0, 1] == 0.0 and pts[0, 2] == 0.0  # pick == 0 -> face 0, the segment from (0,0,0) to (2,0,0)


# ---- 3. Philox known answers ------------------------------------------------------------------------------------------
KAT = [  # Random123's kat_vectors for philox4x32-10: counter, key, expected
    ([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
     [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
]


def test_philox_restatement_reproduces_the_published_vectors():
    for ctr, key, want in KAT:
        assert philox4x32_10(ctr, key) == want
        got = philox4x32_10_np(*[np.array([c, c]) for c in ctr], *key)
        assert [int(w[1]) for w in got] == want
    u = point_uniforms(seed=0x0123456789ABCDEF, stream=(7 << 32) + 5, n=6)
    assert u.shape == (6, 3) and (u >= 0).all() and (u < 1).all()
    w = philox4x32_10([4, 1, 5, 7], [0x89ABCDEF, 0x01234567])  # point 4, purpose 1 -> u2
    assert u[4, 2] == ((w[0] >> 5) * 2.0 ** 26 + (w[1] >> 6)) * 2.0 ** -53
    assert uniform53(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -53 and uniform53(0, 0) == 0.0
    from scipy.spatial.transform import Rotation as R
    r = rotation_uniforms(9, [2, (1 << 40) + 3])
    w = philox4x32_10([0, 2, 3, 1 << 8], [9, 0])
    assert r[1, 1] == ((w[2] >> 5) * 2.0 ** 26 + (w[3] >> 6)) * 2.0 ** -53
    for rot_range in (-1, 30.0):
        rot, quat = slot_rotations(9, [2, (1 << 40) + 3], rot_range)
        assert np.allclose(rot @ rot.transpose(0, 2, 1), np.eye(3), atol=1e-14)
        assert np.allclose(np.linalg.det(rot), 1.0, atol=1e-14)
        assert np.allclose(R.from_quat(quat[:, [1, 2, 3, 0]]).as_matrix(), rot.transpose(0, 2, 1), atol=1e-14)  # inverse
    euler = R.from_matrix(slot_rotations(9, np.arange(50), 30.0)[0]).as_euler("xyz", degrees=True)
    assert np.allclose(euler, (rotation_uniforms(9, np.arange(50)) - 0.5) * 60.0, atol=1e-10)


# ---- 4. save / load, errors, the .obj route ---------------------------------------------------------------------------
def test_save_load_round_trip_and_obj_route(tmp_path):
    shapes = synthetic.make_fracture_meshes(seed=2, shapes=2, parts_per_shape=[3, 2], faces=60)
    for s, parts in enumerate(shapes):
        folder = tmp_path / "data" / f"shape_{s}" / "fractured_0"
        folder.mkdir(parents=True)
        for k, (v, f) in enumerate(parts):
            with open(folder / f"piece_{k}.obj", "w") as fh:
                fh.writelines("v %r %r %r\n" % tuple(p) for p in v.tolist())
                fh.writelines("f %d %d %d\n" % tuple(t) for t in (f + 1).tolist())
    data_list = ["shape_0/fractured_0", "shape_1/fractured_0"]
    a = MeshStore.from_arrays(shapes)
    b = MeshStore.from_folders(str(tmp_path / "data"), data_list)
    a.save(tmp_path / "store.npz")
    c = MeshStore.load(tmp_path / "store.npz")
    for name in ("tri", "cum_area", "part_face_off", "shape_part_off"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
        assert np.array_equal(getattr(a, name), getattr(c, name)) and getattr(a, name).dtype == getattr(c, name).dtype
    assert c.nbytes == a.nbytes
    with pytest.raises(ValueError, match="max_bytes"):
        MeshStore.load(tmp_path / "store.npz", max_bytes=100)
    with pytest.raises(ValueError, match="parts outside"):
        MeshStore.from_folders(str(tmp_path / "data"), data_list, min_num_part=3)


def test_store_refuses_what_cannot_be_sampled():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.0]])
    good = (v, np.array([[0, 1, 2]]))
    with pytest.raises(ValueError, match="without faces"):
        MeshStore.from_arrays([[good, (v, np.zeros((0, 3), dtype=np.int64))]])
    with pytest.raises(ValueError, match="total area"):
        MeshStore.from_arrays([[good, (v, np.array([[0, 1, 1]]))]])
    with pytest.raises(ValueError, match="parts outside"):
        MeshStore.from_arrays([[good]])
    with pytest.raises(ValueError, match="parts outside"):
        MeshStore.from_arrays([[good] * 4], max_num_part=3)
    with pytest.raises(ValueError, match="face index"):
        MeshStore.from_arrays([[good, (v, np.array([[0, 1, 3]]))]])
    with pytest.raises(ValueError, match="offsets"):
        MeshStore(np.zeros((2, 9)), np.ones(2), [0, 1], [0, 1])
    assert MeshStore.from_arrays([[good]], min_num_part=1).num_parts == 1


# ---- 5. the C entry point and the producer without a GPU --------------------------------------------------------------
def test_mesh_sample_batch_validates_its_arguments(built):
    L = _lib.lib()
    one = ctypes.c_void_p(8)  # a non-null pointer that validation never dereferences

    def call(M, N, uniforms=None, rot=None, perm=None, stream_id=None, part_quat=None, tables=one, outs=one):
        return L.mpa_mesh_sample_batch(tables, tables, tables, 4, tables, M, N, uniforms, rot, perm, 1, stream_id,
                                       -1.0, outs, outs, part_quat, None, None)

    assert call(-1, 8) == -1 and b"negative" in L.mpa_last_error()
    assert call(4, -3) == -1 and b"N=-3" in L.mpa_last_error()
    assert call(4, 0) == -1
    assert call(4, 2049) == -1 and b"N=2049" in L.mpa_last_error() and b"LDS" in L.mpa_last_error()
    assert call(0, 2049) == -1  # sizes are checked before the empty batch returns
    assert call(0, 8) == 0 and call(0, 2048, tables=None, outs=None) == 0
    assert call(4, 8, tables=None) == -1 and b"null" in L.mpa_last_error()
    assert call(4, 8, outs=None) == -1 and b"null" in L.mpa_last_error()
    # replay mode needs uniforms, rot and perm together
    assert call(4, 8, uniforms=one) == -1 and b"replay" in L.mpa_last_error()
    assert call(4, 8, uniforms=one, rot=one) == -1
    assert call(4, 8, rot=one, stream_id=one, part_quat=one) == -1 and b"without uniforms" in L.mpa_last_error()
    # device-random mode needs the streams and somewhere to put the quaternions
    assert call(4, 8) == -1 and b"device-random" in L.mpa_last_error()
    assert call(4, 8, stream_id=one) == -1 and call(4, 8, part_quat=one) == -1
    assert L.mpa_abi_version() == 10  # a new symbol, no changed signature


def test_device_producer_has_no_cpu_fallback():
    store = MeshStore.from_arrays(synthetic.make_fracture_meshes(0, 2, 2, 20))
    prod = datasets.DeviceGeometryProducer(store, num_points=16, max_num_part=3, device="cpu")
    with pytest.raises(RuntimeError, match="HIP device only"):
        prod.batch([0, 1])
    with pytest.raises(RuntimeError, match="HIP device only"):
        prod.replay([0], np.zeros((1, 3, 16, 3)), np.zeros((1, 3, 9)), np.zeros((1, 3, 16), np.int32),
                    np.zeros((1, 3, 4), np.float32))
    with pytest.raises(RuntimeError, match="HIP device only"):
        store.device_arrays("cpu")
    with pytest.raises(ValueError, match="num_points"):
        datasets.DeviceGeometryProducer(store, num_points=2049)
    with pytest.raises(ValueError, match="unknown data"):
        datasets.DeviceGeometryProducer(store, data_keys=("match_ids",))
    # the host tables: store part ids per slot, -1 in padded slots; limits of the producer apply
    slot, valid = prod._slots([1, 0])
    np.testing.assert_array_equal(slot, [[2, 3, -1], [0, 1, -1]])
    np.testing.assert_array_equal(valid, [[1, 1, 0], [1, 1, 0]])
    with pytest.raises(IndexError):
        prod._slots([2])
    with pytest.raises(ValueError, match="part count"):
        datasets.DeviceGeometryProducer(store, min_num_part=3, device="cpu")._slots([0])
