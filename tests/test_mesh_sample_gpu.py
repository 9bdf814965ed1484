"""`mpa_mesh_sample_batch` / `DeviceGeometryProducer` on the MI355X.  Replay mode against numpy + the existing transform
kernel, bit for bit; device-random mode against the Philox restatement of tests/test_mesh_store.py (bits of the sampled
cloud, rotations to one float32 rounding) and against the distribution it must draw from."""
import random

import numpy as np
import pytest
import torch

from multi_part_assembly_amd import config, datasets, synthetic
from multi_part_assembly_amd.datasets import DeviceGeometryProducer, GeometryBatchProducer, MeshStore, \
    sample_surface_from_uniforms
from test_mesh_store import box_mesh, point_uniforms, slot_rotations

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB  # both key words are in use
ZERO_AREA = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [0, 0, 1.0]]),
             np.array([[0, 1, 3], [0, 1, 2], [1, 1, 2], [0, 2, 4]]))  # faces 0 and 2 have no area
ONE_FACE = (np.array([[0.1, 0.2, 0.3], [0.5, 0.1, 0.2], [0.2, 0.6, -0.1]]), np.array([[0, 1, 2]]))


def _mixed_shapes(tmp_path):
    """Three shapes of 4, 2 and 5 parts with 1, 4 (two of them degenerate), 12, 200 and 5000 faces."""
    small = synthetic.make_fracture_meshes(seed=1, shapes=2, parts_per_shape=[2, 4], faces=200)
    big = synthetic.make_fracture_meshes(seed=2, shapes=1, parts_per_shape=2, faces=5000)[0]
    return [[ONE_FACE, box_mesh(tmp_path), ZERO_AREA, big[0]], small[0], small[1] + [big[1]]]


def _numpy_clouds(shapes, indices, uniforms):
    return [np.stack([sample_surface_from_uniforms(v, f, uniforms[b, k]) for k, (v, f) in enumerate(shapes[i])])
            for b, i in enumerate(indices)]


# ---- 6. replay mode = numpy, exactly ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rot_range", [-1, 30.0])
def test_replay_is_numpy_and_the_transform_kernel_bit_for_bit(tmp_path, cuda_device, rot_range):
    shapes = _mixed_shapes(tmp_path)
    store = MeshStore.from_arrays(shapes)
    indices, P, N = [0, 1, 2, 0], 5, 517  # padded slots in shapes 0 and 1; N is no multiple of the block
    B = len(indices)
    uniforms = np.random.RandomState(1).random_sample((B, P, N, 3))
    uniforms[:, :, 0, 0] = 0.0                       # pick == 0: the first face, a degenerate one in ZERO_AREA
    uniforms[:, :, 1, 0] = np.nextafter(1.0, 0.0)    # the largest double below 1: the last face with area
    uniforms[:, :, 2, 1:] = 0.0
    uniforms[:, :, 3, 1:] = np.nextafter(1.0, 0.0)
    clouds = _numpy_clouds(shapes, indices, uniforms)

    host = GeometryBatchProducer(num_points=N, max_num_part=P, rot_range=rot_range,
                                 data_keys=("part_ids", "valid_matrix"), device=cuda_device)
    np.random.seed(77)
    random.seed(77)
    want = host.produce(clouds, data_ids=indices)
    np.random.seed(77)
    random.seed(77)
    rot, perm = np.zeros((B, P, 9)), np.zeros((B, P, N), dtype=np.int32)
    quat = np.zeros((B, P, 4), dtype=np.float32)
    for b, pcs in enumerate(clouds):
        for k in range(len(pcs)):  # the draws of produce(), in its order
            rot_mat, q = host._draw_rotation()
            rot[b, k], quat[b, k], perm[b, k] = rot_mat.reshape(9), q, host._draw_order(N)

    dev = DeviceGeometryProducer(store, num_points=N, max_num_part=P, rot_range=rot_range,
                                 data_keys=("part_ids", "valid_matrix"), device=cuda_device)
    got, raw = dev.replay(indices, uniforms, rot, perm, quat, return_raw=True)
    raw = raw.cpu().numpy()
    assert raw.dtype == np.float64
    for b, pcs in enumerate(clouds):
        assert np.array_equal(raw[b, :len(pcs)], pcs), f"sampled cloud of batch entry {b} differs from numpy"
        assert not raw[b, len(pcs):].any()
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].device == want[k].device, k
        assert torch.equal(got[k], want[k]), f"{k} differs from GeometryBatchProducer.produce"
    # the forced uniforms did what they are there for
    zero_area = raw[0, 2]
    assert zero_area[0, 1] == 0.0 and zero_area[0, 2] == 0.0       # pick 0 -> degenerate face 0 (on the x axis)
    assert abs(zero_area[1, 0]) < 1e-15                              # pick just below the total -> face 3 (x = 0)
    on_real_faces = (np.abs(zero_area[:, 2]) < 1e-15) | (np.abs(zero_area[:, 0]) < 1e-15)
    assert on_real_faces[1:].all()


def test_replay_validates_its_host_arrays(tmp_path, cuda_device):
    store = MeshStore.from_arrays(_mixed_shapes(tmp_path))
    dev = DeviceGeometryProducer(store, num_points=8, max_num_part=5, device=cuda_device)
    u, r, q = np.zeros((1, 5, 8, 3)), np.zeros((1, 5, 9)), np.zeros((1, 5, 4), np.float32)
    with pytest.raises(ValueError, match="perm entries"):
        dev.replay([1], u, r, np.full((1, 5, 8), 8, np.int32), q)
    with pytest.raises(ValueError, match="uniforms must be"):
        dev.replay([1], u[:, :, :4], r, np.zeros((1, 5, 8), np.int32), q)


# ---- 7. device-random mode: the bits of the sampled cloud ------------------------------------------------------------
def test_device_random_cloud_is_the_documented_philox_stream(tmp_path, cuda_device):
    shapes = _mixed_shapes(tmp_path)
    store = MeshStore.from_arrays(shapes)
    P, N = 5, 300
    dev = DeviceGeometryProducer(store, num_points=N, max_num_part=P, seed=SEED, device=cuda_device)
    indices, counter = [0, 1, 2], 3
    M = len(indices) * P
    got, raw = dev.batch(indices, batch_counter=counter, return_raw=True)
    raw_np = raw.cpu().numpy()
    for b, i in enumerate(indices):
        for k, (v, f) in enumerate(shapes[i]):
            u = point_uniforms(SEED, counter * M + b * P + k, N)
            assert np.array_equal(raw_np[b, k], sample_surface_from_uniforms(v, f, u)), (b, k)
        assert not raw_np[b, len(shapes[i]):].any()
    # a stream above 2^32 reaches the fourth counter word
    big_counter = (1 << 40) + 5
    _, raw_big = dev.batch([1], batch_counter=big_counter, return_raw=True)
    v, f = shapes[1][1]
    assert np.array_equal(raw_big[0, 1].cpu().numpy(),
                          sample_surface_from_uniforms(v, f, point_uniforms(SEED, big_counter * P + 1, N)))

    again, raw_again = dev.batch(indices, batch_counter=counter, return_raw=True)
    assert torch.equal(raw, raw_again) and set(again) == set(got)
    for k in got:
        assert torch.equal(got[k], again[k]), k
    other, _ = dev.batch(indices, batch_counter=counter + 1, return_raw=True)
    reseeded, _ = DeviceGeometryProducer(store, num_points=N, max_num_part=P, seed=SEED + 1,
                                         device=cuda_device).batch(indices, batch_counter=counter, return_raw=True)
    for changed in (other, reseeded):
        valid = got["part_valids"] > 0
        assert not torch.equal(changed["part_quat"], got["part_quat"])
        differs = (changed["part_pcs"] != got["part_pcs"]).flatten(2).any(-1)
        assert torch.equal(differs, valid)  # every valid part changed, every padded slot is still zero
    # the default counter counts batches
    a, b, c = dev.batch(indices), dev.batch(indices), dev.batch(indices, batch_counter=0)
    assert torch.equal(a["part_pcs"], c["part_pcs"]) and not torch.equal(a["part_pcs"], b["part_pcs"])

    # a slot does not depend on its batch mates: same position, other neighbours; and same stream in another batch size
    swapped = dev.batch([2, 1, 0], batch_counter=counter)
    for k in ("part_pcs", "part_trans", "part_quat"):
        assert torch.equal(swapped[k][1], got[k][1]), k
    first = dev.batch(indices, batch_counter=0)          # entry 1 uses the streams P .. 2 P - 1
    alone = dev.batch([1], batch_counter=1)              # ... and so does a batch of one with counter 1
    for k in ("part_pcs", "part_trans", "part_quat"):
        assert torch.equal(alone[k][0], first[k][1]), k


# ---- 8. device-random mode: rotations -------------------------------------------------------------------------------
def _qrot(q, p):
    """Rotate points p [..., n, 3] by the scalar-first quaternions q [..., 4] (taken as unit), float64."""
    w, v = q[..., None, :1], q[..., None, 1:]
    t = 2.0 * np.cross(v, p)
    return p + w * t + np.cross(v, t)


@pytest.mark.parametrize("rot_range,slots", [(-1, 20000), (30.0, 2000)])
def test_device_random_rotations(cuda_device, rot_range, slots):
    from scipy.spatial.transform import Rotation as R
    P, N = 20, 64
    store = MeshStore.from_arrays(synthetic.make_fracture_meshes(seed=4, shapes=1, parts_per_shape=P, faces=60))
    dev = DeviceGeometryProducer(store, num_points=N, max_num_part=P, rot_range=rot_range, seed=SEED,
                                 device=cuda_device)
    B = slots // P
    got, raw = dev.batch([0] * B, batch_counter=2, return_raw=True)
    raw = raw.cpu().numpy().reshape(slots, N, 3)
    pcs = got["part_pcs"].cpu().numpy().astype(np.float64).reshape(slots, N, 3)
    trans = got["part_trans"].cpu().numpy().astype(np.float64).reshape(slots, 3)
    quat32 = got["part_quat"].cpu().numpy().reshape(slots, 4)
    quat = quat32.astype(np.float64)
    want_rot, want_quat = slot_rotations(SEED, 2 * slots + np.arange(slots), rot_range)

    ulp = 2.0 ** -23  # one float32 ulp at 1.0 (1.2e-7)
    assert np.abs(quat - want_quat).max() <= ulp
    assert np.abs(np.linalg.norm(quat, axis=1) - 1.0).max() <= 1e-6
    assert np.abs(np.linalg.norm(quat32, axis=1) - 1.0).max() <= 1e-6
    # the rotation applied: every coordinate is below 1, so one float32 rounding of the float64 result is below `ulp`
    centroid = raw.mean(axis=1)
    want_pcs = np.einsum("sij,snj->sni", want_rot, raw - centroid[:, None])
    assert np.abs(want_pcs).max() < 1.0
    assert np.abs(pcs - want_pcs).max() <= ulp
    assert np.abs(trans - centroid).max() <= ulp and np.abs(centroid).max() < 1.0
    assert np.abs(pcs.mean(axis=1)).max() <= 1e-6  # zero-centred parts
    # the pose re-assembles the shape: qtransform(part_trans, part_quat, part_pcs) = the sampled cloud
    back = _qrot(quat, pcs) + trans[:, None]
    bound = 2.0 ** -20 * np.abs(raw).max(axis=(1, 2))
    assert (np.abs(back - raw).max(axis=(1, 2)) <= bound).all()

    applied = R.from_quat(quat[:, [1, 2, 3, 0]]).inv()
    if rot_range > 0:
        euler = applied.as_euler("xyz", degrees=True)
        assert np.abs(euler).max() <= rot_range
        assert np.abs(euler).max() > 0.9 * rot_range and np.abs(euler.mean(axis=0)).max() < 6 * rot_range / np.sqrt(3 * slots)
    else:  # Haar: every entry of the mean rotation matrix is near 0 (an entry has variance 1/3)
        mean = applied.as_matrix().mean(axis=0)
        assert np.abs(mean).max() <= 6.0 / np.sqrt(3.0 * slots)
        assert (np.abs(quat).mean(axis=0) > 0.3).all()  # no component is stuck (E|q_i| = 4 / (3 pi) = 0.42 on S^3)


# ---- 9. device-random mode: the distribution ------------------------------------------------------------------------
def _box_statistics(points, v, f):
    """Checks of issue item 9 on points sampled from the 1 x 2 x 4 box: on a face plane and inside the box, face counts
    against area shares (chi-square, 11 degrees of freedom), mean barycentric position per face against the centroid."""
    from scipy.stats import chi2
    lo, hi = np.array([0, 0, 0.0]), np.array([1, 2, 4.0])
    assert ((points >= lo - 1e-12) & (points <= hi + 1e-12)).all()
    assert ((np.abs(points - lo) < 1e-12) | (np.abs(points - hi) < 1e-12)).any(axis=1).all()
    origin, e1, e2, area = datasets.triangle_table(v, f)
    taken = np.zeros(len(points), dtype=bool)
    counts, means = [], []
    for k in range(len(f)):
        normal = np.cross(e1[k], e2[k])
        d = points - origin[k]
        # barycentric lengths along e1, e2 (the box's triangles are right-angled at the fan's first or a later corner:
        # solve the 2 x 2 normal equations)
        g = np.array([[e1[k] @ e1[k], e1[k] @ e2[k]], [e1[k] @ e2[k], e2[k] @ e2[k]]])
        ab = np.linalg.solve(g, np.stack([d @ e1[k], d @ e2[k]]))
        inside = (np.abs(d @ normal) < 1e-9) & (ab[0] >= -1e-12) & (ab[1] >= -1e-12) & (ab[0] + ab[1] <= 1 + 1e-12)
        mine = inside & ~taken   # a point on a shared edge (probability ~ 0) goes to the first face that has it
        taken |= mine
        counts.append(mine.sum())
        means.append(ab[:, mine].mean(axis=1))
    assert taken.all()
    counts = np.array(counts, dtype=np.float64)
    expected = len(points) * area / area.sum()
    stat = ((counts - expected) ** 2 / expected).sum()
    assert stat < chi2.ppf(1 - 1e-6, len(f) - 1), (stat, counts)
    # a barycentric length of a uniform point in a triangle has mean 1/3 and variance 1/18
    for k, m in enumerate(means):
        assert np.abs(m - 1.0 / 3.0).max() <= 6.0 * np.sqrt(1.0 / 18.0 / counts[k]), (k, m, counts[k])
    return stat


def test_device_random_points_follow_the_surface_distribution(tmp_path, cuda_device):
    v, f = box_mesh(tmp_path)
    assert len(f) == 12 and len(np.unique(np.round(datasets.triangle_table(v, f)[3], 9))) == 3  # 1, 2 and 4
    total = 400_000
    # the numpy sampler passes the same checks at the same size (a wrong threshold shows up here first)
    _box_statistics(sample_surface_from_uniforms(v, f, np.random.RandomState(9).random_sample((total, 3))), v, f)
    P, N = 2, 1000
    store = MeshStore.from_arrays([[(v, f), (v, f)]])
    dev = DeviceGeometryProducer(store, num_points=N, max_num_part=P, seed=SEED, device=cuda_device)
    _, raw = dev.batch([0] * (total // (P * N)), batch_counter=0, return_raw=True)
    points = raw.cpu().numpy().reshape(-1, 3)
    assert len(points) == total
    _box_statistics(points, v, f)


# ---- 10. the data_dict contract -------------------------------------------------------------------------------------
@pytest.mark.parametrize("data_keys", [("part_ids",), ("part_ids", "valid_matrix")])
def test_batch_has_the_data_dict_of_the_host_producer(cuda_device, data_keys):
    counts = [2, 5, 3, 4]
    shapes = synthetic.make_fracture_meshes(seed=6, shapes=4, parts_per_shape=counts, faces=120)
    store = MeshStore.from_arrays(shapes)
    P, N = 6, 128
    host = GeometryBatchProducer(num_points=N, max_num_part=P, data_keys=data_keys, device=cuda_device)
    u = np.random.RandomState(0).random_sample((4, P, N, 3))
    indices = [3, 1, 0, 2]
    want = host.produce(_numpy_clouds(shapes, indices, u), data_ids=indices)
    dev = DeviceGeometryProducer(store, num_points=N, max_num_part=P, data_keys=data_keys, seed=1, device=cuda_device)
    got = dev.batch(indices)
    assert list(got) == list(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and got[k].device == want[k].device, k
        assert got[k].is_contiguous(), k
    for k in set(want) - {"part_pcs", "part_trans", "part_quat"}:
        assert torch.equal(got[k], want[k]), k
    valid = got["part_valids"] > 0
    assert valid.sum(1).tolist() == [counts[i] for i in indices]
    assert got["part_pcs"][valid].mean(1).abs().max() <= 1e-6          # zero-centred parts
    assert not got["part_pcs"][~valid].any() and not got["part_trans"][~valid].any() and not got["part_quat"][~valid].any()
    norm = got["part_quat"][valid].norm(dim=-1)
    assert (norm - 1).abs().max() <= 1e-6
    # shuffle_parts permutes the parts of a shape and nothing else
    random.seed(5)
    shuffled = DeviceGeometryProducer(store, num_points=N, max_num_part=P, data_keys=data_keys, seed=1,
                                      device=cuda_device, shuffle_parts=True)
    slot, _ = shuffled._slots(indices)
    plain, _ = dev._slots(indices)
    assert np.array_equal(np.sort(slot, axis=1), np.sort(plain, axis=1)) and not np.array_equal(slot, plain)
    assert torch.equal(shuffled.batch(indices)["part_valids"], got["part_valids"])


@pytest.mark.parametrize("name", ["pn_transformer_everyday", "dgl_dgcnn_everyday"])
def test_train_step_takes_the_device_batch(cuda_device, name):
    from multi_part_assembly_amd.pn_transformer import build_model
    from multi_part_assembly_amd.trainer import Trainer
    cfg = getattr(config, name)()
    P, N = cfg.data.max_num_part, cfg.data.num_pc_points
    counts = [2, 7, 20, 4]
    store = MeshStore.from_arrays(synthetic.make_fracture_meshes(seed=8, shapes=4, parts_per_shape=counts, faces=200))
    dev = DeviceGeometryProducer(store, num_points=N, max_num_part=P, min_num_part=cfg.data.min_num_part,
                                 data_keys=tuple(cfg.data.data_keys), seed=3, device=cuda_device)
    batch = dev.batch([0, 1, 2, 3])
    clone = {k: v.clone() for k, v in batch.items()}

    def step(data):
        torch.manual_seed(0)
        trainer = Trainer(build_model(cfg).to(cuda_device), cfg)
        torch.manual_seed(1)
        return trainer.train_step(data)

    a, b = step(batch), step(clone)
    torch.cuda.synchronize()
    assert torch.isfinite(a).item() and torch.equal(a, b), (a, b)
