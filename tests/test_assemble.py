"""CPU-side checks of the assembly export (multi_part_assembly_amd/assemble.py, csrc/assemble.hip): the numpy
restatement against the reference's recorded `sample_assembly`, the C ABI's argument validation, and the host pieces —
writers, figure layout, ranking order, slot table, colour presets.  The kernels themselves: test_assemble_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import assembly_ref as R
from assembly_ref import read_ply
from multi_part_assembly_amd import _build, _lib, assemble, config, datasets, synthetic

NEW_SYMBOLS = ("mpa_assemble_clouds", "mpa_assemble_clouds_rmat", "mpa_mesh_pose_parts")


@pytest.fixture(scope="module")
def built():
    return _build.build()


# ---- the restatement against the reference's record ------------------------------------------------------------------------
@pytest.mark.parametrize("rot_type", ["quat", "rmat"])
def test_restatement_reproduces_the_reference_record(golden, rot_type):
    z = golden("sample_assembly")
    clouds, offsets = R.assemble_clouds(z["data.part_pcs"], z["data.part_valids"], z[f"{rot_type}.pred_rot"],
                                        z[f"{rot_type}.pred_trans"], z[f"{rot_type}.gt_rot"], z["data.part_trans"],
                                        z["colors"], rot_type)
    B, N = z["data.part_pcs"].shape[0], z["data.part_pcs"].shape[2]
    assert offsets.tolist() == [0, 2 * N, 7 * N, 10 * N] and clouds.shape == (4, 10 * N, 6)
    gt, pred = R.to_lists(clouds, offsets)
    assert len(gt) == B and len(pred) == B
    for b in range(B):
        want = z[f"{rot_type}.gt_pcs.{b}"]
        assert gt[b].dtype == want.dtype == np.float64 and gt[b].shape == want.shape
        assert np.array_equal(gt[b][:, :3].astype(np.float32).view(np.uint32),
                              want[:, :3].astype(np.float32).view(np.uint32))  # xyz bit for bit as float32
        assert np.array_equal(gt[b], want)                                   # (float64 of float32: the colours too)
        assert len(pred[b]) == 3
        for s in range(3):
            want = z[f"{rot_type}.pred_pcs.{b}.{s}"]
            assert pred[b][s].dtype == want.dtype and pred[b][s].shape == want.shape
            assert np.array_equal(pred[b][s][:, :3].astype(np.float32).view(np.uint32),
                                  want[:, :3].astype(np.float32).view(np.uint32))
            assert np.array_equal(pred[b][s][:, 3:], want[:, 3:])
    # the three recorded forwards differ (the record is of a stochastic regressor), so the slabs are told apart
    assert not np.array_equal(clouds[0], clouds[1]) and not np.array_equal(clouds[1], clouds[2])


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_the_abi_version_stays(built):
    assert _lib.ABI_VERSION == 10
    declared = _lib.declared_functions()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and name in declared
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().mpa_abi_version() == 10


def test_argument_validation_needs_no_gpu(built):
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for fn in (L.mpa_assemble_clouds, L.mpa_assemble_clouds_rmat):
        # (pcs, valids, rot, trans, gt_rot, gt_trans, colors, S, B, P, N, C, offsets, clouds, stream)
        for sizes in ((-1, 1, 1, 1, 1), (1, -1, 1, 1, 1), (1, 1, -1, 1, 1), (1, 1, 1, -1, 1), (1, 1, 1, 1, -1)):
            assert fn(p, p, p, p, p, p, p, *sizes, p, p, None) == -1 and b"negative" in L.mpa_last_error()
        assert fn(p, p, p, p, p, p, p, 1, 2, 5, 8, 4, p, p, None) == -1 and b"colours" in L.mpa_last_error()  # C < P
        assert fn(None, None, None, None, None, None, None, 1, 0, 5, 8, 5, None, None, None) == 0              # B = 0
        for hole in range(7):
            args = [p] * 7
            args[hole] = None
            assert fn(*args, 1, 2, 5, 8, 5, p, p, None) == -1 and b"null" in L.mpa_last_error()
        assert fn(p, p, p, p, p, p, p, 1, 2, 5, 8, 5, None, p, None) == -1 and b"null" in L.mpa_last_error()
        assert fn(p, p, p, p, p, p, p, 1, 2, 5, 8, 5, p, None, None) == -1 and b"null" in L.mpa_last_error()
    fn = L.mpa_mesh_pose_parts
    # (tri, part_face_off, parts_total, slot_part, out_face_off, M, faces_out, max_faces, 4 poses, 3 outputs, stream)
    assert fn(p, p, 1, p, p, -1, 4, 4, p, p, p, p, p, p, p, None) == -1 and b"negative" in L.mpa_last_error()
    assert fn(p, p, 1, p, p, 1, -4, 4, p, p, p, p, p, p, p, None) == -1 and b"negative" in L.mpa_last_error()
    assert fn(None, None, 1, None, None, 0, 4, 4, None, None, None, None, None, None, None, None) == 0  # M = 0
    assert fn(None, None, 1, None, None, 3, 0, 0, None, None, None, None, None, None, None, None) == 0  # no faces
    assert fn(None, p, 1, p, p, 1, 4, 4, p, p, p, p, p, p, p, None) == -1 and b"null" in L.mpa_last_error()
    assert fn(p, p, 1, p, p, 1, 4, 4, p, p, p, p, p, p, None, None) == -1 and b"null" in L.mpa_last_error()


def test_wrappers_reject_cpu_tensors(monkeypatch):
    B, P, N = 2, 3, 4
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        assemble.assemble_clouds(z(B, P, N, 3), z(B, P), z(1, B, P, 4), z(1, B, P, 3), z(B, P, 4), z(B, P, 3), z(P, 3),
                                 rot_type="quat")
    # pose_meshes takes poses from anywhere (the ranking's records are host arrays) and moves them to the device; what
    # it refuses is to run without one
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    store = datasets.MeshStore.from_arrays(synthetic.make_fracture_meshes(1, 1, 2, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        assemble.pose_meshes(store, [0, 1], z(2, 4), z(2, 3), z(2, 4), z(2, 3))


# ---- writers -------------------------------------------------------------------------------------------------------------------
def test_write_obj_reads_back_through_load_obj(tmp_path):
    rng = np.random.RandomState(5)
    tri = rng.standard_normal((7, 3, 3)).astype(np.float32)
    assemble.write_obj(tmp_path / "a.obj", tri)
    v, f = datasets.load_obj(tmp_path / "a.obj")
    assert v.dtype == np.float64 and np.array_equal(v, tri.reshape(-1, 3).astype(np.float64))
    assert np.array_equal(f, np.arange(21).reshape(7, 3))
    text = (tmp_path / "a.obj").read_text().splitlines()
    assert sum(l.startswith("v ") for l in text) == 21 and sum(l.startswith("f ") for l in text) == 7
    tri64 = rng.standard_normal((2, 3, 3))
    assemble.write_obj(tmp_path / "b.obj", tri64)
    assert np.array_equal(datasets.load_obj(tmp_path / "b.obj")[0], tri64.reshape(-1, 3))
    assemble.write_obj(tmp_path / "c.obj", np.zeros((0, 3, 3)))
    assert datasets.load_obj(tmp_path / "c.obj")[0].shape == (0, 3)


def test_write_ply_reads_back(tmp_path):
    rng = np.random.RandomState(6)
    xyz = rng.standard_normal((37, 3)).astype(np.float32)
    rgb = rng.randint(0, 256, size=(37, 3))
    assemble.write_ply(tmp_path / "a.ply", xyz, rgb)
    got_xyz, got_rgb = read_ply(tmp_path / "a.ply")
    assert np.array_equal(got_xyz.view(np.uint32), xyz.view(np.uint32)) and np.array_equal(got_rgb, rgb)
    assemble.write_ply(tmp_path / "b.ply", xyz.astype(np.float64))
    got_xyz, got_rgb = read_ply(tmp_path / "b.ply")
    assert np.array_equal(got_xyz, xyz) and got_rgb is None
    assemble.write_ply(tmp_path / "c.ply", np.zeros((0, 3)))
    assert read_ply(tmp_path / "c.ply")[0].shape == (0, 3)
    with pytest.raises(ValueError):
        assemble.write_ply(tmp_path / "d.ply", xyz, rgb[:5])


# ---- figure, ranking, slots, presets -------------------------------------------------------------------------------------------
def test_assembly_figure_shifts_as_the_callback(golden):
    z = golden("sample_assembly")
    gt = [z[f"quat.gt_pcs.{b}"] for b in range(3)]
    pred = [[z[f"quat.pred_pcs.{b}.{s}"] for s in range(3)] for b in range(3)]
    keep = [g.copy() for g in gt]
    figs = assemble.assembly_figure(gt, pred)
    assert len(figs) == 3
    for b in range(3):
        # utils/callback.py:26-33, on copies
        g = gt[b].copy()
        g[:, 0] = g[:, 0] + 1.5
        ps = [p.copy() for p in pred[b]]
        for j in range(3):
            ps[j][:, 0] = ps[j][:, 0] - 1.5 * j
        assert np.array_equal(figs[b], np.concatenate([g, *ps], axis=0))
        assert figs[b].shape == (4 * len(gt[b]), 6) and np.array_equal(gt[b], keep[b])  # inputs untouched


def test_rank_order_is_ascending_and_stable():
    crit = torch.tensor([0.5, 0.25, 0.5, 0.125, 0.25, 0.5])
    assert assemble.rank_order(crit).tolist() == [3, 1, 4, 0, 2, 5]
    assert assemble.rank_order(crit, top=3).tolist() == [3, 1, 4]
    assert assemble.rank_order(crit, top=-1).tolist() == [3, 1, 4, 0, 2, 5]   # (scripts/vis.py's default: everything)
    assert assemble.rank_order(crit, top=99).tolist() == [3, 1, 4, 0, 2, 5]
    assert np.array_equal(assemble.rank_order(crit).numpy(), np.argsort(crit.numpy(), kind="stable"))


def test_slot_parts_follows_the_store_offsets():
    shapes = synthetic.make_fracture_meshes(3, 4, [2, 5, 3, 4], 8)
    store = datasets.MeshStore.from_arrays(shapes, max_num_part=5)
    prod = datasets.DeviceGeometryProducer(store, num_points=16, max_num_part=5, device="cpu")
    table = prod.slot_parts([2, 0, 1])
    assert table.dtype == np.int64 and table.shape == (3, 5)
    off = store.shape_part_off
    for row, s in zip(table, (2, 0, 1)):
        p = off[s + 1] - off[s]
        assert row[:p].tolist() == list(range(off[s], off[s + 1])) and (row[p:] == -1).all()
    shuffled = datasets.DeviceGeometryProducer(store, num_points=16, max_num_part=5, device="cpu", shuffle_parts=True)
    with pytest.raises(RuntimeError, match="shuffle_parts"):
        shuffled.slot_parts([0])


def test_presets_carry_a_colour_per_part_slot():
    presets = [getattr(config, n) for n in dir(config) if n.endswith(("_everyday", "_artifact", "_partnet_chair"))
               and callable(getattr(config, n)) and not n.startswith(("_", "breaking_bad"))]
    assert len(presets) >= 15
    for make in presets:
        cfg = make()
        colors = np.array(cfg.data.colors)
        assert colors.ndim == 2 and colors.shape[1] == 3 and len(colors) >= max(20, cfg.data.max_num_part)
        assert colors.dtype.kind == "i" and colors.min() >= 0 and colors.max() <= 255
        assert len({tuple(c) for c in colors.tolist()}) == len(colors)  # parts are told apart
