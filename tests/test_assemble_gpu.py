"""csrc/assemble.hip on the device: `assemble_clouds` against the reference's recorded `sample_assembly` and the numpy
restatement (tests/assembly_ref.py), `pose_meshes` against the float64 restatement, `BaseModel.sample_assembly` against
its composition from `forward` + `transform_pc` + masking, a captured call, and tools/visualize.py end to end."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import param_fill  # noqa: E402

import assembly_ref as R  # noqa: E402
from assembly_ref import read_ply  # noqa: E402
from multi_part_assembly_amd import assemble, config, datasets, synthetic  # noqa: E402
from multi_part_assembly_amd.pn_transformer import build_model  # noqa: E402
from multi_part_assembly_amd.rotation import Rotation3D  # noqa: E402
from multi_part_assembly_amd.transforms import transform_pc  # noqa: E402
from tool_loader import load_tool  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5  # byte the output buffers are filled with: a float32 of these bytes is -2.87e-16, no value a test produces


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run_clouds(dev, pcs, valids, rot, trans, gt_rot, gt_trans, colors, rot_type):
    """-> (clouds [S + 1, cap, 6], offsets [B + 1]) on the host, of a call into sentinel-filled buffers."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    B, P, N, _ = pcs.shape
    out = assemble.AssembledClouds.empty(B, P, N, len(rot), dev)
    out.packed.fill_(SENTINEL)
    res = assemble.assemble_clouds(t(pcs), t(valids), t(rot), t(trans), t(gt_rot), t(gt_trans), t(colors),
                                   rot_type=rot_type, out=out)
    assert res is out
    clouds, offsets = out.to_host()
    return clouds.copy(), offsets.copy()


def check_against(clouds, offsets, want, want_off):
    """Used rows equal `want` bit for bit, every row behind them still holds the sentinel."""
    assert offsets.tolist() == want_off.tolist()
    used = int(want_off[-1])
    assert want.shape[1] == used
    assert np.array_equal(bits(clouds[:, :used]), bits(want))
    assert (clouds[:, used:].view(np.uint8) == SENTINEL).all()


def random_case(seed, B, P, N, S, rot_type, valid):
    rng = np.random.RandomState(seed)
    pcs = (rng.standard_normal((B, P, N, 3)) * 0.2).astype(np.float32)
    trans, gt_trans = (rng.standard_normal(s + (3,)).astype(np.float32) for s in ((S, B, P), (B, P)))
    if rot_type == "quat":  # not normalised: the kernel must not normalise either
        rot, gt_rot = (rng.standard_normal(s + (4,)).astype(np.float32) for s in ((S, B, P), (B, P)))
    else:
        rot, gt_rot = (rng.standard_normal(s + (3, 3)).astype(np.float32) for s in ((S, B, P), (B, P)))
    colors = rng.randint(0, 256, size=(P + 2, 3)).astype(np.float32)
    return pcs, np.asarray(valid, dtype=np.float32).reshape(B, P), rot, trans, gt_rot, gt_trans, colors


# ---- clouds against the reference's record --------------------------------------------------------------------------------
@pytest.mark.parametrize("rot_type", ["quat", "rmat"])
def test_clouds_equal_the_reference_record(golden, cuda_device, rot_type):
    z = golden("sample_assembly")
    clouds, offsets = run_clouds(cuda_device, z["data.part_pcs"], z["data.part_valids"], z[f"{rot_type}.pred_rot"],
                                 z[f"{rot_type}.pred_trans"], z[f"{rot_type}.gt_rot"], z["data.part_trans"], z["colors"],
                                 rot_type)
    N = z["data.part_pcs"].shape[2]
    assert offsets.tolist() == [0, 2 * N, 7 * N, 10 * N]
    for b in range(3):
        a, e = offsets[b], offsets[b + 1]
        want = z[f"{rot_type}.gt_pcs.{b}"]
        assert np.array_equal(bits(clouds[3, a:e, :3]), bits(want[:, :3])) and np.array_equal(clouds[3, a:e, 3:], want[:, 3:])
        for s in range(3):
            want = z[f"{rot_type}.pred_pcs.{b}.{s}"]
            assert np.array_equal(bits(clouds[s, a:e, :3]), bits(want[:, :3]))
            assert np.array_equal(clouds[s, a:e, 3:], want[:, 3:])
    assert (clouds[:, offsets[-1]:].view(np.uint8) == SENTINEL).all()  # no row >= offsets[B] of any slab changed


@pytest.mark.parametrize("rot_type", ["quat", "rmat"])
def test_padded_slots_are_never_read(golden, cuda_device, rot_type):
    z = golden("sample_assembly")
    pad = z["data.part_valids"] != 1
    args = [z["data.part_pcs"].copy(), z["data.part_valids"], z[f"{rot_type}.pred_rot"].copy(),
            z[f"{rot_type}.pred_trans"].copy(), z[f"{rot_type}.gt_rot"].copy(), z["data.part_trans"].copy()]
    clean = run_clouds(cuda_device, *args, z["colors"], rot_type)
    args[0][pad] = np.nan
    args[2][:, pad] = np.nan
    args[3][:, pad] = np.nan
    args[4][pad] = np.nan
    args[5][pad] = np.nan
    dirty = run_clouds(cuda_device, *args, z["colors"], rot_type)
    used = int(dirty[1][-1])
    assert np.isfinite(dirty[0][:, :used]).all()
    assert np.array_equal(bits(dirty[0]), bits(clean[0])) and np.array_equal(dirty[1], clean[1])


# ---- masks and sizes ----------------------------------------------------------------------------------------------------------
CASES = {
    "rank_colours": (2, 5, 7, 2, [[1, 0, 1, 0, 1], [0, 0, 1, 1, 0]]),   # masks that are no prefix
    "empty_shape": (3, 4, 5, 1, [[1, 1, 0, 0], [0, 0, 0, 0], [0, 1, 0, 1]]),
    "all_empty": (2, 3, 4, 1, [[0, 0, 0], [0, 0, 0]]),
    "one": (1, 1, 1, 1, [[1]]),
    "one_S3": (1, 1, 1, 3, [[1]]),
    "no_prediction": (2, 3, 5, 0, [[1, 1, 0], [1, 1, 1]]),            # S = 0: the ground-truth slab alone
    "N63": (2, 3, 63, 1, [[1, 1, 0], [0, 1, 1]]),
    "N64": (2, 3, 64, 3, [[1, 1, 0], [0, 1, 1]]),
    "N65": (2, 3, 65, 1, [[1, 1, 0], [0, 1, 1]]),
    "N255": (1, 2, 255, 1, [[1, 1]]),                                 # one row short of a block,
    "N257": (1, 2, 257, 3, [[1, 1]]),                                 # one row into the second block of a part
    "not_one": (1, 3, 6, 1, [[1, 0.5, 2]]),                           # real iff == 1
    "B300": (300, 2, 3, 1, None),                                     # more shapes than the prefix kernel's block
}


@pytest.mark.parametrize("rot_type", ["quat", "rmat"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_masks_and_sizes(cuda_device, case, rot_type):
    B, P, N, S, valid = CASES[case]
    if valid is None:
        valid = np.random.RandomState(B).randint(0, 2, size=(B, P))
    args = random_case(11, B, P, N, S, rot_type, valid)
    want, want_off = R.assemble_clouds(*args, rot_type)
    clouds, offsets = run_clouds(cuda_device, *args, rot_type)
    check_against(clouds, offsets, want, want_off)
    if case == "rank_colours":  # slots {0, 2, 4} carry colours 0, 1, 2
        assert np.array_equal(clouds[0, :3 * N, 3:], np.repeat(args[6][:3], N, axis=0))
        assert np.array_equal(clouds[0, 3 * N:5 * N, 3:], np.repeat(args[6][:2], N, axis=0))
    if case == "empty_shape":
        assert offsets[1] == offsets[2]


def test_full_size_and_determinism(cuda_device):
    """B = 32, P = 20, N = 1000, S = 2 (the grid limits: 640 x 4 blocks, a last block of 232 rows), twice."""
    rng = np.random.RandomState(3)
    valid = np.arange(20)[None] < rng.randint(2, 21, size=(32, 1))
    args = random_case(12, 32, 20, 1000, 2, "quat", valid)
    want, want_off = R.assemble_clouds(*args, "quat")
    first = run_clouds(cuda_device, *args, "quat")
    check_against(*first, want, want_off)
    second = run_clouds(cuda_device, *args, "quat")
    assert np.array_equal(bits(first[0]), bits(second[0])) and np.array_equal(first[1], second[1])


def test_single_prediction_and_rotation3d_arguments(golden, cuda_device):
    z = golden("sample_assembly")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(cuda_device)
    pcs, valids, colors = t(z["data.part_pcs"]), t(z["data.part_valids"]), t(z["colors"])
    rot, gt = Rotation3D(t(z["quat.pred_rot"][1]), "quat"), Rotation3D(t(z["quat.gt_rot"]), "quat")
    res = assemble.assemble_clouds(pcs, valids, rot, t(z["quat.pred_trans"][1]), gt, t(z["data.part_trans"]), colors)
    assert res.num_samples == 1 and res.clouds.shape == (2, 3 * 5 * 37, 6) and res.offsets.dtype == torch.int64
    gt_lst, pred_lst = res.to_lists()
    for b in range(3):
        assert gt_lst[b].dtype == np.float64 and np.array_equal(gt_lst[b], z[f"quat.gt_pcs.{b}"])
        assert len(pred_lst[b]) == 1 and np.array_equal(pred_lst[b][0], z[f"quat.pred_pcs.{b}.1"])
    cut_gt, cut_pred = res.to_lists(rows=10 * 37)  # a host-side bound: the slabs are cut before the copy
    assert all(np.array_equal(a, b) for a, b in zip(cut_gt, gt_lst)) and np.array_equal(cut_pred[1][0], pred_lst[1][0])
    assert res.to_host(rows=10 * 37)[0].shape == (2, 370, 6) and res.to_host(rows=10 ** 9)[0].shape == (2, 555, 6)
    with pytest.raises(ValueError, match="no bound"):
        res.to_host(rows=10 * 37 - 1)
    with pytest.raises(RuntimeError, match="colours"):
        assemble.assemble_clouds(pcs, valids, rot, t(z["quat.pred_trans"][1]), gt, t(z["data.part_trans"]), colors[:4])
    with pytest.raises(RuntimeError, match="`out`"):
        assemble.assemble_clouds(pcs, valids, rot, t(z["quat.pred_trans"][1]), gt, t(z["data.part_trans"]), colors,
                                 out=assemble.AssembledClouds.empty(3, 5, 37, 2, cuda_device))


# ---- one device-to-host copy, no synchronisation in the call ---------------------------------------------------------------
class CopyCounter:
    """Counts the device-to-host transfers torch performs while it is installed: every `Tensor` method that can move
    data to the host is wrapped, and a call counts when it reads a CUDA tensor into host memory."""

    def __init__(self, monkeypatch):
        self.count = 0
        for name in ("cpu", "item", "tolist", "numpy", "__array__"):
            self._wrap(monkeypatch, name, lambda self_t, *a, **k: self_t.is_cuda)
        self._wrap(monkeypatch, "to", lambda self_t, *a, **k: self_t.is_cuda and (
            any(str(x) == "cpu" or (isinstance(x, torch.device) and x.type == "cpu") for x in a)
            or str(k.get("device", "")) == "cpu"))
        self._wrap(monkeypatch, "copy_", lambda self_t, src, *a, **k: (not self_t.is_cuda) and torch.is_tensor(src)
                   and src.is_cuda)

    def _wrap(self, monkeypatch, name, moves):
        orig = getattr(torch.Tensor, name)
        counter = self

        def wrapped(self_t, *a, **k):
            if moves(self_t, *a, **k):
                counter.count += 1
            return orig(self_t, *a, **k)

        monkeypatch.setattr(torch.Tensor, name, wrapped)


@pytest.fixture(scope="module")
def models(cuda_device):
    """pn_transformer (quat, rmat) and dgl at the fixture's sizes, stochastic (three samples, 32 noise channels), with
    `param_fill` parameters; built once for the module."""
    built = {}
    for name, make, rot_type in (("pn_quat", config.pn_transformer_everyday, "quat"),
                                 ("pn_rmat", config.pn_transformer_everyday, "rmat"), ("dgl", config.dgl_everyday, "quat")):
        cfg = make()
        cfg.model.rot_type = rot_type
        cfg.model.pc_feat_dim = 64
        if name != "dgl":
            cfg.model.transformer_feat_dim, cfg.model.transformer_heads, cfg.model.transformer_layers = 128, 4, 2
        cfg.data.max_num_part = 5
        cfg.loss.sample_iter, cfg.loss.noise_dim = 3, 32
        torch.manual_seed(41)
        model = build_model(cfg)
        param_fill.fill_parameters(model, 41)
        built[name] = model.to(cuda_device).eval()
    return built


def fixture_batch(golden, dev):
    z = golden("sample_assembly")
    return {k[5:]: torch.from_numpy(z[k].copy()).to(dev) for k in z if k.startswith("data.")}


@pytest.mark.parametrize("name", ["pn_quat", "pn_rmat", "dgl"])
def test_sample_assembly_equals_its_composition(golden, cuda_device, models, monkeypatch, name):
    model = models[name]
    batch = fixture_batch(golden, cuda_device)
    keys = set(batch)
    # the composition: sample_iter forwards, transform_pc, torch masking, the reference's colour loop
    torch.manual_seed(97)
    data = dict(batch)
    gt_rot = Rotation3D(data.pop("part_quat"), "quat").convert(model.rot_type)
    data["part_rot"] = gt_rot
    counter = CopyCounter(monkeypatch)
    with torch.no_grad():
        outs = [model.forward(data) for _ in range(3)]
        forward_copies = counter.count  # what the model's own forwards move to the host (not part of the fused tail)
        posed = [transform_pc(o["trans"], o["rot"], batch["part_pcs"]) for o in outs]
        posed.append(transform_pc(batch["part_trans"], gt_rot, batch["part_pcs"]))
    colors = np.array(model.cfg.data.colors)
    want = []
    for pts in posed:
        per_shape = []
        for b in range(3):
            part = pts[b][batch["part_valids"][b].bool()].cpu().numpy()
            col = np.zeros(part.shape[:2] + (6,))
            col[:, :, :3] = part
            for k in range(len(part)):
                col[k, :, 3:] = colors[k]
            per_shape.append(col.reshape(-1, 6))
        want.append(per_shape)
    assert not np.array_equal(want[0][1], want[1][1])  # the forwards are stochastic
    torch.manual_seed(97)
    counter.count = 0
    gt_lst, pred_lst = model.sample_assembly(batch)
    assert counter.count - forward_copies == 1  # the fused path's one device-to-host copy
    monkeypatch.undo()
    assert set(batch) == keys and "part_quat" in batch and "part_rot" not in batch  # the caller's dict is as it was
    assert len(gt_lst) == 3 and len(pred_lst) == 3
    for b in range(3):
        assert gt_lst[b].dtype == np.float64 and np.array_equal(gt_lst[b], want[3][b])
        assert len(pred_lst[b]) == 3
        for s in range(3):
            assert np.array_equal(bits(pred_lst[b][s][:, :3]), bits(want[s][b][:, :3]))
            assert np.array_equal(pred_lst[b][s][:, 3:], want[s][b][:, 3:])


def test_assemble_clouds_issues_no_synchronisation(golden, cuda_device):
    z = golden("sample_assembly")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(cuda_device)
    args = [t(z[k]) for k in ("data.part_pcs", "data.part_valids", "quat.pred_rot", "quat.pred_trans", "quat.gt_rot",
                              "data.part_trans", "colors")]
    out = assemble.AssembledClouds.empty(3, 5, 37, 3, cuda_device)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        assemble.assemble_clouds(*args, rot_type="quat", out=out)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(out.to_lists()[0][2], z["quat.gt_pcs.2"])


def test_captured_call_replays_on_rewritten_poses(golden, cuda_device):
    z = golden("sample_assembly")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(cuda_device)
    pcs, valids, gt_rot, gt_trans, colors = (t(z[k]) for k in ("data.part_pcs", "data.part_valids", "quat.gt_rot",
                                                                 "data.part_trans", "colors"))
    rot, trans = t(z["quat.pred_rot"]), t(z["quat.pred_trans"])
    static_rot, static_trans = torch.zeros_like(rot), torch.zeros_like(trans)
    static_rot[..., 0] = 1.0
    out = assemble.AssembledClouds.empty(3, 5, 37, 3, cuda_device)
    side = torch.cuda.Stream(device=cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(side):
        assemble.assemble_clouds(pcs, valids, static_rot, static_trans, gt_rot, gt_trans, colors, rot_type="quat", out=out)
    torch.cuda.current_stream(cuda_device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assemble.assemble_clouds(pcs, valids, static_rot, static_trans, gt_rot, gt_trans, colors, rot_type="quat", out=out)
    static_rot.copy_(rot)
    static_trans.copy_(trans)
    out.packed.fill_(SENTINEL)
    graph.replay()
    replayed, off = out.to_host()
    eager = assemble.assemble_clouds(pcs, valids, rot, trans, gt_rot, gt_trans, colors, rot_type="quat")
    want, want_off = eager.to_host()
    used = int(want_off[-1])
    assert np.array_equal(off, want_off) and np.array_equal(bits(replayed[:, :used]), bits(want[:, :used]))
    assert (replayed[:, used:].view(np.uint8) == SENTINEL).all()
    assert np.array_equal(eager.to_lists()[1][1][2], z["quat.pred_pcs.1.2"])


# ---- meshes ---------------------------------------------------------------------------------------------------------------------
FACES = (1, 63, 64, 65, 5000)


@pytest.fixture(scope="module")
def mesh_case(cuda_device):
    """One store whose parts have 1, 63, 64, 65 and 5000 faces (the first faces of `make_fracture_meshes` parts, the
    vertices rounded to float32 so that the kernel's `orig` can hold them exactly), posed as 6 slots, one of them empty."""
    rng = np.random.RandomState(21)
    parts = []
    for k, faces in enumerate(FACES):
        v, f = synthetic.make_fracture_meshes(100 + k, 1, 1, 2 * faces + 16)[0][0]
        assert len(f) >= faces
        parts.append((v.astype(np.float32).astype(np.float64), f[:faces]))
    store = datasets.MeshStore.from_arrays([parts[:2], parts[2:]], max_num_part=5)
    slot_part = np.array([4, 0, -1, 3, 1, 2], dtype=np.int64)
    quat = rng.standard_normal((2, 6, 4)).astype(np.float32)
    quat /= np.linalg.norm(quat, axis=-1, keepdims=True)
    gt_trans, pred_trans = (rng.standard_normal((6, 3)) * 0.3).astype(np.float32), (rng.standard_normal((6, 3)) * 0.3).astype(np.float32)
    return store, parts, slot_part, quat[0], gt_trans, quat[1], pred_trans


def test_mesh_pose_parts_matches_float64(cuda_device, mesh_case):
    store, parts, slot_part, gt_quat, gt_trans, pred_quat, pred_trans = mesh_case
    F_sel = sum(FACES)
    out = assemble.PosedMeshes(*(torch.full((F_sel + 3, 3, 3), -7.0, device=cuda_device) for _ in range(3)), None)
    view = assemble.PosedMeshes(out.orig[:F_sel], out.input[:F_sel], out.pred[:F_sel], None)
    res = assemble.pose_meshes(store, slot_part, torch.from_numpy(gt_quat).to(cuda_device), gt_trans, pred_quat, pred_trans,
                               rot_type="quat", out=view)
    assert res.face_off.tolist() == np.concatenate([[0], np.cumsum([5000, 1, 0, 65, 63, 64])]).tolist()
    got = res.to_host()
    g_rmat, p_rmat = R.quat_to_rmat(gt_quat), R.quat_to_rmat(pred_quat)
    w_orig, w_in, w_pred, w_off = R.mesh_pose_parts(store.tri, store.part_face_off, slot_part, g_rmat, gt_trans, p_rmat,
                                                    pred_trans)
    assert np.array_equal(w_off, res.face_off)
    for name, g, w in zip(("orig", "input", "pred"), got, (w_orig, w_in, w_pred)):
        assert g.dtype == np.float32 and g.shape == (F_sel, 3, 3)
        ok = R.float32_or_adjacent(g, w)
        assert ok.all(), (name, int((~ok).sum()))
    # the rows behind the selection were not touched
    for x in (out.orig, out.input, out.pred):
        assert (x[F_sel:] == -7.0).all()
    # `orig` is the mesh: re-sampled by the sampler's restatement it gives the points of the stored mesh
    u = np.random.RandomState(4).random_sample((50, 3))
    for m, part in enumerate(slot_part):
        if part < 0:
            continue
        tri = res.slot(got, m)[0].astype(np.float64)
        v, f = parts[part]
        assert np.array_equal(datasets.sample_surface_from_uniforms(tri.reshape(-1, 3), np.arange(3 * len(tri)).reshape(-1, 3), u),
                              datasets.sample_surface_from_uniforms(v, f, u))
    # pred takes the part home when the prediction equals the ground truth: R R^T = I up to the float32 rounding of the
    # matrix entries (<= 3e-7 each, so <= 2e-6 per entry of the product) times |v - T| <= 2, and one rounding of the result
    home = assemble.pose_meshes(store, slot_part, gt_quat, gt_trans, gt_quat, gt_trans).to_host()
    assert np.abs(home[2] - home[0]).max() < 1e-5
    # rot_type 'rmat' takes the matrices as they are
    as_rmat = assemble.pose_meshes(store, slot_part, gt_quat, gt_trans, p_rmat.reshape(6, 3, 3), pred_trans, rot_type="rmat")
    assert np.array_equal(bits(as_rmat.to_host()[2]), bits(got[2]))


def test_mesh_pose_parts_leaves_other_slots_alone(cuda_device, mesh_case):
    store, parts, slot_part, gt_quat, gt_trans, pred_quat, pred_trans = mesh_case
    only = np.where(np.arange(6) == 3, slot_part, -1)  # the same poses, one slot selected
    res = assemble.pose_meshes(store, only, gt_quat, gt_trans, pred_quat, pred_trans)
    assert res.face_off.tolist() == [0, 0, 0, 0, 65, 65, 65] and res.pred.shape == (65, 3, 3)
    full = assemble.pose_meshes(store, slot_part, gt_quat, gt_trans, pred_quat, pred_trans)
    a = full.face_off[3]
    assert torch.equal(res.pred, full.pred[a:a + 65]) and torch.equal(res.input, full.input[a:a + 65])


# ---- the tool -----------------------------------------------------------------------------------------------------------------
def test_visualize_tool_end_to_end(cuda_device, tmp_path):
    """tools/visualize.py on 6 synthetic shapes written as fracture folders, an untrained model, --vis 2."""
    vis = load_tool("visualize")
    counts = [2, 4, 3, 2, 4, 3]
    shapes = synthetic.make_fracture_meshes(7, 6, counts, 40)
    folders = []
    for s, parts in enumerate(shapes):
        rel = os.path.join("everyday", "Bottle" if s < 4 else "Cup", f"shape{s}", "fractured_0")
        os.makedirs(tmp_path / "data" / rel)
        for k, (v, f) in enumerate(parts):
            assemble.write_obj(tmp_path / "data" / rel / f"piece_{k}.obj", v[f])
        folders.append(os.path.dirname(rel))
    (tmp_path / "data" / "val.txt").write_text("\n".join(folders) + "\n")
    cfg = config.pn_transformer_everyday()
    cfg.model.pc_feat_dim, cfg.model.transformer_feat_dim = 64, 128
    cfg.model.transformer_heads, cfg.model.transformer_layers = 4, 2
    torch.manual_seed(5)
    model = build_model(cfg)
    torch.save(model.state_dict(), tmp_path / "weights.pt")
    config.vis_test_preset = lambda: cfg.clone()
    try:
        written = vis.main(["--preset", "vis_test_preset", "--weight", str(tmp_path / "weights.pt"), "--data-dir",
                            str(tmp_path / "data"), "--data-fn", "val.txt", "--max-num-part", "4", "--num-points", "50",
                            "--vis", "2", "--out", str(tmp_path / "out")])
    finally:
        del config.vis_test_preset
    root = tmp_path / "out" / "all"
    assert sorted(os.listdir(root)) == sorted(os.path.basename(w) for w in written) and len(written) == 2
    # what the tool must have computed, from the library directly
    run = cfg.clone()
    run.data.max_num_part, run.data.num_pc_points = 4, 50
    model = build_model(run).to(cuda_device)
    model.load_state_dict(torch.load(tmp_path / "weights.pt"))
    listed = datasets.read_fracture_list(str(tmp_path / "data"), "val.txt", "", 2, 4)
    store = datasets.MeshStore.from_folders(str(tmp_path / "data"), listed, 2, 4)
    prod = datasets.DeviceGeometryProducer(store, num_points=50, max_num_part=4, data_keys=run.data.data_keys,
                                           device=cuda_device)
    batch = prod.batch(list(range(6)), batch_counter=0)
    records = assemble.rank_assemblies(model, [batch], top=2)
    crit = [r["criterion"] for r in assemble.rank_assemblies(model, [batch])]
    assert len(crit) == 6 and crit == sorted(crit) and [r["criterion"] for r in records] == crit[:2]
    for rank, rec in enumerate(records):
        i = int(rec["data_id"])
        p = int(rec["part_valids"].sum())
        assert p == store.shape_part_off[i + 1] - store.shape_part_off[i]
        shape = "-".join(listed[i].split(os.sep)[-2:])
        target = root / f"rank{rank}-{p}pcs-{shape}"
        names = [f"piece_{k}" for k in range(p)]
        want_files = {"assembly.ply"} | {f"{pre}{n}.obj" for n in names for pre in ("", "input_", "pred_")} | {
            f"{pre}{n}.ply" for n in names for pre in ("input_", "pred_")}
        assert set(os.listdir(target)) == want_files
        meshes = assemble.pose_meshes(store, prod.slot_parts([i]), rec["gt_quat"], rec["gt_trans"], rec["pred_quat"],
                                      rec["pred_trans"])
        tri = meshes.to_host()
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda_device)
        clouds = assemble.assemble_clouds(batch["part_pcs"][i][None], t(rec["part_valids"]).float()[None],
                                          t(rec["pred_quat"])[None], t(rec["pred_trans"])[None], t(rec["gt_quat"])[None],
                                          t(rec["gt_trans"])[None], t(np.array(run.data.colors, dtype=np.float32)),
                                          rot_type="quat")
        rows, off = clouds.to_host()
        for k, n in enumerate(names):
            orig, inp, pred = meshes.slot(tri, k)
            for pre, want in (("", orig), ("input_", inp), ("pred_", pred)):
                v, f = datasets.load_obj(target / f"{pre}{n}.obj")
                assert np.array_equal(v.astype(np.float32).reshape(-1, 3, 3), want) and len(f) == len(want)
            assert np.array_equal(bits(read_ply(target / f"pred_{n}.ply")[0]), bits(rows[0, k * 50:(k + 1) * 50, :3]))
            assert np.array_equal(bits(read_ply(target / f"input_{n}.ply")[0]),
                                  bits(batch["part_pcs"][i, k].cpu().numpy()))
        fig_xyz, fig_rgb = read_ply(target / "assembly.ply")
        fig = assemble.assembly_figure(*clouds.to_lists())[0]
        assert np.array_equal(fig_xyz, fig[:, :3].astype(np.float32)) and np.array_equal(fig_rgb, fig[:, 3:].astype(np.uint8))
