"""The contact table computed from clouds and poses: the numpy restatement (`contacts_ref`) against a float64 brute
force, its tie rule, structure and threshold edge, the invariant that the ground-truth poses score a connectivity accuracy
of exactly 1 on a generated table, and the host-side plumbing (ABI table, argument checks, the new data key, the metrics
of a geometry model, the tools' arguments).  No GPU: the wrapper's host path runs the restatement."""
import warnings

import numpy as np
import pytest
import torch

from multi_part_assembly_amd import _lib, contacts, contacts_ref, datasets, eval_utils, synthetic
from multi_part_assembly_amd.base_model import BaseModel
from multi_part_assembly_amd.evaluate import PAPER_METRICS, evaluate_categories, format_table
from multi_part_assembly_amd.rotation import Rotation3D, quat_to_matrix
from tool_loader import load_tool as _tool

F32 = np.float32


def make_case(seed, B=3, P=4, N=40, spread=0.25, size=0.15):
    """Clouds of `size` around centres `spread` apart with random unit quaternions: some pairs touch, some do not."""
    rng = np.random.RandomState(seed)
    pcs = (rng.uniform(-1, 1, (B, P, N, 3)) * size).astype(F32)
    quat = rng.standard_normal((B, P, 4))
    quat = (quat / np.linalg.norm(quat, axis=-1, keepdims=True)).astype(F32)
    trans = (rng.uniform(-1, 1, (B, P, 3)) * spread).astype(F32)
    valids = np.ones((B, P), dtype=F32)
    return pcs, valids, quat, trans


def posed_f32(pcs, quat, trans, b, p):
    return contacts_ref.pose_quat(pcs[b, p], contacts_ref.sanitize_quat(quat[b, p]), trans[b, p])


def exact_transform_pc(trans, rot, pc, rot_type=None):
    """`transform_pc` for host tensors with the arithmetic of the pose kernels (the restatement's): what the composed
    `calc_connectivity_acc` evaluates on the device."""
    if rot_type is None:
        rot, rot_type = rot.rot, rot.rot_type
    fn = contacts_ref.pose_quat if rot_type == "quat" else contacts_ref.pose_rmat
    lead = pc.shape[:-2]
    width = (4,) if rot_type == "quat" else (3, 3)
    r, t, v = rot.reshape((-1,) + width).numpy(), trans.reshape(-1, 3).numpy(), pc.reshape((-1,) + pc.shape[-2:]).numpy()
    out = [fn(v[k], r[k], t[k]) for k in range(len(v))]
    return torch.from_numpy(np.stack(out) if out else np.zeros((0,) + pc.shape[-2:], F32)).reshape(lead + pc.shape[-2:])


# ---- the restatement against float64 ----------------------------------------------------------------------------------------
def test_pose_restatement_is_the_float64_rotation_to_rounding():
    pcs, _, quat, trans = make_case(0, B=1, P=2, N=64)
    for p in range(2):
        got = posed_f32(pcs, quat, trans, 0, p).astype(np.float64)
        rmat = quat_to_matrix(torch.from_numpy(quat[0, p]).double()[None])[0].double().numpy()
        want = pcs[0, p].astype(np.float64) @ rmat.T + trans[0, p].astype(np.float64)
        # two Hamilton products and a translation on coordinates below 1: a few dozen roundings of 6e-8 (and the matrix
        # above went through float32)
        assert np.abs(got - want).max() < 2e-6
        rm = quat_to_matrix(torch.from_numpy(quat[0, p])[None])[0].numpy()
        got = contacts_ref.pose_rmat(pcs[0, p], rm, trans[0, p]).astype(np.float64)
        want = pcs[0, p].astype(np.float64) @ rm.astype(np.float64).T + trans[0, p].astype(np.float64)
        assert np.abs(got - want).max() < 1e-6


def test_restatement_equals_float64_brute_force_on_its_posed_clouds():
    """The search itself: on the float32 posed coordinates, float64 distances give the same pair and dmin to 4 ulp.  Clouds
    are redrawn until the best pair beats the runner-up by more than 1e-5 relative in float64, so that the float32
    rounding of the distances (a few 2^-24) cannot change the winner."""
    checked, seed = 0, 100
    while checked < 6:
        seed += 1
        pcs, valids, quat, trans = make_case(seed, B=1, P=3, N=33)
        posed = [posed_f32(pcs, quat, trans, 0, p).astype(np.float64) for p in range(3)]
        want = {}
        for i in range(3):
            for j in range(i + 1, 3):
                d = ((posed[i][:, None] - posed[j][None]) ** 2).sum(-1)
                order = np.sort(d.reshape(-1))
                if not order[1] - order[0] > 1e-5 * order[0]:
                    want = None
                    break
                want[i, j] = (d.min(),) + divmod(int(d.argmin()), d.shape[1])
            if want is None:
                break
        if want is None:
            continue
        checked += 1
        _, dist, index = contacts_ref.contact_points(pcs, valids, quat, trans)
        for (i, j), (d, a, c) in want.items():
            assert (index[0, i, j], index[0, j, i]) == (a, c)
            assert dist[0, i, j] == dist[0, j, i]
            assert abs(float(dist[0, i, j]) - d) <= 4 * float(np.spacing(dist[0, i, j]))


# ---- ties -------------------------------------------------------------------------------------------------------------------
def identity_pose(B, P):
    quat = np.zeros((B, P, 4), dtype=F32)
    quat[..., 0] = 1
    return quat, np.zeros((B, P, 3), dtype=F32)


def duplicated_case():
    """Two parts whose closest points are each stored twice: (3, 7) in part 0, (2, 5) in part 1."""
    rng = np.random.RandomState(3)
    pcs = rng.uniform(0.2, 0.5, (1, 2, 9, 3)).astype(F32)
    pcs[0, 1] *= -1
    pcs[0, 0, 3] = pcs[0, 0, 7] = (0.03125, 0.0, 0.0)
    pcs[0, 1, 2] = pcs[0, 1, 5] = (-0.03125, 0.0, 0.0)
    quat, trans = identity_pose(1, 2)
    return pcs, np.ones((1, 2), dtype=F32), quat, trans


def lattice_case():
    """Two parts holding the same 3 x 3 x 3 lattice (exact in float32) in different orders: 27 pairs at distance 0."""
    grid = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(F32) / 8
    perm = np.random.RandomState(4).permutation(27)
    pcs = np.stack([grid, grid[perm]])[None]
    quat, trans = identity_pose(1, 2)
    return pcs, np.ones((1, 2), dtype=F32), quat, trans, perm


def test_tie_rule_is_lexicographic():
    pcs, valids, quat, trans = duplicated_case()
    table, dist, index = contacts_ref.contact_points(pcs, valids, quat, trans)
    assert (index[0, 0, 1], index[0, 1, 0]) == (3, 2) and dist[0, 0, 1] == F32(0.0625) ** 2
    assert table[0, 0, 1].tolist() == [1, 0.03125, 0, 0] and table[0, 1, 0].tolist() == [1, -0.03125, 0, 0]
    pcs, valids, quat, trans, perm = lattice_case()
    table, dist, index = contacts_ref.contact_points(pcs, valids, quat, trans)
    assert dist[0, 0, 1] == 0 and index[0, 0, 1] == 0 and index[0, 1, 0] == int(np.argmax(perm == 0))
    assert np.array_equal(table[0, 0, 1, 1:], pcs[0, 0, 0]) and np.array_equal(table[0, 1, 0, 1:], pcs[0, 0, 0])


# ---- structure ----------------------------------------------------------------------------------------------------------------
def check_structure(table, dist, index, pcs, valids, thre_sq=F32(0.01)):
    """Everything the definition says about the layout of the three outputs, for any inputs."""
    B, P = valids.shape
    flag = table[..., 0]
    assert set(np.unique(flag)) <= {0.0, 1.0}
    assert np.array_equal(flag, flag.transpose(0, 2, 1)) and np.array_equal(dist, dist.transpose(0, 2, 1))
    real = valids == 1
    pair = real[:, :, None] & real[:, None, :] & ~np.eye(P, dtype=bool)[None]
    assert not table[~pair].any() and (dist[~pair] == F32(1e32)).all() and (index[~pair] == -1).all()
    assert np.array_equal(flag[pair] == 1, dist[pair] < thre_sq)
    assert not table[flag == 0].any()  # rows of non-contacts are zero
    for b, i, j in zip(*np.nonzero(pair)):
        assert 0 <= index[b, i, j] < pcs.shape[2]
        if flag[b, i, j]:
            assert table[b, i, j, 1:].tobytes() == pcs[b, i, index[b, i, j]].tobytes()  # bit copies


def test_structure_with_padding_and_nan_in_padded_slots():
    pcs, valids, quat, trans = make_case(7, B=4, P=5, N=30)
    valids[0] = [1, 0, 1, 1, 0]   # a mask that is no prefix
    valids[1] = [0, 0, 1, 0, 0]   # one real part
    valids[2] = 0                 # none
    quat[3, 1] = 0                # a zero quaternion of a real part: the identity
    out = contacts_ref.contact_points(pcs, valids, quat, trans)
    check_structure(*out, pcs, valids)
    assert out[0][0, 0, 2, 0] + out[0][0, 0, 3, 0] + out[0][0, 2, 3, 0] + out[0][3, ..., 0].sum() > 0  # something touches
    assert not out[0][1].any() and not out[0][2].any()
    ident = quat.copy()
    ident[3, 1] = (1, 0, 0, 0)
    for x, y in zip(out, contacts_ref.contact_points(pcs, valids, ident, trans)):
        assert np.array_equal(x, y)
    dirty = [a.copy() for a in (pcs, quat, trans)]
    for a in dirty:
        a[valids != 1] = np.nan
    for x, y in zip(out, contacts_ref.contact_points(dirty[0], valids, dirty[1], dirty[2])):
        assert np.array_equal(x, y)
    only = contacts_ref.contact_points(pcs, valids, quat, trans, samples=[3])
    assert np.array_equal(only[0][3], out[0][3]) and not only[0][:3].any()


def test_rmat_table_follows_the_matrix_arithmetic():
    pcs, valids, quat, trans = make_case(8, B=2, P=3, N=25)
    rmat = quat_to_matrix(torch.from_numpy(quat)).numpy()
    out = contacts_ref.contact_points(pcs, valids, rmat, trans)
    check_structure(*out, pcs, valids)
    a, c = out[2][0, 0, 1], out[2][0, 1, 0]
    d = contacts_ref.pair_distances(contacts_ref.pose_rmat(pcs[0, 0], rmat[0, 0], trans[0, 0]),
                                    contacts_ref.pose_rmat(pcs[0, 1], rmat[0, 1], trans[0, 1]))
    assert d[a, c] == d.min() == out[1][0, 0, 1]


# ---- the threshold ------------------------------------------------------------------------------------------------------------
def test_threshold_is_strict():
    quat, trans = identity_pose(1, 2)
    valids = np.ones((1, 2), dtype=F32)
    thre = 0.015625  # 0.125 ** 2, exact in float32
    pcs = np.zeros((1, 2, 1, 3), dtype=F32)
    pcs[0, 1, 0, 0] = 0.125
    table, dist, _ = contacts_ref.contact_points(pcs, valids, quat, trans, thre_sq=thre)
    assert dist[0, 0, 1] == F32(thre) and not table.any()
    pcs[0, 1, 0, 0] = np.nextafter(F32(0.125), F32(0))
    table, dist, _ = contacts_ref.contact_points(pcs, valids, quat, trans, thre_sq=thre)
    assert dist[0, 0, 1] < F32(thre) and table[0, 0, 1, 0] == table[0, 1, 0, 0] == 1
    got = contacts.contact_points(torch.from_numpy(pcs), torch.from_numpy(valids), torch.from_numpy(quat),
                                  torch.from_numpy(trans), thre=thre)
    assert np.array_equal(got.numpy(), table)


# ---- the invariant -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["quat", "rmat"])
def test_ground_truth_poses_score_exactly_one_on_their_own_table(monkeypatch, kind):
    monkeypatch.setattr(eval_utils, "transform_pc", exact_transform_pc)
    pcs, valids, quat, trans = make_case(11, B=3, P=5, N=48)
    valids[1, 3:] = 0
    rot = Rotation3D(torch.from_numpy(quat), "quat")
    if kind == "rmat":
        rot = rot.convert("rmat")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        table = contacts.contact_points(torch.from_numpy(pcs), torch.from_numpy(valids), rot, torch.from_numpy(trans))
    want = contacts_ref.contact_points(pcs, valids, rot.rot.numpy(), trans)[0]
    assert np.array_equal(table.numpy(), want) and table[..., 0].sum() >= 2
    assert torch.equal(contacts.adjacency(table), (table[..., 0] == 1).float())
    acc = eval_utils.calc_connectivity_acc(torch.from_numpy(trans), rot, table)
    assert acc.shape == (3,) and (acc == 1.0).all()
    none = contacts.contact_points(torch.from_numpy(pcs), torch.from_numpy(valids), rot, torch.from_numpy(trans), thre=0.0)
    assert not none.any()
    assert torch.isnan(eval_utils.calc_connectivity_acc(torch.from_numpy(trans), rot, none)).all()


# ---- the ABI table and the wrapper's checks -----------------------------------------------------------------------------------
def test_abi_declares_the_operator():
    declared = _lib.declared_functions()
    for name in ("mpa_contact_points", "mpa_contact_points_rmat"):
        assert name in declared and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == 12
    assert _lib.ABI_VERSION == 10
    L = _lib.lib()
    args = (None, None, None, None, 0.01)
    assert L.mpa_contact_points(*args, 0, 4, 8, None, None, None, None) == 0   # B = 0 is a no-op
    for B, P, N, word in ((1, 65, 8, b"part slots"), (1, 4, 2049, b"points per part"), (1, 4, 0, b"points per part"),
                          (-1, 4, 8, b"negative"), (1 << 20, 64, 8, b"2^31"), (1, 4, 8, b"null")):
        assert L.mpa_contact_points(*args, B, P, N, None, None, None, None) == -1 and word in L.mpa_last_error()
        assert L.mpa_contact_points_rmat(*args, B, P, N, None, None, None, None) == -1


def test_wrapper_checks_its_arguments(monkeypatch):
    monkeypatch.setattr(eval_utils, "_warned", set())
    pcs, valids, quat, trans = (torch.from_numpy(a) for a in make_case(1, B=2, P=3, N=6))
    with pytest.raises(ValueError, match="part_pcs must be"):
        contacts.contact_points(pcs[0], valids, quat, trans)
    with pytest.raises(ValueError, match="shape mismatch"):
        contacts.contact_points(pcs, valids[:, :2], quat, trans)
    with pytest.raises(ValueError, match="shape mismatch"):
        contacts.contact_points(pcs, valids, Rotation3D(quat).convert("rmat").rot, trans)  # a matrix tensor is no quaternion
    with pytest.raises(ValueError, match="`out` holds"):
        contacts.contact_points(pcs, valids, quat, trans, return_dist=True, out=(torch.empty(2, 3, 3, 4),))
    with pytest.raises(ValueError, match="`out` tensor must be"):
        contacts.contact_points(pcs, valids, quat, trans, out=torch.empty(2, 3, 3, 3))
    with pytest.warns(UserWarning, match="contact_points") as rec:
        table, dist, index = contacts.contact_points(pcs, valids, quat, trans, return_dist=True, return_index=True)
        out = torch.full((2, 3, 3, 4), 7.0)
        assert contacts.contact_points(pcs, valids, quat, trans, out=out) is out and torch.equal(out, table)
    assert len([w for w in rec if "contact_points" in str(w.message)]) == 1  # the single warning
    assert table.dtype == dist.dtype == torch.float32 and index.dtype == torch.int32
    assert not contacts.supported(pcs) and not contacts.supported(torch.empty(1, 65, 8, 3))


# ---- stores, producers, data keys ----------------------------------------------------------------------------------------------
def test_data_key_and_device_only_paths():
    store = datasets.MeshStore.from_arrays(synthetic.make_fracture_meshes(5, 2, 3, 60), max_num_part=4)
    prod = datasets.DeviceGeometryProducer(store, num_points=16, max_num_part=4, data_keys=("part_ids", "contact_points"),
                                           device="cpu", contact_thre=0.02)
    assert prod.contact_thre == 0.02 and "contact_points" in prod.data_keys
    with pytest.raises(RuntimeError, match="HIP device only"):
        prod.batch([0, 1])
    with pytest.raises(ValueError, match="unknown data bogus"):
        datasets.DeviceGeometryProducer(store, num_points=16, max_num_part=4, data_keys=("bogus",))
    with pytest.raises(ValueError, match="unknown data contact_points"):  # the host producer is left alone
        datasets.GeometryBatchProducer(data_keys=("contact_points",))
    pn = synthetic.make_partnet_like_store(3, max_parts=4, num_points=8, with_contacts=False)
    assert not pn.has_contacts
    with pytest.raises(RuntimeError, match="HIP device only"):
        pn.with_computed_contacts(device="cpu")
    with pytest.raises(RuntimeError, match="HIP device only"):
        synthetic.make_partnet_like_store(3, max_parts=4, num_points=8, with_contacts="computed", device="cpu")
    with pytest.raises(ValueError, match="with_contacts"):
        synthetic.make_partnet_like_store(3, max_parts=4, num_points=8, with_contacts="files")
    assert synthetic.make_partnet_like_store(3, max_parts=4, num_points=8).has_contacts  # True stays the default


# ---- metrics of a geometry model -----------------------------------------------------------------------------------------------
class _Stub:
    semantic, fused_metrics = False, False


def test_calc_metrics_reports_connectivity_for_geometry_batches(monkeypatch):
    monkeypatch.setattr(eval_utils, "transform_pc", exact_transform_pc)
    monkeypatch.setattr(eval_utils, "chamfer_distance",
                        lambda a, b: ((torch.cdist(a, b) ** 2).min(2)[0], (torch.cdist(a, b) ** 2).min(1)[0]))
    pcs, valids, quat, trans = (torch.from_numpy(a) for a in make_case(11, B=2, P=4, N=20))
    gt = Rotation3D(quat)
    batch = {"part_pcs": pcs, "part_valids": valids}
    out = {"trans": trans * 4 + 0.3, "rot": gt}  # the parts pulled apart
    plain = BaseModel._calc_metrics(_Stub(), batch, out, trans, gt)
    assert list(plain) == ["part_acc", "trans_mse", "rot_mse", "trans_rmse", "rot_rmse", "trans_mae", "rot_mae"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        batch["contact_points"] = contacts.contact_points(pcs, valids, gt, trans)
    assert batch["contact_points"][..., 0].sum() > 0
    with_ca = BaseModel._calc_metrics(_Stub(), batch, out, trans, gt)
    assert set(with_ca) == set(plain) | {"connectivity_acc"}
    for k in plain:
        assert torch.equal(plain[k], with_ca[k])
    assert 0.0 <= float(with_ca["connectivity_acc"][0]) < 1.0
    perfect = BaseModel._calc_metrics(_Stub(), batch, {"trans": trans, "rot": gt}, trans, gt)
    assert (perfect["connectivity_acc"] == 1.0).all()


def test_category_table_shows_connectivity_only_when_asked_and_present():
    class Ev:
        def __init__(self, table):
            self.table = table

        def run(self, batches, prefix="val"):
            return {f"{prefix}/{k}": v for k, v in self.table[batches].items()}

    geo = {"Bottle": {"rot_rmse": 80.149, "rot_mae": 68.0, "trans_rmse": 0.15, "trans_mae": 0.12,
                      "transform_pt_cd_loss": 0.0148, "part_acc": 0.2474, "connectivity_acc": 0.3333}}
    plain = evaluate_categories(Ev(geo), lambda c: c, ["Bottle"])
    assert list(plain["metrics"]) == list(PAPER_METRICS)
    with_ca = evaluate_categories(Ev(geo), lambda c: c, ["Bottle"], connectivity=True)
    assert list(with_ca["metrics"]) == list(PAPER_METRICS) + ["connectivity_acc"]
    assert with_ca["metrics"]["connectivity_acc"] == {"values": [33.3], "mean": 33.3}
    assert format_table(with_ca).startswith(format_table(plain)) and "connectivity_acc:\n33.3 & 33.3" in format_table(with_ca)
    del geo["Bottle"]["connectivity_acc"]
    assert evaluate_categories(Ev(geo), lambda c: c, ["Bottle"], connectivity=True) == evaluate_categories(
        Ev(geo), lambda c: c, ["Bottle"])


# ---- the tools' arguments -----------------------------------------------------------------------------------------------------
def test_tools_parse_their_arguments():
    rate = _tool("contact_rate")
    args = rate.parse_args([])
    assert (args.batch, args.parts, args.points, args.calls, args.windows, args.thre, args.out) == (32, 20, 1000, 10, 5, 0.01, "")
    args = rate.parse_args(["--calls", "3", "--windows", "2", "--out", "x.json", "--points", "64"])
    assert (args.calls, args.windows, args.out, args.points) == (3, 2, "x.json", 64)
    ev = _tool("evaluate")
    base = ["--preset", "identity_everyday", "--data-dir", "d", "--data-fn", "f"]
    assert ev.parse_args(base).connectivity is False and ev.parse_args(base + ["--connectivity"]).connectivity is True
