"""tests/eval_ref.py (the float64 restatement the GPU tests of csrc/eval_metrics.hip compare with) against the reference's
own recorded outputs, tests/golden/eval_metrics_v2.npz, at both recorded shapes and for both rotation kinds — at the
tolerances tests/test_eval_metrics_gpu.py::test_part_acc_and_trans_metrics_match_reference applies to the kernel: part
accuracy and connectivity exactly, translation metrics to rtol 1e-5, rotation metrics to rtol 2e-4.  The fixture's
generator kept every thresholded value 1 % away from 0.01, so the exact comparisons are fair.  No GPU."""
import numpy as np
import pytest
import torch

import eval_ref
from multi_part_assembly_amd import eval_utils
from multi_part_assembly_amd.rotation import Rotation3D, quat_to_matrix

CASES = [(shape, kind) for shape in ("big", "small") for kind in ("quat", "rmat")]


def _load(golden, shape, kind):
    z = golden("eval_metrics_v2")
    pre = f"{shape}.{kind}."
    t = lambda k: torch.from_numpy(z[k].copy())
    return z, pre, dict(pcs=t(f"{shape}.pcs"), valids=t(f"{shape}.valids"), gt_t=t(f"{shape}.gt_t"), pr_t=t(f"{shape}.pr_t"),
                        contact=t(f"{shape}.contact_points"), pr_r=t(pre + "pr_rot"), gt_r=t(pre + "gt_rot"))


@pytest.mark.parametrize("shape,kind", CASES)
def test_part_accuracy_reproduces_the_recorded_values_exactly(golden, shape, kind):
    z, pre, d = _load(golden, shape, kind)
    a = eval_ref.pose64(d["pr_t"], d["pr_r"], kind, d["pcs"])
    b = eval_ref.pose64(d["gt_t"], d["gt_r"], kind, d["pcs"])
    per_part = eval_ref.chamfer_per_part(a, b)
    assert per_part.shape == d["valids"].shape
    margin = eval_ref.threshold_margin(per_part[d["valids"] == 1])
    assert margin > 0.009, margin  # the generator asserted 1 % on its own float64 posing
    ok, n = eval_ref.part_acc_counts(per_part, d["valids"])
    assert ok.dtype == n.dtype == torch.int64
    np.testing.assert_array_equal(eval_ref.ratio32(ok, n), z[pre + "part_acc"])
    assert 0 < int(ok.sum()) < int(n.sum())  # the case decides something


@pytest.mark.parametrize("shape,kind", CASES)
def test_translation_and_rotation_metrics_reproduce_the_recorded_values(golden, shape, kind):
    z, pre, d = _load(golden, shape, kind)
    tr = eval_ref.trans_metrics(d["pr_t"], d["gt_t"], d["valids"])
    ro = eval_ref.rot_metrics(d["pr_r"], d["gt_r"], kind, d["valids"])
    for m in ("mse", "rmse", "mae"):
        assert tr[m].dtype == ro[m].dtype == torch.float64
        np.testing.assert_allclose(tr[m].numpy(), z[pre + f"trans_{m}"], rtol=1e-5, err_msg=m)
        np.testing.assert_allclose(ro[m].numpy(), z[pre + f"rot_{m}"], rtol=2e-4, err_msg=m)


@pytest.mark.parametrize("shape,kind", CASES)
def test_connectivity_reproduces_the_recorded_values_exactly(golden, shape, kind):
    z, pre, d = _load(golden, shape, kind)
    B, P = d["valids"].shape
    hits, contacts, dist = eval_ref.connectivity(d["pr_t"], d["pr_r"], kind, d["contact"])
    assert contacts == int((d["contact"][..., 0] == 1).sum()) == dist.numel() and 0 < hits < contacts
    assert eval_ref.threshold_margin(dist) > 0.009
    np.testing.assert_array_equal(np.full(B, eval_ref.ratio32(hits, contacts)), z[pre + "connectivity_acc_pred"])
    ident = torch.tensor([1.0, 0, 0, 0]).repeat(B, P, 1)
    ident = ident if kind == "quat" else quat_to_matrix(ident)
    hits, contacts, dist = eval_ref.connectivity(torch.zeros_like(d["pr_t"]), ident, kind, d["contact"])
    assert eval_ref.threshold_margin(dist) > 0.009
    np.testing.assert_array_equal(np.full(B, eval_ref.ratio32(hits, contacts)), z[pre + "connectivity_acc_zero"])


def test_counts_and_means_follow_the_value_of_valids():
    """Part accuracy counts valids == 1 only; `_valid_mean` weights by the value; no valid part gives 0 / 0 = NaN."""
    valids = torch.tensor([[1.0, 0.5, 2.0, 0.0], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 0.0, 1.0]])
    per_part = torch.tensor([[0.02, 0.001, 0.001, 0.001], [0.001] * 4, [0.001, 0.0099, 0.001, 0.01]], dtype=torch.float64)
    ok, n = eval_ref.part_acc_counts(per_part, valids)
    assert ok.tolist() == [0, 0, 2] and n.tolist() == [1, 0, 3]
    acc = eval_ref.ratio32(ok, n)
    assert acc.dtype == np.float32 and acc[0] == 0.0 and np.isnan(acc[1]) and acc[2] == np.float32(2) / np.float32(3)
    mean = eval_ref.valid_mean(torch.tensor([[1.0, 2.0, 3.0, 100.0], [1.0] * 4, [1.0, 2.0, 100.0, 4.0]]), valids)
    assert mean[0] == (1.0 + 0.5 * 2.0 + 2.0 * 3.0) / 3.5 and torch.isnan(mean[1]) and mean[2] == 7.0 / 3.0
    # the same from the package's float32 composition
    comp = eval_utils._valid_mean(torch.tensor([[1.0, 2.0, 3.0, 100.0], [1.0] * 4, [1.0, 2.0, 100.0, 4.0]]), valids)
    np.testing.assert_allclose(comp.numpy(), mean.numpy(), rtol=1e-6, equal_nan=True)


def test_constructor_rule_after_matrix_to_quaternion():
    """The candidate magnitudes of matrix_to_quaternion satisfy sum_k s_k = 4, so the chosen component is >= 0.5 and
    the rule `norm <= 0.5 -> identity` can fire only where every s_k = 1 and the matrix is symmetric with a zero
    diagonal — in practice the all-zero matrix of a padded slot (quaternion (0.5, 0, 0, 0), norm exactly 0.5).  A scaled
    rotation such as 0.3 R keeps norm > 0.5 and is NOT replaced.  Both hold for the float32 composition as well."""
    g = torch.Generator().manual_seed(11)
    q = torch.nn.functional.normalize(torch.randn(6, 4, generator=g), dim=-1)
    R = quat_to_matrix(q)
    mats = torch.cat([torch.zeros(1, 3, 3), 0.3 * R, R])
    got = eval_ref.to_quat(mats, "rmat")
    assert got.dtype == torch.float64
    assert got[0].tolist() == [1.0, 0.0, 0.0, 0.0]
    raw = eval_ref.rotation.matrix_to_quaternion(mats.double())
    assert float(raw[0].norm()) == 0.5 and float(raw[1:].norm(dim=-1).min()) > 0.5
    assert torch.equal(got[1:], raw[1:])
    np.testing.assert_allclose(eval_ref.matrix_candidates(mats).pow(2).sum(-1).numpy(), 4.0, rtol=1e-12)
    comp = Rotation3D(mats, "rmat").to_quat()
    np.testing.assert_allclose(comp.numpy(), got.numpy(), atol=2e-6)
    # and the metrics built on it agree with the float32 composition
    valids = torch.ones(1, 13)
    pr, gt = mats[None], mats.flip(0)[None]
    want = eval_ref.rot_metrics(pr, gt, "rmat", valids)
    for m in ("mse", "rmse", "mae"):
        comp = eval_utils.rot_metrics(Rotation3D(pr, "rmat"), Rotation3D(gt, "rmat"), valids, m)
        np.testing.assert_allclose(comp.numpy(), want[m].numpy(), rtol=2e-4, err_msg=m)


def test_chamfer_value_of_a_shifted_lattice_is_twice_the_squared_shift():
    """Every point's nearest neighbour in a copy shifted by less than half the spacing is its own image."""
    k = torch.arange(5, dtype=torch.float64) * 0.25
    a = torch.cartesian_prod(k, k, k)[:37]
    shift = torch.tensor([0.03, -0.05, 0.02], dtype=torch.float64)
    got = eval_ref.chamfer_per_part(a[None], (a + shift)[None])
    np.testing.assert_allclose(got.numpy(), [2 * float(shift.pow(2).sum())], rtol=1e-12)
    assert eval_ref.chamfer_per_part(a[None, :1], a[None, :1]).tolist() == [0.0]  # N = 1, identical
