"""Host side of the fused evaluation metrics (csrc/eval_metrics.hip): the ABI surface, the composition `assembly_metrics`
falls back to, the models' `state_dict` key sets against the reference's recorded lists, and the identity baseline.
Nothing here needs a GPU; the kernels themselves are checked in tests/test_eval_metrics_gpu.py."""
import json
import re
import warnings
from pathlib import Path

import pytest
import torch

from multi_part_assembly_amd import _lib, config, eval_utils
from multi_part_assembly_amd.pn_transformer import build_model
from multi_part_assembly_amd.rotation import Rotation3D, quat_to_matrix

GOLDEN = Path(__file__).resolve().parent / "golden"

NEW_SYMBOLS = ("mpa_assembly_metrics_workspace", "mpa_assembly_metrics", "mpa_assembly_metrics_rmat", "mpa_connectivity_acc")


def test_abi_version_is_still_10():
    assert _lib.ABI_VERSION == 10
    assert re.search(r"#define MPA_ABI_VERSION 10\b", _lib.HEADER_PATH.read_text())


def test_new_symbols_are_declared_on_both_sides():
    declared = _lib.declared_functions()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is missing from include/mpa_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
    assert sorted(_lib.SIGNATURES) == declared


def test_new_entry_points_validate_their_arguments_without_a_gpu():
    import ctypes
    from multi_part_assembly_amd import _build
    _build.build()
    L = _lib.lib()
    n = ctypes.c_int64()
    assert L.mpa_assembly_metrics_workspace(32, 20, ctypes.byref(n)) == 0 and n.value == 8 * 7 * 32 * 20
    args = [None] * 6
    assert L.mpa_assembly_metrics(*args, 0, 20, 1000, None, None, None, None) == 0  # empty batch: nothing to do
    assert L.mpa_assembly_metrics(*args, 2, 20, 4096, None, None, None, None) == -1 and b"2048" in L.mpa_last_error()
    assert L.mpa_assembly_metrics_rmat(*args, 2, 20, 1000, None, None, None, None) == -1 and b"null" in L.mpa_last_error()
    assert L.mpa_connectivity_acc(None, None, None, 0, 2, 20, None, None) == -1 and b"null" in L.mpa_last_error()
    assert L.mpa_connectivity_acc(None, None, None, 0, 0, 20, None, None) == 0


# ---- CPU stand-ins of the two HIP operators behind calc_part_acc (there is no CPU Chamfer / pose kernel in the package) ----
def _cpu_transform_pc(trans, rot, pc, rot_type=None):
    if rot_type is None:
        rot, rot_type = rot.rot, rot.rot_type
    r = quat_to_matrix(rot) if rot_type == "quat" else rot
    return (r[..., None, :, :] @ pc[..., None]).squeeze(-1) + trans[..., None, :]


def _cpu_chamfer(a, b):
    d = torch.cdist(a, b) ** 2
    return d.min(2)[0], d.min(1)[0]


def _inputs(seed=5, B=3, P=4, N=24):
    g = torch.Generator().manual_seed(seed)
    valids = torch.tensor([[1.0, 1, 0, 0], [1, 1, 1, 1], [1, 1, 1, 0]])
    pts = torch.randn(B, P, N, 3, generator=g) * 0.1 * valids[..., None, None]
    gt_t = torch.randn(B, P, 3, generator=g) * 0.3
    pr_t = gt_t + torch.randn(B, P, 3, generator=g) * torch.tensor([0.0, 0.01, 0.2, 1.0])[None, :, None]
    gt_q = torch.nn.functional.normalize(torch.randn(B, P, 4, generator=g), dim=-1)
    pr_q = torch.nn.functional.normalize(gt_q + 0.1 * torch.randn(B, P, 4, generator=g), dim=-1)
    return pts, pr_t, gt_t, pr_q, gt_q, valids


@pytest.mark.parametrize("rot_type", ["quat", "rmat"])
def test_assembly_metrics_on_the_cpu_is_the_composition_bit_for_bit(monkeypatch, rot_type):
    monkeypatch.setattr(eval_utils, "transform_pc", _cpu_transform_pc)
    monkeypatch.setattr(eval_utils, "chamfer_distance", _cpu_chamfer)
    monkeypatch.setattr(eval_utils, "_warned", set())
    pts, pr_t, gt_t, pr_q, gt_q, valids = _inputs()
    pr_r, gt_r = Rotation3D(pr_q).convert(rot_type), Rotation3D(gt_q).convert(rot_type)
    with pytest.warns(UserWarning, match="assembly_metrics") as rec:
        got = eval_utils.assembly_metrics(pts, pr_t, gt_t, pr_r, gt_r, valids)
        again = eval_utils.assembly_metrics(pts, pr_t, gt_t, pr_r, gt_r, valids)
    assert len([w for w in rec if "assembly_metrics" in str(w.message)]) == 1  # the single warning
    want = {"part_acc": eval_utils.calc_part_acc(pts, pr_t, gt_t, pr_r, gt_r, valids)}
    for m in ("mse", "rmse", "mae"):
        want[f"trans_{m}"] = eval_utils.trans_metrics(pr_t, gt_t, valids, m)
        want[f"rot_{m}"] = eval_utils.rot_metrics(pr_r, gt_r, valids, m)
    assert set(got) == set(want) == set(eval_utils.METRIC_KEYS)
    for k in want:
        assert got[k].shape == (3,) and torch.equal(got[k], want[k]), k
        assert torch.equal(again[k], want[k]), k
    assert 0.0 < float(got["part_acc"].mean()) < 1.0  # the inputs mix correct and wrong parts


def test_connectivity_dispatch_on_the_cpu_is_the_composition(monkeypatch):
    monkeypatch.setattr(eval_utils, "transform_pc", _cpu_transform_pc)
    monkeypatch.setattr(eval_utils, "_warned", set())
    _, pr_t, _, pr_q, _, _ = _inputs()
    g = torch.Generator().manual_seed(9)
    contact = torch.zeros(3, 4, 4, 4)
    contact[..., 0] = (torch.rand(3, 4, 4, generator=g) < 0.4).float()
    contact[..., 1:] = torch.randn(3, 4, 4, 3, generator=g) * 0.2
    rot = Rotation3D(pr_q)
    want = eval_utils.calc_connectivity_acc(pr_t, rot, contact)
    with pytest.warns(UserWarning, match="calc_connectivity_acc"):
        got = eval_utils.calc_connectivity_acc(pr_t, rot, contact, fused=True)
    assert torch.equal(got, want)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the default path stays silent, and the fused one has warned already
        eval_utils.calc_connectivity_acc(pr_t, rot, contact)
        eval_utils.calc_connectivity_acc(pr_t, rot, contact, fused=True)


# ---- state_dict key sets ----------------------------------------------------------------------------------------------------
def _recorded():
    return json.loads((GOLDEN / "state_dict_keys.json").read_text())


@pytest.mark.parametrize("preset", ["pn_transformer_everyday", "pn_transformer_refine_everyday", "global_everyday",
                                    "global_partnet_chair", "dgl_everyday", "dgl_dgcnn_everyday", "rgl_net_everyday",
                                    "lstm_everyday", "lstm_partnet_chair", "identity_everyday"])
def test_state_dict_keys_equal_the_reference_list(preset):
    """A reference checkpoint then loads with strict key matching.  `num_batches_tracked` buffers are ignored only where the
    reference's list has none for that module."""
    want = set(_recorded()["state_dict_keys"][preset])
    got = set(build_model(getattr(config, preset)()).state_dict().keys())
    extra = {k for k in got - want if k.endswith(".num_batches_tracked")}
    assert got - extra == want, (sorted(got - extra - want)[:8], sorted(want - got)[:8])


# ---- the identity baseline ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", ["identity_everyday", "identity_artifact", "identity_partnet_chair"])
def test_identity_model_predicts_the_zero_pose(preset):
    cfg = getattr(config, preset)()
    model = build_model(cfg)
    from multi_part_assembly_amd.identity import IdentityModel
    assert isinstance(model, IdentityModel) and list(model.parameters()) == [] and model.state_dict() == {}
    assert model.load_state_dict({"anything": torch.zeros(1)}) is None  # a no-op, whatever it is given
    assert model.semantic == (preset == "identity_partnet_chair") and model.sample_iter == 5
    out = model.forward({"part_pcs": torch.randn(2, 3, 8, 3)})
    assert out["trans"].shape == (2, 3, 3) and not out["trans"].any()
    assert torch.equal(out["rot"].rot, torch.tensor([1.0, 0, 0, 0]).expand(2, 3, 4))
    cfg.model.rot_type = "rmat"
    out = build_model(cfg).forward({"part_pcs": torch.randn(2, 3, 8, 3)})
    assert torch.equal(out["rot"].rot, torch.eye(3).expand(2, 3, 3, 3))


def test_fixture_records_the_margins_its_generator_asserted():
    """make_golden_eval.py asserts in float64 that nothing sits within 1 % of a 0.01 threshold and that no rotation is
    near the asin pole; the figures of the accepted draw travel with the fixture."""
    import numpy as np
    z = np.load(Path(__file__).resolve().parent / "golden" / "eval_metrics_v2.npz")
    for case in ("big", "small"):
        chamfer_margin, contact_margin, asin_arg_max = z[f"{case}.margins"].tolist()
        assert chamfer_margin > 0.01 and contact_margin > 0.01 and asin_arg_max <= 0.99, case
