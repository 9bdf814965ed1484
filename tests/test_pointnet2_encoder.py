"""CPU checks of the PointNet++ SSG encoder (multi_part_assembly_amd/pointnet2.py) against tests/golden/pointnet2_ssg.npz,
the record of the reference's own `PointNet2SSG` run over this package's operator module on its host path
(tests/golden/make_golden_pointnet2.py): same torch CPU operators on the same values, so the float32 records are matched at
rel = 1e-5 and no selection can flip.  Plus the registry, the model families and the trainer's graph-mode fall-back."""
import copy
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from multi_part_assembly_amd import config
from multi_part_assembly_amd.encoder import DGCNN, PointNet, build_encoder
from multi_part_assembly_amd.pn_transformer import build_model
from multi_part_assembly_amd.pointnet2 import PointNet2SSG

sys.path.insert(0, str(GOLDEN))
import param_fill  # noqa: E402

REL = 1e-5


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("pointnet2_ssg")


@pytest.fixture(scope="module")
def cpu_run(fixture):
    """One training forward + backward and one eval forward of the encoder on the fixture's inputs, shared."""
    enc = PointNet2SSG(128)
    param_fill.fill_parameters(enc, int(fixture["seed"]))
    enc.train()
    pts, w = torch.from_numpy(fixture["points"]), torch.from_numpy(fixture["w"])
    levels = []
    out = enc(pts, record=levels)
    (out * w).sum().backward()
    enc.eval()
    with torch.no_grad():
        out_eval = enc(pts)
    return enc, out, out_eval, levels


def test_state_dict_names_and_shapes_equal_the_reference(fixture):
    sd = PointNet2SSG(128).state_dict()
    assert list(sd) == fixture["names"].tolist()
    assert [",".join(map(str, v.shape)) for v in sd.values()] == fixture["shapes"].tolist()
    for i in range(3):
        for j in (0, 1, 3, 4, 6, 7):
            assert f"SA_modules.{i}.mlps.0.{j}.weight" in sd
    assert sd["SA_modules.1.mlps.0.0.weight"].shape == (128, 131, 1, 1)
    assert sd["SA_modules.2.mlps.0.6.weight"].shape == (128, 512, 1, 1)


def test_features_and_levels_match_the_reference_records(fixture, cpu_run):
    _, out, out_eval, levels = cpu_run
    assert out.shape == (3, 128) and out.dtype == torch.float32
    param_fill.compare(fixture, "f32.", "out.train", out.detach().numpy(), REL)
    param_fill.compare(fixture, "f32.", "out.eval", out_eval.numpy(), REL)
    assert [None if x is None else tuple(x.shape) for x, _ in levels] == [(3, 512, 3), (3, 128, 3), None]
    assert [tuple(f.shape) for _, f in levels] == [(3, 128, 512), (3, 256, 128), (3, 128, 1)]
    for i, (new_xyz, feats) in enumerate(levels):
        if new_xyz is not None:
            param_fill.compare(fixture, "f32.", f"new_xyz.{i}", new_xyz.detach().numpy(), REL)
        param_fill.compare(fixture, "f32.", f"features.{i}", feats.detach().numpy(), REL)
    # the zero rows of cloud 0 are never sampled
    assert float(levels[0][0][0].abs().sum(dim=-1).min()) > 0


def test_running_statistics_and_gradients_match_the_reference_records(fixture, cpu_run):
    enc = cpu_run[0]
    seen = 0
    for k, v in enc.state_dict().items():
        if "running_" in k:
            param_fill.compare(fixture, "f32.", f"stat.{k}", v.numpy(), REL)
            seen += 1
        elif k.endswith("num_batches_tracked"):
            assert int(v) == 1
    assert seen == 18
    for k, p in enc.named_parameters():
        assert p.grad is not None, k
        floor = 0.0
        if k.endswith(".bias"):  # a bias gradient that is zero up to rounding is held relative to its layer's weight gradient
            floor = float(dict(enc.named_parameters())[k[:-len("bias")] + "weight"].grad.abs().max())
        param_fill.compare(fixture, "f32.", f"grad.{k}", p.grad.numpy(), REL, floor=floor)


def test_pinned_relu_decisions_reproduce_the_pass_and_follow_a_flip(fixture):
    """tests/pointnet2_pinned.py, the anchor of the GPU test where the device decides a ReLU the other way: in float64
    the free pass is the fixture's float64 pass (records stored in float32), pinned at its own decisions it reproduces
    itself bit for bit, every level has a pre-activation below float32 rounding, and ONE decision flipped at the smallest
    pre-activation of SA2's first ReLU moves that layer's BatchNorm bias gradient by more than 1e-3 — the distance a
    float32-grade run that takes that decision shows against the unpinned records."""
    import anchored
    import pointnet2_pinned as pp
    from test_pointnet2_encoder_gpu import picked, records
    r64 = records(fixture, "f64.")
    g64, z64 = pp.cpu_pass(fixture, torch.float64)
    assert len(z64) == 9 and set(g64) == {k for k in r64 if k.startswith("grad.")}
    for k, v in g64.items():
        if anchored._zero_scale(k, r64) is None:
            assert anchored.err(picked(v), r64[k]) <= 2e-7, k
    own = [z > 0 for z in z64]
    assert pp.sites_off(own, z64) == (0, 0.0)
    again, _ = pp.cpu_pass(fixture, torch.float64, own)
    assert all(torch.equal(again[k], g64[k]) for k in g64)
    rel = z64[3].abs() / z64[3].abs().amax(dim=(0, 2, 3), keepdim=True)
    assert float(rel.min()) < 2.0 ** -24
    flipped = list(own)
    flipped[3] = own[3].clone()
    flipped[3].view(-1)[rel.flatten().argmin()] ^= True
    assert pp.sites_off(flipped, z64) == (1, float(rel.min()))
    moved, _ = pp.cpu_pass(fixture, torch.float64, flipped)
    assert anchored.err(moved["grad.SA_modules.1.mlps.0.1.bias"], g64["grad.SA_modules.1.mlps.0.1.bias"]) > 1e-3
    for k in ("grad.SA_modules.1.mlps.0.3.weight", "grad.SA_modules.2.mlps.0.0.weight"):  # above the site: the value did not move
        assert anchored.err(moved[k], g64[k]) < 1e-6, k


def test_forward_parts_runs_the_valid_parts_only():
    enc = PointNet2SSG(64).train()
    twin = copy.deepcopy(enc)
    g = torch.Generator().manual_seed(0)
    pcs = torch.rand(4, 80, 3, generator=g) + 0.2
    pcs[1] = float("nan")                                     # a padded slot is never read
    valids = torch.tensor([1.0, 0.0, 1.0, 1.0])
    out = enc.forward_parts(pcs, valids)
    assert out.shape == (4, 64) and torch.isfinite(out).all() and float(out[1].detach().abs().max()) == 0.0
    assert torch.equal(twin(pcs[[0, 2, 3]]), out[[0, 2, 3]])  # (training-mode BatchNorm: the batch is the valid parts)
    assert enc.host_sync_per_forward is True


def test_registry():
    enc = build_encoder("pointnet2_ssg", 256)
    assert isinstance(enc, PointNet2SSG) and enc.feat_dim == 256
    with pytest.raises(NotImplementedError, match="MSG"):
        build_encoder("pointnet2_msg", 256)
    with pytest.raises(NotImplementedError):
        build_encoder("pointnet3", 256)
    assert isinstance(build_encoder("pointnet", 128), PointNet) and isinstance(build_encoder("dgcnn", 128), DGCNN)


@pytest.mark.parametrize("preset", ["pn_transformer_everyday", "pn_transformer_refine_everyday", "global_everyday",
                                    "dgl_everyday", "rgl_net_everyday", "lstm_everyday"])
def test_every_model_family_builds_with_the_encoder(preset):
    cfg = getattr(config, preset)()
    cfg.model.encoder = "pointnet2_ssg"
    model = build_model(cfg)
    assert isinstance(model.encoder, PointNet2SSG) and model.encoder.feat_dim == model.pc_feat_dim
    if preset == "global_everyday":
        assert isinstance(model.global_encoder, PointNet2SSG)
    assert any(k.startswith("encoder.SA_modules.2.mlps.0.7.") for k in model.state_dict())


def test_graph_mode_warns_and_runs_eager():
    from multi_part_assembly_amd.trainer import Trainer

    cfg = config.pn_transformer_everyday()
    cfg.model.encoder = "pointnet2_ssg"
    model = build_model(cfg)
    with pytest.warns(UserWarning, match="use_graph=True is not available for PNTransformer"):
        trainer = Trainer(model, cfg, use_graph=True)
    assert trainer.use_graph is False
    cfg = config.pn_transformer_everyday()                    # the PointNet encoder keeps its captured step
    assert Trainer(build_model(cfg), cfg, use_graph=True).use_graph is True
