"""The PointNet++ SSG encoder on the MI355X: against the float64 records of the reference's own modules
(tests/golden/pointnet2_ssg.npz, bars of tests/anchored.py with the fixture's float32 records as r32; the device's ReLU
decisions are read out, held to the float64 pre-activations and, where one differs, held fixed in the CPU passes the
gradients are compared with: tests/pointnet2_pinned.py); against the same
module fed by the restatement's indices, grouped tensors and backward sums computed on the host; `forward_parts`; and one
training step of two model families."""
import sys

import numpy as np
import pytest
import torch

import anchored
import pointnet2_pinned
from conftest import GOLDEN
from multi_part_assembly_amd import config, pointnet2_utils as pu, synthetic
from multi_part_assembly_amd.pn_transformer import build_model
from multi_part_assembly_amd.pointnet2 import PointNet2SSG
from multi_part_assembly_amd.trainer import Trainer

sys.path.insert(0, str(GOLDEN))
import param_fill  # noqa: E402

pytestmark = pytest.mark.gpu


def picked(a):
    """The elements `param_fill.compact` keeps of a tensor: all of a small one, a strided sample of a large one."""
    a = a.detach().cpu().reshape(-1)
    if a.numel() <= param_fill.FULL_LIMIT:
        return a
    return a[torch.from_numpy(np.linspace(0, a.numel() - 1, param_fill.SAMPLE).astype(np.int64))]


def records(fixture, prefix):
    out = {}
    for k, v in fixture.items():
        if k.startswith(prefix) and not k.endswith("#norms"):
            out[k[len(prefix):].replace("#sample", "")] = torch.from_numpy(v)
    return out


def run_encoder(fixture, device, decisions=None):
    """`decisions`: a list that receives, per ReLU of the training forward in execution order, where its output is positive."""
    enc = PointNet2SSG(128)
    param_fill.fill_parameters(enc, int(fixture["seed"]))
    enc = enc.to(device).train()
    pts, w = torch.from_numpy(fixture["points"]).to(device), torch.from_numpy(fixture["w"]).to(device)
    levels = []
    hooks = [] if decisions is None else [seq[i].register_forward_hook(lambda m, x, y: decisions.append((y > 0).cpu()))
                                          for seq, i in pointnet2_pinned.relu_slots(enc)]
    out = enc(pts, record=levels)
    for h in hooks:
        h.remove()
    (out * w).sum().backward()
    enc.eval()
    with torch.no_grad():
        out_eval = enc(pts)
    got = {"out.train": out, "out.eval": out_eval}
    for i, (new_xyz, feats) in enumerate(levels):
        if new_xyz is not None:
            got[f"new_xyz.{i}"] = new_xyz
        got[f"features.{i}"] = feats
    got.update({f"stat.{k}": v for k, v in enc.state_dict().items() if "running_" in k})
    got.update({f"grad.{k}": p.grad for k, p in enc.named_parameters()})
    return {k: v.detach().clone() for k, v in got.items()}


def test_encoder_against_the_float64_records_of_the_reference_modules(cuda_device, golden):
    fixture = golden("pointnet2_ssg")
    r32, r64 = records(fixture, "f32."), records(fixture, "f64.")
    decisions = []
    got = {k: picked(v) for k, v in run_encoder(fixture, cuda_device, decisions).items()}
    assert set(got) == set(r64) == set(r32)
    # The ReLU decisions of the device run against the float64 pre-activations (tests/pointnet2_pinned.py): every level has
    # pre-activations within 1e-7 of zero, which no float32-grade evaluation can decide.  The CPU pass is the fixture's
    # float64 pass (its records are stored in float32: 6e-8); a decision may differ from the float64 sign only within
    # FLIP_PREACT of zero; where one does, the gradients are held to the float32 / float64 CPU passes with the device's
    # decisions held fixed instead of the records (with none off, the records themselves: the two are the same pass).
    g64, z64 = pointnet2_pinned.cpu_pass(fixture, torch.float64)
    assert len(decisions) == len(z64) == 9 and set(g64) == {k for k in r64 if k.startswith("grad.")}
    for k, v in g64.items():
        if anchored._zero_scale(k, r64) is None:
            assert anchored.err(picked(v), r64[k]) <= 2e-7, k
    off, off_rel = pointnet2_pinned.sites_off(decisions, z64)
    print(f"ReLU decisions off the float64 sign: {off} of {sum(z.numel() for z in z64)}, largest |z64| / channel maximum {off_rel:.1e}")
    assert off_rel <= anchored.FLIP_PREACT
    if off:
        r64.update({k: picked(v) for k, v in pointnet2_pinned.cpu_pass(fixture, torch.float64, decisions)[0].items()})
        r32.update({k: picked(v) for k, v in pointnet2_pinned.cpu_pass(fixture, torch.float32, decisions)[0].items()})
    rows, bad = anchored.check(got, r32, r64)
    print(anchored.summary("pointnet2_ssg", rows, r32, r64))
    for e, e32, bar, k in sorted(rows, reverse=True)[:8]:
        print(f"  {k}: err {e:.2e}  e32 {e32:.2e}  bar {bar:.2e}")
    assert not bad, "\n".join(bad)
    for i in (0, 1):                                          # the centres are copies: the same points, bit for bit
        assert torch.equal(got[f"new_xyz.{i}"], r32[f"new_xyz.{i}"])


def on_host(fn):
    """`fn` of pointnet2_utils run on host copies of its tensor arguments (the numpy restatement), result back on the device."""
    def call(*args):
        device = next(a.device for a in args if torch.is_tensor(a))
        return fn(*[a.cpu() if torch.is_tensor(a) else a for a in args]).to(device)
    return call


def test_hip_operators_equal_the_restatement_inside_the_encoder(cuda_device, golden, monkeypatch):
    """Both runs use the same library kernels for the shared MLPs on equal inputs: the features are bit-equal, the
    gradients within the project's bar."""
    fixture = golden("pointnet2_ssg")
    hip = run_encoder(fixture, cuda_device)
    for name in ("furthest_point_sample", "ball_query", "_group_forward", "_group_backward"):
        monkeypatch.setattr(pu, name, on_host(getattr(pu, name)))
    host = run_encoder(fixture, cuda_device)
    monkeypatch.undo()
    assert set(hip) == set(host)
    for k in hip:
        if not k.startswith("grad."):
            assert torch.equal(hip[k], host[k]), k
    worst = 0.0
    for k in hip:
        if k.startswith("grad."):
            scale = float(host[k].abs().max())
            if k.endswith(".bias"):  # zero up to rounding in front of a normalisation: relative to the layer's weights
                scale = max(scale, float(host[k[:-len("bias")] + "weight"].abs().max()))
            e = float((hip[k] - host[k]).abs().max()) / scale
            worst = max(worst, e)
            assert e <= anchored.CEIL, (k, e)
    print(f"largest gradient distance HIP operators vs host restatement: {worst:.2e}")


def test_forward_parts_gives_zero_rows_and_never_reads_padded_slots(cuda_device):
    torch.manual_seed(0)
    enc = PointNet2SSG(64).to(cuda_device).train()
    pcs = torch.rand(5, 600, 3, device=cuda_device) - 0.5
    valids = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0], device=cuda_device)
    clean = enc.forward_parts(pcs, valids)
    dirty = pcs.clone()
    dirty[valids == 0] = float("nan")
    for bn in (m for m in enc.modules() if isinstance(m, torch.nn.BatchNorm2d)):
        bn.reset_running_stats()
    out = enc.forward_parts(dirty, valids)
    assert out.shape == (5, 64) and torch.isfinite(out).all()
    assert float(out[1].abs().max()) == 0.0 and float(out[3].abs().max()) == 0.0 and float(out[0].abs().max()) > 0.0
    assert torch.equal(out, clean)
    out.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in enc.parameters())
    assert torch.equal(enc.forward_parts(pcs, torch.zeros(5, device=cuda_device)), torch.zeros(5, 64, device=cuda_device))


@pytest.mark.parametrize("preset", ["pn_transformer_everyday", "dgl_everyday"])
def test_one_training_step(cuda_device, preset):
    cfg = getattr(config, preset)()
    cfg.model.encoder = "pointnet2_ssg"
    cfg.data.max_num_part = 3
    torch.manual_seed(1)
    model = build_model(cfg).to(cuda_device)
    trainer = Trainer(model, cfg)
    batch = synthetic.make_batch(2, max_parts=3, num_points=600, seed=11, device=cuda_device, num_parts=[2, 3])
    batch.pop("num_parts", None)
    loss = trainer._fwd_bwd(batch)
    assert torch.isfinite(loss).item()
    for name, p in model.encoder.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        assert p.dim() == 1 or float(p.grad.abs().max()) > 0.0, name
    before = trainer.flat.flat_param.clone()
    loss = trainer.train_step(batch)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item() and not torch.equal(before, trainer.flat.flat_param)
