"""The fused evaluation path of the PointNet++ encoder on the MI355X (csrc/pointnet2_sa_mlp.hip): the kernel against the
float64 restatement under the bars of tests/anchored.py (r32 = the float32 library chain on the same indices, so the bar
comes from the library's own distance to float64, never from the kernel), its structural contract, the pack kernel, the
encoder on the fixture, `forward_parts`, stale weights, memory, and the evaluation pass end to end."""
import copy
import os

import numpy as np
import pytest
import torch

import anchored
import sa_mlp_cases as cases
from multi_part_assembly_amd import _lib, assemble, config, synthetic
from multi_part_assembly_amd import pointnet2_fused as fused
from multi_part_assembly_amd.evaluate import Evaluator
from multi_part_assembly_amd.pn_transformer import build_model
from multi_part_assembly_amd.pointnet2 import PointNet2SSG
from multi_part_assembly_amd.trainer import Trainer
from tool_loader import load_tool

pytestmark = pytest.mark.gpu


def dev_call(mlp, xyz, new_xyz, feats, idx, device, out=None):
    """Pack the three layers of `mlp` and run the kernel on device copies of the host tensors."""
    d = lambda t: None if t is None else t.to(device).contiguous()
    mlp = mlp.to(device)
    prs = cases.pairs(mlp)
    packed = [fused.pack_layer(conv, bn) for conv, bn in prs]
    widths = [conv.out_channels for conv, _ in prs]
    if out is None:
        got = fused.sa_mlp_max(d(xyz), d(new_xyz), d(feats), d(idx), packed, widths)
    else:
        M, N, _ = xyz.shape
        S, K = (1, N) if idx is None else idx.shape[1:]
        _lib.launch("mpa_sa_mlp_max_forward", device, d(xyz), d(new_xyz), d(feats), d(idx), M, N, S, K,
                    0 if feats is None else feats.shape[2], *packed, *widths, out)
        got = out
    mlp.cpu()
    return got


# (M, N, S, K, C, widths): every K in {1, 2, 63, 64, 65, 129}, S in {1, 2, 3, 130}, M in {1, 3}, C in {0, 1, 61, 128, 256} and
# every width triple once, and each tile edge crossed once: K below / at / above the tile height of 64 (C1 <= 128) and of
# 32 (C1 > 128), several centres per tile with a ragged last tile (K = 2: 8 centres per tile, 9 centres), a centre walked
# in 2, 3 and 5 tiles, a layer-2 chunk loop of 1 and 4 chunks, 1 to 4 column chunks of layer 3.
GROUPED = [
    (1, 50, 1, 1, 0, (32, 32, 32)),
    (3, 40, 3, 2, 1, (32, 32, 32)),
    (1, 100, 2, 63, 61, (64, 64, 128)),
    (3, 100, 130, 64, 128, (128, 128, 256)),
    (1, 90, 2, 65, 1, (64, 64, 128)),
    (1, 200, 3, 65, 256, (256, 512, 64)),
    (1, 300, 2, 129, 256, (256, 512, 256)),
    (3, 90, 1, 129, 128, (128, 128, 256)),
    (1, 60, 3, 5, 7, (512, 96, 384)),
    (1, 60, 2, 33, 0, (64, 32, 512)),
]
GROUP_ALL = [
    (3, 1, 0, (32, 32, 32)),
    (1, 127, 61, (64, 64, 128)),
    (3, 128, 128, (128, 128, 256)),
    (1, 129, 256, (256, 512, 64)),
    (1, 300, 256, (256, 512, 256)),
]


def _anchored_case(label, mlp, inputs, device, capsys):
    r32, r64 = cases.references(mlp, *inputs)
    got = dev_call(mlp, *inputs, device)
    assert got.shape == r64.shape and got.dtype == torch.float32
    anchored.assert_anchored({"out": got}, {"out": r32}, {"out": r64}, label, capsys)


@pytest.mark.parametrize("case", GROUPED, ids=lambda c: "M{}-N{}-S{}-K{}-C{}-{}".format(*c[:5], "x".join(map(str, c[5]))))
def test_kernel_against_the_float64_restatement_grouped(cuda_device, case, capsys):
    M, N, S, K, C, widths = case
    mlp = cases.make_mlp(C, widths, seed=sum(case[:5]))
    _anchored_case(f"sa_mlp_max {case}", mlp, cases.make_inputs(M, N, S, K, C, seed=7 + sum(case[:5])), cuda_device, capsys)


@pytest.mark.parametrize("case", GROUP_ALL, ids=lambda c: "M{}-N{}-C{}-{}".format(*c[:3], "x".join(map(str, c[3]))))
def test_kernel_against_the_float64_restatement_group_all(cuda_device, case, capsys):
    M, N, C, widths = case
    mlp = cases.make_mlp(C, widths, seed=N + C)
    inputs = cases.make_inputs(M, N, 1, N, C, seed=11 + N + C, group_all=True)
    _anchored_case(f"sa_mlp_max group-all {case}", mlp, inputs, cuda_device, capsys)


# ---- structure -------------------------------------------------------------------------------------------------------------
def test_repeated_equal_and_out_of_range_indices(cuda_device, capsys):
    M, N, S, K, C, widths = 2, 70, 5, 64, 61, (64, 64, 128)
    mlp = cases.make_mlp(C, widths, seed=1)
    xyz, new_xyz, feats, idx = cases.make_inputs(M, N, S, K, C, seed=2)
    idx[0, 0, 9:] = idx[0, 0, :1]                 # a padded ball: the tail repeats the first hit
    idx[0, 1] = 17                                # all equal
    idx[1, 2, 5] = N                              # outside [0, N): a zero row, never dereferenced
    idx[1, 2, 6] = -1
    idx[1, 3] = 2 ** 31 - 1                       # a whole ball outside
    idx[1, 4, 0] = -(2 ** 31)
    _anchored_case("sa_mlp_max structural indices", mlp, (xyz, new_xyz, feats, idx), cuda_device, capsys)
    got = dev_call(mlp, xyz, new_xyz, feats, idx, cuda_device).cpu()
    one = idx.clone()
    one[0, 1, 1:] = 17
    assert torch.equal(got, dev_call(mlp, xyz, new_xyz, feats, one, cuda_device).cpu())
    # the all-equal ball is the MLP of one row; the all-outside ball the MLP of [-centre ; 0]
    single = dev_call(mlp, xyz, new_xyz, feats, idx[:, :, :1].contiguous(), cuda_device).cpu()
    assert torch.equal(got[0, 1], single[0, 1]) and torch.equal(got[1, 3], single[1, 3])


def test_every_output_element_is_written_and_two_runs_are_bit_equal(cuda_device):
    for (M, N, S, K, C, widths) in ((3, 40, 3, 2, 1, (32, 32, 32)), (1, 200, 3, 65, 256, (256, 512, 64))):
        mlp = cases.make_mlp(C, widths, seed=3)
        inputs = cases.make_inputs(M, N, S, K, C, seed=4)
        first = dev_call(mlp, *inputs, cuda_device)
        out = torch.full((M, S, widths[2]), float("nan"), device=cuda_device)
        second = dev_call(mlp, *inputs, cuda_device, out=out)
        assert torch.isfinite(second).all() and torch.equal(first, second)


def test_captured_call_replays_on_changed_inputs(cuda_device):
    M, N, S, K, C, widths = 3, 100, 130, 64, 128, (128, 128, 256)
    mlp = cases.make_mlp(C, widths, seed=5).to(cuda_device)
    prs = cases.pairs(mlp)
    static = [t.to(cuda_device) for t in cases.make_inputs(M, N, S, K, C, seed=6)]

    def run():
        return fused.sa_mlp_max(*static, [fused.pack_layer(conv, bn) for conv, bn in prs], list(widths))

    stream = torch.cuda.Stream(cuda_device)
    stream.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(stream):
        run()                                     # warm-up outside the capture
    torch.cuda.current_stream(cuda_device).wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        captured = run()
    fresh = cases.make_inputs(M, N, S, K, C, seed=60)
    with torch.no_grad():
        for s, f in zip(static, fresh):
            s.copy_(f)
        prs[1][0].weight.mul_(1.25)               # the packing is part of the captured call
        prs[2][1].running_var.add_(0.5)
    graph.replay()
    torch.cuda.synchronize()
    eager = run()
    assert torch.equal(captured, eager)
    before = dev_call(cases.make_mlp(C, widths, seed=5), *cases.make_inputs(M, N, S, K, C, seed=6), cuda_device)
    assert not torch.equal(before, eager)


# ---- the pack kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,widths", [(0, (32, 32, 32)), (61, (64, 96, 128)), (256, (256, 512, 64))])
def test_pack_kernel(cuda_device, C, widths):
    mlp = cases.make_mlp(C, widths, seed=8 + C)
    with torch.no_grad():
        mlp[0].weight[0, 0, 0, 0] = 1.0 + 2.0 ** -23          # all three planes are needed
        mlp[0].weight[1, 0, 0, 0] = 0.0
    host = cases.host_layers(mlp, np.float32)
    mlp = mlp.to(cuda_device)
    for (conv, bn), (W, scale, shift) in zip(cases.pairs(mlp), host):
        cout, cin = W.shape
        nbytes = fused.packed_bytes(cout, cin)
        real = fused.pack_layer(conv, bn)
        assert real.numel() == nbytes and real.dtype == torch.uint8
        # the same call over a sentinel-filled buffer: every byte is written, the padded columns with zeros
        buf = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=cuda_device)
        _lib.launch("mpa_sa_mlp_pack", cuda_device, conv.weight.detach().reshape(cout, cin).contiguous(), bn.weight, bn.bias,
                    bn.running_mean, bn.running_var, float(bn.eps), cout, cin, buf)
        assert torch.equal(buf, real)
        planes, sc, sh = (t.cpu() for t in fused.unpack_layer(buf, cout, cin))
        cinp = planes.shape[2]
        assert cinp % 32 == 0 and cinp - cin < 32
        total = (planes[0] + planes[1]) + planes[2]                      # float32, exact
        assert torch.equal(total[:, :cin], torch.from_numpy(W))
        assert float(planes[:, :, cin:].abs().max()) == 0.0 if cinp > cin else True
        assert torch.equal(planes[0][:, :cin], torch.from_numpy(W).bfloat16().float())
        for got, want in ((sc, scale), (sh, shift)):
            want = torch.from_numpy(want)
            ulp = torch.from_numpy(np.spacing(np.abs(want.numpy()).astype(np.float32)))
            assert bool(((got - want).abs() <= ulp).all())


# ---- the encoder -----------------------------------------------------------------------------------------------------------
def test_encoder_against_the_float64_records(cuda_device, golden, capsys):
    fixture = golden("pointnet2_ssg")
    enc, pts = cases.fixture_encoder(fixture, cuda_device)
    enc.set_eval_mlp("fused")
    with torch.no_grad():
        out = enc(pts)
    r32, r64 = cases.records(fixture, "f32."), cases.records(fixture, "f64.")
    anchored.assert_anchored({"out.eval": cases.picked(out)}, r32, r64, "pointnet2_ssg fused eval", capsys)


def test_encoder_256_and_its_levels_against_a_float64_run(cuda_device, golden, capsys):
    """The anchor is the module itself in float64 on the host (fused mode on host tensors = the restatement, which
    tests/test_pointnet2_fused.py ties to the float64 library chain at 1e-12); r32 is the float32 library chain on the host."""
    fixture = golden("pointnet2_ssg")
    enc, pts = cases.fixture_encoder(fixture, "cpu", feat_dim=256)
    with torch.no_grad():
        lv32, lv64, lvd = [], [], []
        r32 = {"out": enc(pts, record=lv32)}
        dbl = copy.deepcopy(enc).double().set_eval_mlp("fused")
        r64 = {"out": dbl(pts.double(), record=lv64)}
        got = {"out": enc.to(cuda_device).set_eval_mlp("fused")(pts.to(cuda_device), record=lvd)}
    for i in range(3):
        r32[f"features.{i}"], r64[f"features.{i}"], got[f"features.{i}"] = lv32[i][1], lv64[i][1], lvd[i][1]
        if lv32[i][0] is not None:
            assert torch.equal(lvd[i][0].cpu(), lv32[i][0])          # the centres are copies
    assert got["out"].shape == (3, 256) and got["features.0"].shape == (3, 128, 512)
    anchored.assert_anchored(got, r32, r64, "PointNet2SSG(256) fused eval", capsys)


def test_forward_parts_in_fused_eval(cuda_device):
    torch.manual_seed(0)
    enc = PointNet2SSG(64).to(cuda_device).eval().set_eval_mlp("fused")
    pcs = torch.rand(5, 600, 3, device=cuda_device) - 0.5
    valids = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0], device=cuda_device)
    dirty = pcs.clone()
    dirty[valids == 0] = float("nan")
    with torch.no_grad():
        out = enc.forward_parts(dirty, valids)
        compact = enc(pcs[valids != 0])
        none = enc.forward_parts(dirty, torch.zeros(5, device=cuda_device))
    assert out.shape == (5, 64) and torch.isfinite(out).all()
    assert float(out[1].abs().max()) == 0.0 and float(out[3].abs().max()) == 0.0 and float(out[0].abs().max()) > 0.0
    assert torch.equal(out[valids != 0], compact)
    assert torch.equal(none, torch.zeros(5, 64, device=cuda_device))
    assert enc.host_sync_per_forward is True


def test_no_stale_weights_after_a_training_step(cuda_device):
    """The trainer's fused Adam writes the parameters through the flat buffer's raw pointer: nothing may be cached."""
    cfg = config.pn_transformer_everyday()
    cfg.model.encoder = "pointnet2_ssg"
    cfg.model.pointnet2_eval = "fused"
    cfg.data.max_num_part = 3
    torch.manual_seed(1)
    model = build_model(cfg).to(cuda_device)
    trainer = Trainer(model, cfg)
    batch = synthetic.make_batch(2, max_parts=3, num_points=600, seed=11, device=cuda_device, num_parts=[2, 3])
    batch.pop("num_parts", None)
    pcs = batch["part_pcs"].flatten(0, 1)[:5].contiguous()

    def fused_eval(enc):
        enc.eval()
        with torch.no_grad():
            out = enc(pcs)
        enc.train()
        return out

    first = fused_eval(model.encoder)
    trainer.train_step(batch)
    torch.cuda.synchronize()
    second = fused_eval(model.encoder)
    torch.manual_seed(2)
    fresh = build_model(cfg).to(cuda_device)
    fresh.load_state_dict(model.state_dict())
    assert fresh.encoder.eval_mlp == "fused"
    assert torch.equal(second, fused_eval(fresh.encoder))
    assert not torch.equal(first, second)


def test_nothing_of_the_grouped_size_is_allocated(cuda_device):
    M, N = 8, 1000
    torch.manual_seed(0)
    enc = PointNet2SSG(128).to(cuda_device).eval().set_eval_mlp("fused")
    pts = torch.rand(M, N, 3, device=cuda_device) - 0.5
    with torch.no_grad():
        enc(pts)                                              # library handles, the kernels' code objects
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(cuda_device)
        base = torch.cuda.memory_allocated(cuda_device)
        out = enc(pts)
        torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(cuda_device) - base
    print(f"fused eval, M = {M}, N = {N}: peak rise {rise / 2 ** 20:.2f} MiB")
    assert out.shape == (M, 128)
    assert rise < M * 64 * 512 * 64 * 4                      # the smallest activation the library chain makes at SA1
    assert rise < 5 * 10 ** 6                                 # indices, centres, level outputs, packed weights


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _eval_model(preset, device, mode):
    cfg = getattr(config, preset)()
    cfg.model.encoder = "pointnet2_ssg"
    cfg.model.pointnet2_eval = mode
    cfg.data.max_num_part = 4
    if "transformer_layers" in cfg.model:
        cfg.model.transformer_layers = 2
    torch.manual_seed(3)
    model = build_model(cfg).to(device)
    with torch.no_grad():                                     # running statistics of a forward, not the initial (0, 1)
        model.train()
        for m in model.modules():
            if isinstance(m, PointNet2SSG):
                m(torch.rand(4, 300, 3, device=device) - 0.5)
    return model


@pytest.mark.parametrize("preset", ["pn_transformer_everyday", "global_everyday"])
def test_evaluator_with_the_knob_on(cuda_device, preset, capsys):
    batches = [synthetic.make_batch(3, max_parts=4, num_points=300, seed=30 + i, device=cuda_device) for i in range(2)]
    model = _eval_model(preset, cuda_device, "fused")
    state = {k: v.clone() for k, v in model.state_dict().items()}
    assert model.training
    res = Evaluator(model).run(batches)
    again = Evaluator(model).run(batches)
    assert model.training and all(m.training for m in model.modules())
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[k]), k
    lib = Evaluator(_eval_model(preset, cuda_device, "library")).run(batches)
    assert list(res) == list(lib) and all(np.isfinite(v) for v in res.values())
    assert res == again
    with capsys.disabled():
        worst = max(res, key=lambda k: abs(res[k] - lib[k]))
        print(f"\n  {preset}: fused vs library evaluation table, largest difference {abs(res[worst] - lib[worst]):.3e} "
              f"({worst}: {res[worst]:.6f} vs {lib[worst]:.6f})", end="")


def test_evaluate_tool_runs_to_a_table(cuda_device, tmp_path, capsys, monkeypatch):
    tool = load_tool("evaluate")
    shapes = synthetic.make_fracture_meshes(7, 4, [2, 3, 2, 3], 40)
    folders = []
    for s, parts in enumerate(shapes):
        rel = os.path.join("everyday", "Bottle" if s < 2 else "Cup", f"shape{s}", "fractured_0")
        os.makedirs(tmp_path / "data" / rel)
        for k, (v, f) in enumerate(parts):
            assemble.write_obj(tmp_path / "data" / rel / f"piece_{k}.obj", v[f])
        folders.append(os.path.dirname(rel))
    (tmp_path / "data" / "val.txt").write_text("\n".join(folders) + "\n")
    cfg = config.pn_transformer_everyday()
    cfg.model.encoder = "pointnet2_ssg"
    cfg.model.pc_feat_dim, cfg.model.transformer_feat_dim = 64, 128
    cfg.model.transformer_heads, cfg.model.transformer_layers = 4, 2
    cfg.data.num_pc_points = 200
    torch.manual_seed(5)
    torch.save(build_model(cfg).state_dict(), tmp_path / "weights.pt")
    cfg.model.encoder = "pointnet"                            # the flags, not the preset, select the encoder and its path
    monkeypatch.setattr(config, "fused_eval_test_preset", lambda: cfg.clone(), raising=False)
    monkeypatch.setattr(config, "EVERYDAY_CATEGORIES", ["Bottle", "Cup"])
    seen = []
    real = fused.sa_level_eval
    monkeypatch.setattr(fused, "sa_level_eval", lambda *a: seen.append(1) or real(*a))
    tool.main(["--preset", "fused_eval_test_preset", "--weight", str(tmp_path / "weights.pt"), "--data-dir",
               str(tmp_path / "data"), "--data-fn", "val.txt", "--max-num-part", "4", "--category", "all",
               "--encoder", "pointnet2_ssg", "--pointnet2-eval", "fused"])
    table = capsys.readouterr().out
    assert "categories: Bottle & Cup & mean" in table and "part_acc" in table
    assert len(seen) == 6                                     # three levels, one batch per category


def test_workload_shape_once(cuda_device):
    """M = 352 clouds of 1000 points, the whole encoder, against the library path on the device."""
    torch.manual_seed(0)
    enc = PointNet2SSG(128).to(cuda_device)
    pts = torch.rand(352, 1000, 3, device=cuda_device) - 0.5
    with torch.no_grad():
        enc.train()
        enc(pts[:8])
        enc.eval()
        lib = enc(pts)
        got = enc.set_eval_mlp("fused")(pts)
    e = float((got - lib).abs().max()) / float(lib.abs().max())
    print(f"M = 352: max |fused - library| / max |library| = {e:.2e}")
    assert got.shape == (352, 128) and e <= anchored.CEIL
