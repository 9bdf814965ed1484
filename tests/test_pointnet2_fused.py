"""The fused evaluation path of the PointNet++ encoder without a GPU: the numpy restatement `pointnet2_ref.sa_mlp_max`
against the float64 library chain, the pack definition, the encoder's fused evaluation on host tensors against the
float64 records of tests/golden/pointnet2_ssg.npz, the routing of `PointNet2SSG.eval_mlp`, the configuration key and the
tools' flag, and the argument contract of the three entry points of csrc/pointnet2_sa_mlp.hip."""
import copy
import ctypes
import warnings

import numpy as np
import pytest
import torch

import anchored
import sa_mlp_cases as cases
from multi_part_assembly_amd import _build, _lib, config
from multi_part_assembly_amd import pointnet2_fused as fused
from multi_part_assembly_amd import pointnet2_ref as ref
from multi_part_assembly_amd import pointnet2_utils as pu
from multi_part_assembly_amd.encoder import DGCNN, PointNet
from multi_part_assembly_amd.pn_transformer import build_model
from multi_part_assembly_amd.pointnet2 import PointNet2SSG, PointnetSAModule
from tool_loader import load_tool as _tool

PRESETS = ["pn_transformer_everyday", "pn_transformer_refine_everyday", "global_everyday", "dgl_everyday",
           "rgl_net_everyday", "lstm_everyday"]


@pytest.fixture(scope="module")
def built():
    return _build.build()


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------
def _f64_group(features, idx):
    """`grouping_operation` without its cast to float32: features [M, C, N], idx [M, S, K] -> [M, C, S, K]."""
    M, C, N = features.shape
    ok = (idx >= 0) & (idx < N)
    safe = torch.where(ok, idx, torch.zeros_like(idx)).long()
    out = torch.gather(features[:, :, None, :].expand(M, C, idx.shape[1], N), 3, safe[:, None].expand(M, C, *idx.shape[1:]))
    return torch.where(ok[:, None], out, torch.zeros((), dtype=features.dtype))


def test_restatement_equals_the_float64_library_chain(monkeypatch):
    """QueryAndGroup / GroupAll -> Conv2d, BatchNorm2d.eval(), ReLU, max_pool2d in float64 on the same indices."""
    mlp = cases.make_mlp(4, (8, 8, 16), seed=3)
    xyz, new_xyz, feats, idx = cases.make_inputs(2, 40, 5, 7, 4, seed=4)
    idx[0, 1, 3] = 40                     # outside [0, N): a zero point and zero features
    idx[1, 2, 5] = -1
    idx[1, 4, 2:] = idx[1, 4, 0]          # a ball padded by repetition
    dbl = copy.deepcopy(mlp).double()
    monkeypatch.setattr(pu, "ball_query", lambda radius, nsample, a, b: idx)
    monkeypatch.setattr(pu, "grouping_operation", _f64_group)
    g = pu.QueryAndGroup(0.2, 7)(xyz.double(), new_xyz.double(), feats.double().transpose(1, 2).contiguous())
    assert torch.equal(g, cases.grouped(xyz.double(), new_xyz.double(), feats.double(), idx))
    want = cases.library_chain(dbl, g)
    got = ref.sa_mlp_max(xyz.double().numpy(), new_xyz.double().numpy(), feats.double().numpy(), idx.numpy(),
                         cases.host_layers(mlp, np.float64))
    assert got.dtype == np.float64 and got.shape == (2, 5, 16)
    assert float(np.abs(got - want.numpy()).max()) <= 1e-12 * float(want.abs().max())
    # one group of every point
    xyz, _, feats, _ = cases.make_inputs(2, 9, 1, 9, 4, seed=5, group_all=True)
    g = pu.GroupAll()(xyz.double(), None, feats.double().transpose(1, 2).contiguous())
    want = cases.library_chain(dbl, g)
    got = ref.sa_mlp_max(xyz.double().numpy(), None, feats.double().numpy(), None, cases.host_layers(mlp, np.float64))
    assert got.shape == (2, 1, 16)
    assert float(np.abs(got - want.numpy()).max()) <= 1e-12 * float(want.abs().max())
    # the dtype of the inputs is the dtype of the evaluation
    got32 = ref.sa_mlp_max(xyz.numpy(), None, feats.numpy(), None, cases.host_layers(mlp, np.float32))
    assert got32.dtype == np.float32 and float(np.abs(got32 - got).max()) <= 1e-5 * float(np.abs(got).max())
    with pytest.raises(ValueError):
        ref.sa_mlp_max(xyz.numpy(), None, None, idx.numpy(), cases.host_layers(mlp, np.float32))


def test_pack_definition():
    mlp = cases.make_mlp(4, (8, 8, 16), seed=6)
    for (conv, bn), (W, scale, shift) in zip(cases.pairs(mlp), cases.host_layers(mlp, np.float32)):
        gamma, beta, mean, var = (t.detach().numpy() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
        want = gamma / np.sqrt(var + np.float32(bn.eps))
        assert scale.dtype == np.float32 and np.array_equal(scale, want)
        assert np.array_equal(shift, beta - mean * want)
        assert np.array_equal(W, conv.weight.detach().numpy().reshape(W.shape))
    s64, t64 = ref.sa_scale_shift(gamma.astype(np.float64), beta, mean, var, bn.eps)
    assert s64.dtype == t64.dtype == np.float64


# ---- 2. the encoder on host tensors ----------------------------------------------------------------------------------------
def test_fused_eval_on_host_tensors_against_the_float64_records(golden):
    fixture = golden("pointnet2_ssg")
    enc, pts = cases.fixture_encoder(fixture)
    assert enc.set_eval_mlp("fused") is enc
    with torch.no_grad():
        out = enc(pts)
    assert out.shape == (3, 128) and out.dtype == torch.float32
    r32, r64 = cases.records(fixture, "f32."), cases.records(fixture, "f64.")
    anchored.assert_anchored({"out.eval": cases.picked(out)}, r32, r64, "pointnet2_ssg fused eval (host restatement)")


def test_default_is_the_library_path_and_training_is_untouched():
    assert PointNet2SSG.eval_mlp == "library" and PointNet2SSG(64).eval_mlp == "library"
    with pytest.raises(ValueError, match="eval_mlp"):
        PointNet2SSG(64).set_eval_mlp("hip")
    torch.manual_seed(0)
    enc = PointNet2SSG(64).train()
    twin = copy.deepcopy(enc)
    enc.set_eval_mlp("fused")
    assert twin.eval_mlp == "library" and enc.host_sync_per_forward is True
    pts = torch.rand(2, 80, 3, generator=torch.Generator().manual_seed(1)) - 0.5
    a, b = enc(pts), twin(pts)
    a.sum().backward()
    b.sum().backward()
    assert torch.equal(a, b)
    for (k, x), (_, y) in zip(enc.state_dict().items(), twin.state_dict().items()):
        assert torch.equal(x, y), k
    for (k, p), (_, q) in zip(enc.named_parameters(), twin.named_parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), k
    assert list(enc.state_dict()) == list(twin.state_dict())


def test_grad_enabled_eval_takes_the_library_path(monkeypatch):
    torch.manual_seed(0)
    enc = PointNet2SSG(64).eval().set_eval_mlp("fused")
    pts = torch.rand(2, 80, 3, generator=torch.Generator().manual_seed(1)) - 0.5
    taken = []
    real = fused.sa_level_eval
    monkeypatch.setattr(fused, "sa_level_eval", lambda *a: taken.append(1) or real(*a))
    out = enc(pts)                                            # gradients enabled: today's path
    assert not taken and out.requires_grad
    lib = out.detach()
    with torch.no_grad():
        levels = []
        got = enc(pts, record=levels)
    assert len(taken) == 3 and not got.requires_grad
    assert [tuple(f.shape) for _, f in levels] == [(2, 128, 512), (2, 256, 128), (2, 64, 1)]
    assert levels[2][0] is None and tuple(levels[0][0].shape) == (2, 512, 3)
    assert float((got - lib).abs().max()) <= 1e-5 * float(lib.abs().max())
    enc.train()
    with torch.no_grad():
        enc(pts)
    assert len(taken) == 3                                    # training mode: the library chain, gradients or not


@pytest.mark.parametrize("kind", ["bn_false", "two_layers"])
def test_a_level_outside_the_envelope_falls_back_with_one_warning(kind):
    torch.manual_seed(0)
    enc = PointNet2SSG(64)
    if kind == "bn_false":
        enc.SA_modules[0] = PointnetSAModule(npoint=512, radius=0.2, nsample=64, mlp=[0, 64, 64, 128], bn=False)
    else:
        enc.SA_modules[0] = PointnetSAModule(npoint=512, radius=0.2, nsample=64, mlp=[0, 64, 128])
    assert fused.envelope_miss(enc.SA_modules[0]) is not None and fused.envelope_miss(enc.SA_modules[1]) is None
    enc.eval()
    pts = torch.rand(2, 80, 3, generator=torch.Generator().manual_seed(1)) - 0.5
    with torch.no_grad():
        lib = enc(pts)
        enc.set_eval_mlp("fused")
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            got = enc(pts)
            enc(pts)
    assert len(seen) == 1 and "library operators" in str(seen[0].message)
    assert float((got - lib).abs().max()) <= 1e-5 * float(lib.abs().max())


# ---- 3. the configuration key and the tools ---------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", PRESETS)
def test_config_key_reaches_every_encoder(preset):
    cfg = getattr(config, preset)()
    assert "pointnet2_eval" not in cfg.model
    cfg.model.encoder = "pointnet2_ssg"
    plain = build_model(cfg)
    assert plain.pointnet2_eval == "library" and plain.encoder.eval_mlp == "library"
    cfg.model.pointnet2_eval = "fused"
    model = build_model(cfg)
    encoders = [m for m in model.modules() if isinstance(m, PointNet2SSG)]
    assert encoders and all(e.eval_mlp == "fused" for e in encoders) and model.encoder in encoders
    if preset == "global_everyday":
        assert len(encoders) == 2 and model.global_encoder.eval_mlp == "fused"
    assert list(model.state_dict()) == list(plain.state_dict())
    cfg.model.pointnet2_eval = "hip"
    with pytest.raises(ValueError, match="pointnet2_eval"):
        build_model(cfg)


@pytest.mark.parametrize("arch,cls", [("pointnet", PointNet), ("dgcnn", DGCNN)])
def test_other_encoders_ignore_the_key(arch, cls):
    cfg = config.pn_transformer_everyday()
    cfg.model.encoder = arch
    cfg.model.pointnet2_eval = "fused"
    model = build_model(cfg)
    assert isinstance(model.encoder, cls) and not hasattr(model.encoder, "eval_mlp")


def test_tools_take_the_flag():
    train = _tool("train")
    assert train.parse_args(["--preset", "pn_transformer_everyday", "--synthetic", "--pointnet2-eval", "fused"]).pointnet2_eval == "fused"
    assert train.parse_args(["--preset", "pn_transformer_everyday", "--synthetic"]).pointnet2_eval is None
    common = ["--preset", "pn_transformer_everyday", "--data-dir", "d", "--data-fn", "f"]
    ev = _tool("evaluate")
    args = ev.parse_args(common + ["--encoder", "pointnet2_ssg", "--pointnet2-eval", "fused"])
    assert args.pointnet2_eval == "fused" and args.encoder == "pointnet2_ssg"
    assert ev.parse_args(common).pointnet2_eval is None
    vis = _tool("visualize")
    args = vis.parse_args(common + ["--out", "o", "--encoder", "pointnet2_ssg", "--pointnet2-eval", "fused"])
    assert args.pointnet2_eval == "fused" and args.encoder == "pointnet2_ssg"
    assert vis.parse_args(common + ["--out", "o"]).pointnet2_eval is None
    with pytest.raises(SystemExit):
        ev.parse_args(common + ["--pointnet2-eval", "hip"])


# ---- 4. the entry points without a GPU --------------------------------------------------------------------------------------
def test_abi_declares_the_entry_points():
    declared = _lib.declared_functions()
    for name, nargs in (("mpa_sa_mlp_packed_bytes", 3), ("mpa_sa_mlp_pack", 10), ("mpa_sa_mlp_max_forward", 17)):
        assert name in declared and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.ABI_VERSION == 10


def test_packed_bytes_is_the_documented_formula(built):
    for cout, cin in ((32, 1), (64, 3), (128, 131), (256, 259), (512, 512), (96, 32), (96, 33), (0, 5)):
        cinp = -(-cin // 32) * 32
        assert fused.packed_bytes(cout, cin) == 6 * cout * cinp + 8 * cout, (cout, cin)
    L = _lib.lib()
    out = ctypes.c_int64()
    assert L.mpa_sa_mlp_packed_bytes(-1, 3, ctypes.byref(out)) == -1 and b"negative" in L.mpa_last_error()
    assert L.mpa_sa_mlp_packed_bytes(32, 3, None) == -1 and b"null" in L.mpa_last_error()


def test_entry_points_validate_without_a_gpu(built):
    L = _lib.lib()
    one = ctypes.c_void_p(256)  # a non-null, aligned pointer that validation never dereferences

    def fwd(M=2, N=40, S=5, K=7, C=4, C1=32, C2=32, C3=32, xyz=one, new_xyz=one, feat=one, idx=one, layers=(one, one, one),
            out=one):
        return L.mpa_sa_mlp_max_forward(xyz, new_xyz, feat, idx, M, N, S, K, C, *layers, C1, C2, C3, out, None)

    for name in ("M", "N", "S", "K", "C", "C1", "C2", "C3"):
        assert fwd(**{name: -1}) == -1 and b"negative" in L.mpa_last_error(), name
    assert fwd(M=0) == 0 and fwd(S=0) == 0 and fwd(C3=0) == 0          # empty problems
    assert fwd(M=0, xyz=None, out=None) == 0
    assert fwd(C1=48) == -1 and b"C1=48" in L.mpa_last_error()
    assert fwd(C2=16) == -1 and b"C2=16" in L.mpa_last_error()
    assert fwd(C3=544) == -1 and b"C3=544" in L.mpa_last_error()
    assert fwd(C=513) == -1 and b"C=513" in L.mpa_last_error()
    assert fwd(K=0) == -1 and b"K=0" in L.mpa_last_error()
    assert fwd(N=0) == -1 and b"N=0" in L.mpa_last_error()
    assert fwd(M=1 << 20, N=1 << 10) == -1 and b"2^31" in L.mpa_last_error()       # 3 M N
    assert fwd(M=1 << 12, S=1 << 12, K=128) == -1 and b"2^31" in L.mpa_last_error()  # M S K
    assert fwd(M=1 << 11, N=1 << 11, C=512) == -1 and b"2^31" in L.mpa_last_error()  # M N C
    for name in ("xyz", "out", "feat"):
        assert fwd(**{name: None}) == -1 and b"null" in L.mpa_last_error(), name
    assert fwd(C=0) == -1 and b"null" in L.mpa_last_error()              # features without channels
    assert fwd(layers=(one, None, one)) == -1 and b"null" in L.mpa_last_error()
    assert fwd(idx=None) == -1 and b"together" in L.mpa_last_error()     # idx and new_xyz come as a pair
    assert fwd(idx=None, new_xyz=None, S=2) == -1 and b"S=1" in L.mpa_last_error()
    assert fwd(layers=(one, ctypes.c_void_p(264), one)) == -1 and b"aligned" in L.mpa_last_error()

    def pack(cout=32, cin=7, w=one, gamma=one, packed=one):
        return L.mpa_sa_mlp_pack(w, gamma, one, one, one, 1e-5, cout, cin, packed, None)

    assert pack(cout=-32) == -1 and b"negative" in L.mpa_last_error()
    assert pack(cout=0) == 0
    assert pack(cout=48) == -1 and b"Cout=48" in L.mpa_last_error()
    assert pack(cout=544) == -1 and b"Cout=544" in L.mpa_last_error()
    assert pack(cin=0) == -1 and b"Cin=0" in L.mpa_last_error()
    assert pack(cin=516) == -1 and b"Cin=516" in L.mpa_last_error()
    assert pack(w=None) == -1 and b"null" in L.mpa_last_error()
    assert pack(gamma=None) == -1 and pack(packed=None) == -1
