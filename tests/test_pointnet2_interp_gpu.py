"""csrc/pointnet2_interp.hip against the numpy restatement (multi_part_assembly_amd/pointnet2_ref.py), index for index and bit
for bit: three_nn across the block edge (256 unknown points), the LDS tile edge (512 known points) and the tails of its
four-point trips, on clouds full of ties; three_interpolate forward and backward across the channel tile, the staged and
unstaged feature rows (8192 floats), the chunk of 1024 unknown points, with empty and very long contribution lists and
indices out of range; sentinels, run-to-run identity, graph capture, the workload shape once; the autograd wrappers;
`PointnetFPModule` against the float64 record of the reference's module (tests/golden/pointnet2_fp_msg.npz, bars of
tests/anchored.py); `PointNet2MSG` fed by the HIP operators against the same module fed by the host restatement, and one
training step of a model that carries it."""
import numpy as np
import pytest
import torch

import anchored
from multi_part_assembly_amd import _lib, config, pointnet2_ref as ref, pointnet2_utils as pu, synthetic
from multi_part_assembly_amd.pn_transformer import build_model
from multi_part_assembly_amd.pointnet2 import PointNet2MSG
from multi_part_assembly_amd.trainer import Trainer
from test_pointnet2_interp import KINDS, cloud_pair, fp_module, fp_pass, fp_tensors, interp_case, msg_encoder

pytestmark = pytest.mark.gpu
f32 = np.float32
TILE = 512            # known points per LDS tile of three_nn_kernel


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def padded(n, dtype, device, fill):
    """A buffer of n elements with 64 guard elements behind it, all `fill`."""
    buf = torch.full((n + 64,), fill, dtype=dtype, device=device)
    return buf, buf[:n]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def three_nn_raw(unknown, known, device):
    """The entry point itself on sentinel-filled, guarded outputs -> (dist, idx) numpy."""
    M, n, _ = unknown.shape
    m = known.shape[1]
    dbuf, dview = padded(3 * M * n, torch.float32, device, -7.0)
    ibuf, iview = padded(3 * M * n, torch.int32, device, -12345)
    _lib.launch("mpa_three_nn", device, dev(unknown, device), dev(known, device), M, n, m, dview, iview)
    assert (dbuf[3 * M * n:] == -7.0).all() and (ibuf[3 * M * n:] == -12345).all()
    return dview.cpu().numpy().reshape(M, n, 3), iview.cpu().numpy().reshape(M, n, 3)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257])
def test_three_nn_equals_the_restatement(cuda_device, n):
    for mi, m in enumerate((1, 2, 3, 4, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)):
        for s, kind in enumerate(KINDS):
            M = (1, 3)[(mi + s) % 2]
            unknown, known = cloud_pair(kind, M, n, m, 100 * n + 10 * mi + s)
            dist, idx = three_nn_raw(unknown, known, cuda_device)
            want_dist, want_idx = ref.three_nn(unknown, known)
            assert np.array_equal(idx, want_idx), (kind, M, n, m)
            assert np.array_equal(bits(dist), bits(want_dist)), (kind, M, n, m)
            if m < 3:
                assert np.isinf(dist[..., m:]).all() and not idx[..., m:].any()
            if kind == "same":
                assert not dist[..., 0].any()


def test_three_nn_with_nan_coordinates_returns_indices_in_range(cuda_device):
    unknown, known = cloud_pair("random", 2, 300, 70, 7)
    known[0, 5], known[1, 17, 1], unknown[0, 3], unknown[1, 40, 2] = np.nan, np.inf, np.nan, -np.inf
    dist, idx = three_nn_raw(unknown, known, cuda_device)
    assert idx.min() >= 0 and idx.max() < 70
    want_dist, want_idx = ref.three_nn(unknown, known)
    assert np.array_equal(idx, want_idx) and np.array_equal(bits(dist), bits(want_dist))
    assert not (idx[0] == 5).any() and not idx[0, 3].any() and np.isinf(dist[0, 3]).all()


def interpolate_raw(feat, idx, w, g, device):
    """Both entry points on NaN-filled, guarded outputs -> (out, grad_features) numpy."""
    M, C, m = feat.shape
    n = idx.shape[1]
    fbuf, fview = padded(M * C * m, torch.float32, device, float("nan"))      # NaN behind the features: never read
    fview.copy_(dev(feat, device).reshape(-1))
    didx, dw = dev(idx, device), dev(w, device)
    obuf, oview = padded(M * C * n, torch.float32, device, float("nan"))
    _lib.launch("mpa_three_interpolate_forward", device, fview, didx, dw, M, C, m, n, oview)
    assert torch.isnan(obuf[M * C * n:]).all()
    ws = torch.empty(max(1, _lib.query("mpa_three_interpolate_workspace", M, n, m)), dtype=torch.uint8, device=device)
    gbuf, gview = padded(M * C * m, torch.float32, device, float("nan"))
    _lib.launch("mpa_three_interpolate_backward", device, dev(g, device), didx, dw, M, C, n, m, ws, gview)
    assert torch.isnan(gbuf[M * C * m:]).all()
    return oview.cpu().numpy().reshape(M, C, n), gview.cpu().numpy().reshape(M, C, m)


# (n, m): the sizes of the operator tests; 1025 unknown points: two chunks of both kernels; 3000 known points: two staged
# feature rows per block instead of eight; 8193: rows read from global memory
INTERP_SHAPES = [(1, 1), (2, 3), (63, 2), (64, 65), (65, 64), (255, 4), (256, 63), (257, 513), (1025, 5), (2100, 64),
                 (33, 3000), (40, 8193)]


@pytest.mark.parametrize("C", [1, 3, 64, 65, 259])
def test_three_interpolate_forward_and_backward_are_bit_equal(cuda_device, C):
    for s, (n, m) in enumerate(INTERP_SHAPES):
        M = (1, 3)[s % 2]
        feat, idx, w, g = interp_case(M, C, m, n, 10 * C + s, out_of_range=s % 3 == 2)
        out, grad = interpolate_raw(feat, idx, w, g, cuda_device)
        assert np.array_equal(bits(out), bits(ref.three_interpolate(feat, idx, w))), (C, n, m)
        assert np.array_equal(bits(grad), bits(ref.three_interpolate_backward(g, idx, w, m))), (C, n, m)
        if m > 2:
            assert not (idx == m - 1).any() and not bits(grad[:, :, m - 1]).any()     # no referrer: exactly +0
        if M > 1 and s % 3 != 2:
            assert (idx[1] == idx[1, 0, 0]).all()                                      # a list of 3 n entries


def test_out_of_range_indices_are_neither_read_nor_written_through(cuda_device):
    M, C, m, n = 2, 5, 40, 90
    feat, idx, w, g = interp_case(M, C, m, n, 3, out_of_range=True)
    idx[0, 0], idx[1, 1] = (-1, m, 2 ** 31 - 1), (-2 ** 31, m + 100000, 0)
    out, grad = interpolate_raw(feat, idx, w, g, cuda_device)
    assert np.array_equal(bits(out), bits(ref.three_interpolate(feat, idx, w))) and not out[0, :, 0].any()
    assert np.array_equal(bits(grad), bits(ref.three_interpolate_backward(g, idx, w, m)))
    none = np.full_like(idx, m)                                                        # nothing in range at all
    out, grad = interpolate_raw(feat, none, w, g, cuda_device)
    assert not bits(out).any() and not bits(grad).any()


def test_two_runs_are_identical_and_a_captured_call_equals_the_eager_call(cuda_device):
    n, m, C = 600, 70, 37
    res = {}
    u1, k1 = cloud_pair("random", 2, n, m, 1)
    u2, k2 = cloud_pair("duplicated", 2, n, m, 2)
    feat, _, _, g = interp_case(2, C, m, n, 5)
    static_u, static_k = dev(u1, cuda_device), dev(k1, cuda_device)
    dfeat, dg = dev(feat, cuda_device), dev(g, cuda_device)

    def call():
        res["dist"], res["idx"] = pu.three_nn(static_u, static_k)
        recip = 1.0 / (res["dist"] + 1e-8)
        res["weight"] = recip / recip.sum(dim=2, keepdim=True)
        res["out"] = pu._interpolate_forward(dfeat, res["idx"], res["weight"])
        res["grad"] = pu._interpolate_backward(dg, res["idx"], res["weight"], m)

    side = torch.cuda.Stream(device=cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream(cuda_device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    static_u.copy_(dev(u2, cuda_device))
    static_k.copy_(dev(k2, cuda_device))
    held = dict(res)
    for v in held.values():
        v.fill_(-3)
    graph.replay()
    torch.cuda.synchronize()
    replayed = {k: v.clone() for k, v in held.items()}
    runs = []
    for _ in range(2):
        call()
        runs.append({k: v.clone() for k, v in res.items()})
    for k in replayed:
        assert torch.equal(runs[0][k], runs[1][k]), k
        assert torch.equal(replayed[k].view(torch.int32), runs[0][k].view(torch.int32)), k
    want_dist, want_idx = ref.three_nn(u2, k2)
    assert np.array_equal(replayed["idx"].cpu().numpy(), want_idx)
    assert np.array_equal(bits(replayed["dist"].cpu().numpy()), bits(want_dist))
    wt = replayed["weight"].cpu().numpy()
    assert np.array_equal(bits(replayed["out"].cpu().numpy()), bits(ref.three_interpolate(feat, want_idx, wt)))
    assert np.array_equal(bits(replayed["grad"].cpu().numpy()), bits(ref.three_interpolate_backward(g, want_idx, wt, m)))


def test_workload_shape_once(cuda_device):
    """M = 352 clouds, n = 1000 unknown and m = 128 known points, C = 256: the neighbours of 12 clouds in full; the
    interpolation and its backward sums on eight (cloud, channel) rows (the kernels compute all of them)."""
    M, n, m, C = 352, 1000, 128, 256
    gen = torch.Generator(device=cuda_device).manual_seed(0)
    unknown = torch.rand(M, n, 3, device=cuda_device, generator=gen) - 0.5
    known = unknown[:, ::7][:, :m].contiguous()                                # a subset: these points are their own neighbours
    dist, idx = pu.three_nn(unknown, known)
    assert dist.shape == idx.shape == (M, n, 3) and idx.dtype == torch.int32
    clouds = [0, 1, 2, 3, 100, 101, 175, 176, 300, 349, 350, 351]
    want_dist, want_idx = ref.three_nn(unknown[clouds].cpu().numpy(), known[clouds].cpu().numpy())
    assert np.array_equal(idx[clouds].cpu().numpy(), want_idx)
    assert np.array_equal(bits(dist[clouds].cpu().numpy()), bits(want_dist))
    assert int(idx.min()) >= 0 and int(idx.max()) < m and not dist[:, ::7][:, :m, 0].any()
    recip = 1.0 / (dist + 1e-8)
    weight = recip / recip.sum(dim=2, keepdim=True)
    feat = torch.randn(M, C, m, device=cuda_device, generator=gen).requires_grad_()
    out = pu.three_interpolate(feat, idx, weight)
    assert out.shape == (M, C, n)
    g = torch.randn(M, C, n, device=cuda_device, generator=gen)
    out.backward(g)
    for b, c in [(0, 0), (0, 255), (5, 3), (100, 64), (200, 1), (351, 0), (351, 255), (17, 99)]:
        ib, wb = idx[b:b + 1].cpu().numpy(), weight[b:b + 1].cpu().numpy()
        f_row, g_row = feat[b, c].detach().cpu().numpy()[None, None], g[b, c].cpu().numpy()[None, None]
        assert np.array_equal(bits(out[b, c].detach().cpu().numpy()), bits(ref.three_interpolate(f_row, ib, wb)[0, 0])), (b, c)
        assert np.array_equal(bits(feat.grad[b, c].cpu().numpy()), bits(ref.three_interpolate_backward(g_row, ib, wb, m)[0, 0])), (b, c)


def test_autograd_wrappers(cuda_device):
    feat, idx, w, g = interp_case(3, 7, 12, 40, 6)
    unknown, known = cloud_pair("random", 3, 40, 12, 6)
    dist, nn_idx = pu.three_nn(dev(unknown, cuda_device).requires_grad_(), dev(known, cuda_device).requires_grad_())
    assert not dist.requires_grad and not nn_idx.requires_grad and dist.grad_fn is None
    assert dist.dtype == torch.float32 and nn_idx.dtype == torch.int32 and dist.is_cuda
    tf, tw = dev(feat, cuda_device).requires_grad_(), dev(w, cuda_device).requires_grad_()
    out = pu.three_interpolate(tf, dev(idx, cuda_device), tw)
    (grad,) = torch.autograd.grad(out, tf, dev(g, cuda_device))
    assert np.array_equal(bits(out.detach().cpu().numpy()), bits(ref.three_interpolate(feat, idx, w)))
    assert np.array_equal(bits(grad.cpu().numpy()), bits(ref.three_interpolate_backward(g, idx, w, 12)))
    out = pu.three_interpolate(tf, dev(idx, cuda_device), tw)
    out.backward(dev(g, cuda_device))
    assert tw.grad is None and torch.equal(tf.grad, grad)
    half = pu.three_interpolate(tf.double(), dev(idx, cuda_device).long(), tw)     # cast to float32 / int32, as upstream
    assert half.dtype == torch.float32 and torch.equal(half, out)


def fp_records(fixture, prefix):
    return {k[len(prefix):]: torch.from_numpy(v) for k, v in fixture.items() if k.startswith(prefix)}


def test_fp_module_against_the_float64_record_of_the_reference_module(cuda_device, golden, capsys):
    fixture = golden("pointnet2_fp_msg")
    r32, r64 = fp_records(fixture, "fp.f32."), fp_records(fixture, "fp.f64.")
    fp = fp_module(fixture).to(cuda_device)
    got, idx = fp_pass(fp, fp_tensors(fixture, cuda_device))
    assert set(got) == set(r64) == set(r32)
    assert np.array_equal(idx.cpu().numpy(), fixture["fp.idx"])
    assert torch.equal(got["out.dist"].cpu(), r32["out.dist"])                 # the operator's own bits
    rows = anchored.assert_anchored(got, r32, r64, "pointnet2_fp", capsys)
    assert len(rows) == len(got)                                               # every tensor under a relative bar
    with capsys.disabled():
        for e, e32, bar, k in sorted(rows, reverse=True)[:4]:
            print(f"\n    {k}: err {e:.2e}  e32 {e32:.2e}  bar {bar:.2e}", end="")


def on_host(fn):
    """`fn` of pointnet2_utils run on host copies of its tensor arguments (the numpy restatement), result back on the device."""
    def call(*args):
        device = next(a.device for a in args if torch.is_tensor(a))
        out = fn(*[a.cpu() if torch.is_tensor(a) else a for a in args])
        return tuple(o.to(device) for o in out) if isinstance(out, tuple) else out.to(device)
    return call


def test_fp_module_on_hip_operators_equals_the_module_on_the_restatement(cuda_device, golden, monkeypatch):
    fixture = golden("pointnet2_fp_msg")
    x = fp_tensors(fixture, cuda_device)
    hip, _ = fp_pass(fp_module(fixture).to(cuda_device), x)
    for name in ("three_nn", "_interpolate_forward", "_interpolate_backward"):
        monkeypatch.setattr(pu, name, on_host(getattr(pu, name)))
    host, _ = fp_pass(fp_module(fixture).to(cuda_device), x)
    monkeypatch.undo()
    for k in hip:                                   # equal operator bits in, the same library kernels behind
        if k.startswith(("out.", "stat.")):
            assert torch.equal(hip[k], host[k]), k
        else:                                       # (the library's backward kernels need not be run-to-run identical)
            assert float((hip[k] - host[k]).abs().max()) <= anchored.CEIL * float(host[k].abs().max()), k


def run_msg(fixture, device):
    """The training-mode forward of the fixture's encoder on its points: every level's record and the running statistics."""
    enc = msg_encoder(fixture).to(device)
    levels = []
    with torch.no_grad():
        out = enc(torch.from_numpy(fixture["msg.points"]).to(device), record=levels)
    got = {"out.train": out}
    for i, (new_xyz, feats) in enumerate(levels):
        if new_xyz is not None:
            got[f"new_xyz.{i}"] = new_xyz
        got[f"features.{i}"] = feats
    got.update({f"stat.{k}": v for k, v in enc.state_dict().items() if "running_" in k})
    return {k: v.detach().clone() for k, v in got.items()}


def test_msg_encoder_on_hip_operators_equals_the_encoder_on_the_restatement(cuda_device, golden, monkeypatch):
    """Both runs use the same library kernels for the shared MLPs on equal inputs: centres, features of every level and
    running statistics are bit-equal (the check of tests/test_pointnet2_encoder_gpu.py for the SSG encoder; the backward
    operators are the same calls as there and are not run again)."""
    fixture = golden("pointnet2_fp_msg")
    hip = run_msg(fixture, cuda_device)
    for name in ("furthest_point_sample", "ball_query", "_group_forward"):
        monkeypatch.setattr(pu, name, on_host(getattr(pu, name)))
    host = run_msg(fixture, cuda_device)
    monkeypatch.undo()
    assert set(hip) == set(host) and hip["out.train"].shape == (2, 64) and hip["features.0"].shape == (2, 320, 512)
    assert hip["features.1"].shape == (2, 640, 128) and len(hip) == 6 + 2 * 21
    for k in hip:
        assert torch.equal(hip[k], host[k]), k
    r32 = {k[len("msg.f32."):]: v for k, v in fixture.items() if k.startswith("msg.f32.new_xyz.")}
    for k, v in r32.items():                                   # the centres are copies: the reference record's points, bit for bit
        assert np.array_equal(hip[k].cpu().numpy().reshape(-1), v), k


def test_one_training_step_of_a_model_with_the_msg_encoder(cuda_device):
    cfg = config.pn_transformer_everyday()
    cfg.data.max_num_part = 3
    torch.manual_seed(1)
    model = build_model(cfg)
    model.encoder = PointNet2MSG(model.pc_feat_dim)
    model = model.to(cuda_device)
    trainer = Trainer(model, cfg)
    batch = synthetic.make_batch(2, max_parts=3, num_points=96, seed=11, device=cuda_device, num_parts=[2, 3])
    batch.pop("num_parts", None)
    # The 21 convolutions of the encoder have 21 distinct shapes; MIOpen builds the backward kernels of each on first
    # use, 11 of the 13 seconds this test took with it.  What is under test is the step over the HIP operators, not the
    # library's choice of convolution kernel, so the step runs on torch's own convolutions (0.4 s for a first pass).
    with torch.backends.cudnn.flags(enabled=False):
        loss = trainer._fwd_bwd(batch)
        assert torch.isfinite(loss).item()
        for name, p in model.encoder.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
            assert p.dim() == 1 or float(p.grad.abs().max()) > 0.0, name
        before = trainer.flat.flat_param.clone()
        loss = trainer.train_step(batch)
        torch.cuda.synchronize()
    assert torch.isfinite(loss).item() and not torch.equal(before, trainer.flat.flat_param)
