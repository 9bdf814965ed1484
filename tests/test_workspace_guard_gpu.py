"""Bounds check of every caller-owned workspace of libmpa_hip.so, one test per family of entry points.

A family's wrapper runs once, forward and backward, on plain `torch.empty` workspaces while every library call it makes
is recorded: the entry point, its arguments as they were before the call and its outputs as they were after it.  Each
recorded call is then made again through the C ABI directly, with every workspace, output and in/out buffer replaced by
a slice of a larger allocation: exactly as many elements as the wrapper passed (a workspace: exactly what its
`*_workspace` query returns), with a margin of GUARD elements on either side, margins and interior filled with a bit
pattern that no result contains.  After every call

  * every margin of every buffer handed out so far must still hold the pattern (nothing is written out of bounds), and
  * every output must equal the wrapper's bit for bit (no field of a layout overlaps another, and nothing depends on
    what a workspace or an output held before the call).  Some outputs have elements that no call writes (the rows of
    padded parts in `mpa_assembly_order`'s array): the recorder fills the wrapper's outputs with a second pattern
    before the wrapper's call, and the two calls must have written the same elements, with the same bits.

A backward call finds the workspace and the outputs of its forward call in the guarded buffers of the replay, so the
state a workspace carries from one to the other is covered.  ROLES names the buffers of every entry point; the recorder
itself asserts that no call changed an argument that ROLES takes for an input.
"""
import pytest
import torch

import anchored as A
from multi_part_assembly_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 1 << 18   # elements of margin on either side of every guarded buffer
PATTERN = 0x5A    # every byte of the margins and of the interiors before the call (float32: 1.5e16)
PATTERN_WRAPPER = 0xA5  # every byte of the wrapper's own outputs before its call (float32: -2.9e-16)

# entry point -> {index of the argument (the stream excluded): "ws" workspace | "out" written | "io" updated in place}
ROLES = {
    "mpa_assembly_order": {5: "out"},
    "mpa_assembly_loss_forward_ordered": {13: "ws", 14: "ws", 15: "out"},
    "mpa_assembly_loss_forward_rmat_ordered": {13: "ws", 14: "ws", 15: "out"},
    "mpa_assembly_loss_backward": {11: "ws", 12: "ws", 13: "out", 14: "out"},
    "mpa_assembly_loss_backward_rmat": {11: "ws", 12: "ws", 13: "out", 14: "out"},
    "mpa_pointnet_forward": {5: "io", 6: "io", 13: "ws", 14: "ws", 15: "out"},
    "mpa_pointnet_backward": {8: "ws", 9: "ws", 10: "out", 11: "out", 12: "out"},
    "mpa_transformer_forward": {12: "ws", 13: "out"},
    "mpa_transformer_backward": {12: "ws", 13: "out", 14: "out"},
    "mpa_pose_head_forward": {4: "ws", 5: "out", 6: "out"},
    "mpa_pose_head_backward": {6: "ws", 7: "out", 8: "out"},
    "mpa_pose_head6_forward": {4: "ws", 5: "out", 6: "out"},
    "mpa_pose_head6_backward": {6: "ws", 7: "out", 8: "out"},
    "mpa_mlp_layer_forward": {6: "io", 7: "io", 15: "ws", 16: "out"},
    "mpa_mlp_layer_backward": {10: "ws", 11: "out", 12: "out", 13: "out", 14: "out", 15: "out"},
    "mpa_pair_layer_forward": {6: "io", 7: "io", 16: "ws", 17: "out"},
    "mpa_pair_layer_backward": {11: "ws", 12: "out", 13: "out", 14: "out", 15: "out", 16: "out", 17: "out"},
    "mpa_narrow_linear_relu_forward": {6: "out"},
    "mpa_narrow_linear_relu_backward": {7: "ws", 8: "out", 9: "out", 10: "out"},
    "mpa_relation_head_forward": {6: "ws", 7: "out"},
    "mpa_relation_head_backward": {6: "ws", 7: "out", 8: "out", 9: "out"},
    "mpa_gru_forward": {8: "ws", 9: "out", 10: "io"},
    "mpa_gru_backward": {8: "ws", 9: "out", 10: "out", 11: "out", 12: "io"},
    "mpa_seq2seq_decoder_forward": {13: "ws", 14: "out", 15: "out", 16: "out", 17: "io"},
    "mpa_seq2seq_decoder_backward": {6: "ws", 7: "out", 8: "out", 9: "out", 10: "out", 11: "io"},
    "mpa_dgcnn_forward": {5: "io", 6: "io", 15: "ws", 16: "out"},
    "mpa_dgcnn_backward": {7: "ws", 8: "out", 9: "out", 10: "out", 11: "out", 12: "out", 13: "out"},
    "mpa_knn_exact": {5: "ws", 6: "out"},
    "mpa_chamfer_forward_variant": {5: "out", 6: "out", 7: "out", 8: "out", 10: "ws"},
    "mpa_assembly_metrics": {9: "ws", 10: "out", 11: "out"},
    "mpa_assembly_metrics_rmat": {9: "ws", 10: "out", 11: "out"},
}


def _bytes(t):
    return t.reshape(-1).view(torch.uint8)


def _written(t, pattern):
    """Mask of the elements of `t` that do not hold `pattern` in every byte, and `t` as integers of its element size."""
    ints = t.reshape(-1).view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    pat = torch.empty(1, dtype=ints.dtype, device=t.device)
    _bytes(pat).fill_(pattern)
    return ints != pat, ints


def _same_writes(buf, after):
    wb, ib = _written(buf, PATTERN)
    wa, ia = _written(after, PATTERN_WRAPPER)
    return torch.equal(wb, wa) and torch.equal(ib[wb], ia[wa])


def _tensors(arg):
    return list(arg) if isinstance(arg, (list, tuple)) else [arg]


def _snapshot(args):
    return [[t.detach().clone() if isinstance(t, torch.Tensor) else t for t in _tensors(a)] for a in args]


class Recorder:
    """Stands in for `_lib.launch` while a wrapper runs: makes the call and keeps (name, arguments, their values before,
    their values after)."""

    def __init__(self, launch):
        self.launch, self.calls = launch, []

    def __call__(self, name, dev, *args, timer=None):
        if name not in ROLES:
            return self.launch(name, dev, *args, timer=timer)
        for i, a in enumerate(args):
            if ROLES[name].get(i) == "out":  # (what `torch.empty` left there is arbitrary anyway)
                for t in _tensors(a):
                    if isinstance(t, torch.Tensor):
                        _bytes(t).fill_(PATTERN_WRAPPER)
        pre = _snapshot(args)
        self.launch(name, dev, *args, timer=timer)
        torch.cuda.synchronize(dev)
        post = _snapshot(args)
        for i, (a, b) in enumerate(zip(pre, post)):
            if i not in ROLES[name]:
                for x, y in zip(a, b):
                    assert not isinstance(x, torch.Tensor) or torch.equal(_bytes(x), _bytes(y)), \
                        f"{name}: argument {i} changed during the call, and ROLES takes it for an input"
        self.calls.append((name, dev, args, pre, post))


@pytest.fixture
def record(monkeypatch):
    rec = Recorder(_lib.launch)
    monkeypatch.setattr(_lib, "launch", rec)
    return rec


class Guards:
    def __init__(self, dev):
        self.dev, self.all, self.twin = dev, [], {}

    def new(self, like, fill=None):
        n = like.numel()
        big = torch.empty(n + 2 * GUARD, dtype=like.dtype, device=self.dev)
        _bytes(big).fill_(PATTERN)
        if fill is not None:
            big[GUARD:GUARD + n].copy_(fill.reshape(-1))
        self.all.append((big, n))
        return big[GUARD:GUARD + n]

    def intact(self):
        return all(bool((_bytes(big[:GUARD]) == PATTERN).all()) and bool((_bytes(big[GUARD + n:]) == PATTERN).all())
                   for big, n in self.all)


def replay(rec):
    """Every recorded call again, through the C ABI, on guarded buffers; returns the number of calls made."""
    L = _lib.lib()
    done = 0
    for dev in {c[1] for c in rec.calls}:
        g = Guards(dev)
        for name, _, args, pre, post in [c for c in rec.calls if c[1] == dev]:
            conv, outs = [], []
            for i, a in enumerate(args):
                role = ROLES[name].get(i)
                row = []
                for t, before, after in zip(_tensors(a), pre[i], post[i]):
                    if not isinstance(t, torch.Tensor):
                        row.append(t)
                        continue
                    assert t.is_contiguous(), (name, i)
                    key = t.data_ptr()
                    if t.numel() and key in g.twin:      # produced by an earlier call of the replay
                        buf = g.twin[key]
                    elif role is None:
                        buf = before
                    else:
                        buf = g.new(t, before if role == "io" else None)
                        if t.numel():
                            g.twin[key] = buf
                    if role in ("out", "io"):
                        outs.append((i, role, buf, after))
                    row.append(buf)
                conv.append(_lib.ptr_array(row) if isinstance(a, (list, tuple)) else
                            row[0].data_ptr() if isinstance(row[0], torch.Tensor) else row[0])
            with torch.cuda.device(dev):
                st = getattr(L, name)(*conv, torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(st, name)
            torch.cuda.synchronize(dev)
            assert g.intact(), f"{name}: a guard margin was written"
            for i, role, buf, after in outs:
                same = torch.equal(_bytes(buf), _bytes(after)) if role == "io" else _same_writes(buf, after)
                assert same, f"{name}: argument {i} differs from the wrapper's result"
            done += 1
    return done


def _names(rec):
    return [c[0] for c in rec.calls]


# ---- fused loss ----------------------------------------------------------------------------------------------------
LOSS_SHAPES = [(1, 1, 1), (3, 5, 37), (2, 3, 64), (2, 3, 65), (1, 64, 33), (1, 2, 2048), (1, 2, 2049)]


@pytest.mark.parametrize("rot", ["quat", "rmat"])
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=["x".join(map(str, s)) for s in LOSS_SHAPES])
def test_fused_loss(cuda_device, record, shape, rot):
    """Forward and backward under every search (0 brute, 1 grid, 2 leaf, 3 auto), with the library's own k-d order and
    with a caller-made one.  2049 points per part is the first size without a leaf region (no order to make)."""
    from multi_part_assembly_amd.loss import _AssemblyLoss, part_order
    from multi_part_assembly_amd.rotation import quat_to_matrix
    B, P, N = shape
    dev = cuda_device
    g = torch.Generator().manual_seed(B * 10000 + P * 100 + N)
    pcs = (torch.randn(B, P, N, 3, generator=g) * 0.2).to(dev)
    valids = (torch.arange(P)[None] < torch.randint(1, P + 1, (B, 1), generator=g)).float().to(dev)
    quat = lambda: torch.nn.functional.normalize(torch.randn(B, P, 4, generator=g), dim=-1).to(dev)
    as_rot = (lambda q: quat_to_matrix(q).contiguous()) if rot == "rmat" else (lambda q: q)
    rp, rg = as_rot(quat()), as_rot(quat())
    tp, tg = (torch.randn(B, P, 3, generator=g) * 0.05).to(dev), (torch.randn(B, P, 3, generator=g) * 0.05).to(dev)
    go = torch.randn(5, B, generator=g).to(dev)
    order = part_order(pcs, valids)
    assert (order is None) == (N > 2048)
    runs = 0
    for search in (0, 1, 2, 3):
        for o in (None, order) if order is not None else (None,):
            a, b = rp.clone().requires_grad_(), tp.clone().requires_grad_()
            losses, _ = _AssemblyLoss.apply(pcs, valids, a, b, rg, tg, True, False, o, search)
            losses.backward(go)
            runs += 1
    assert replay(record) == 2 * runs + (order is not None)


# ---- PointNet ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,valids", [((1, 1, 64), None), ((3, 33, 128), [1, 0, 1]), ((5, 100, 256), None)],
                         ids=["1x1x64", "3x33x128", "5x100x256"])
def test_pointnet(cuda_device, record, shape, valids):
    enc, pts, v, w = A.pointnet_case(shape, valids)
    enc.to(cuda_device)
    out = enc.forward_parts(pts.to(cuda_device), v.to(cuda_device))
    (out * w.to(cuda_device)).sum().backward()
    assert _names(record) == ["mpa_pointnet_forward", "mpa_pointnet_backward"]
    assert replay(record) == 2


# ---- transformer and pose heads ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(1, 1, 256, 8, 1024, 2), (2, 32, 64, 1, 64, 1)], ids=["1x1x256x8x1024x2", "2x32x64x1x64x1"])
def test_transformer(cuda_device, record, dims):
    from multi_part_assembly_amd.transformer import _TransformerFn
    enc, tok0, valid, w = A.transformer_case(dims)
    enc.to(cuda_device).train()
    tok = tok0.to(cuda_device).requires_grad_()
    out = _TransformerFn.apply(tok, valid.reshape(-1).float().to(cuda_device), dims[3], 0.1, 0xA5EED0123457, None,
                               *enc._params())
    (out * w.to(cuda_device)).sum().backward()
    assert _names(record) == ["mpa_transformer_forward", "mpa_transformer_backward"]
    assert replay(record) == 2


@pytest.mark.parametrize("rot_type,entry", [("quat", "mpa_pose_head"), ("rmat", "mpa_pose_head6")])
@pytest.mark.parametrize("rows,width", [(2, 8), (1, 64), (35, 135)], ids=["2x8", "1x64", "35x135"])
def test_pose_heads(cuda_device, record, rows, width, rot_type, entry):
    """Widths that are (64) and are not (8, 135) multiples of the GEMM panels' 64 columns: the padded x' | w' | dx' | dw'
    tail of the workspace."""
    from multi_part_assembly_amd.regressor import PoseRegressor
    torch.manual_seed(rows + width)
    head = PoseRegressor(width, rot_type=rot_type).to(cuda_device).train()
    assert head.native
    x = torch.randn(rows, width, device=cuda_device, requires_grad=True)
    r, t = head(x)
    ((r * torch.randn_like(r)).sum() + (t * torch.randn_like(t)).sum()).backward()
    assert _names(record) == [entry + "_forward", entry + "_backward"]
    assert replay(record) == 2


# ---- the smaller families: one case each, at the smallest shape of the family's own GPU test ------------------------
def test_mlp_layer(cuda_device, record):
    """35 rows, 128 -> 512 with BatchNorm (tests/test_callers_gpu.py: the pair MLPs' first layer over 7 x 5 rows)."""
    from multi_part_assembly_amd.mlp import mlp_layer
    torch.manual_seed(1)
    conv, bn = torch.nn.Conv1d(128, 512, 1).to(cuda_device), torch.nn.BatchNorm1d(512).to(cuda_device)
    x = torch.randn(35, 128, device=cuda_device, requires_grad=True)
    y = mlp_layer(x, conv.weight, conv.bias, bn, relu=True, training=True)
    (y * torch.randn_like(y)).sum().backward()
    assert _names(record) == ["mpa_mlp_layer_forward", "mpa_mlp_layer_backward"]
    assert replay(record) == 2


def test_pair_layer(cuda_device, record):
    """(B, P, F) = (3, 5, 64) into the edge MLP's 512 channels (tests/test_callers_gpu.py)."""
    from multi_part_assembly_amd.mlp import pair_layer
    torch.manual_seed(2)
    conv, bn = torch.nn.Conv1d(128, 512, 1).to(cuda_device), torch.nn.BatchNorm1d(512).to(cuda_device)
    a = torch.randn(3, 5, 64, device=cuda_device, requires_grad=True)
    b = torch.randn(3, 5, 64, device=cuda_device, requires_grad=True)
    y = pair_layer(a, b, conv.weight, conv.bias, bn, relu=True, training=True)
    (y * torch.randn_like(y)).sum().backward()
    assert _names(record) == ["mpa_pair_layer_forward", "mpa_pair_layer_backward"]
    assert replay(record) == 2


def test_narrow_linear(cuda_device, record):
    """(R, K, N) = (5, 1, 3) (tests/test_callers_gpu.py)."""
    from multi_part_assembly_amd.gnn_ops import narrow_linear_relu
    torch.manual_seed(3)
    lin = torch.nn.Linear(1, 3).to(cuda_device)
    x = torch.randn(5, 1, device=cuda_device, requires_grad=True)
    y = narrow_linear_relu(x, lin.weight, lin.bias)
    (y * torch.randn_like(y)).sum().backward()
    assert _names(record) == ["mpa_narrow_linear_relu_forward", "mpa_narrow_linear_relu_backward"]
    assert replay(record) == 2


def test_relation_head(cuda_device, record):
    """8 rows of width 8 (tests/test_lib_call.py)."""
    from multi_part_assembly_amd.gnn_ops import relation_head
    torch.manual_seed(4)
    lin = torch.nn.Linear(8, 1).to(cuda_device)
    h = torch.randn(8, 8, device=cuda_device, requires_grad=True)
    y = relation_head(h, lin.weight, lin.bias)
    (y * torch.randn_like(y)).sum().backward()
    assert _names(record) == ["mpa_relation_head_forward", "mpa_relation_head_backward"]
    assert replay(record) == 2


def test_gru(cuda_device, record):
    """(D, B, T, H) = (2, 3, 5, 128) (tests/test_callers_gpu.py, where the grid is co-resident)."""
    from multi_part_assembly_amd.gru import gru_recurrent, raise_if_failed, supported
    D, B, T, H = 2, 3, 5, 128
    assert supported(H, B, D)
    torch.manual_seed(5)
    gi = torch.randn(D, B, T, 3 * H, device=cuda_device, requires_grad=True)
    h0 = torch.randn(D, B, H, device=cuda_device)
    whh = (torch.randn(D, 3 * H, H, device=cuda_device) / H ** 0.5).requires_grad_()
    bhh = (0.1 * torch.randn(D, 3 * H, device=cuda_device)).requires_grad_()
    out = gru_recurrent(gi, h0, whh, bhh)
    (out * torch.randn_like(out)).sum().backward()
    raise_if_failed(cuda_device, synchronize=True)
    assert _names(record) == ["mpa_gru_forward", "mpa_gru_backward"]
    assert replay(record) == 2


def test_seq2seq_decoder(cuda_device, record):
    """B = 4 sequences of one part, teacher forcing (tests/test_lstm_gpu.py: the "P1" case, co-resident there)."""
    import random
    import numpy as np
    from multi_part_assembly_amd.lstm import Seq2Seq
    B, P = 4, 1
    torch.manual_seed(6)
    np.random.seed(6)
    random.seed(6)
    s2s = Seq2Seq(128, 128, 256).to(cuda_device).train()
    x = torch.randn(P, B, 128, device=cuda_device, requires_grad=True)
    valids = torch.ones(B, P, device=cuda_device)
    y, _ = s2s(x, x.detach(), valids=valids, teacher_forcing_ratio=1.0, hip=True)
    (y * torch.randn_like(y)).sum().backward()
    names = _names(record)  # (the encoder in front of the decoder runs on csrc/gru.hip: its two calls are replayed too)
    assert "mpa_seq2seq_decoder_forward" in names and "mpa_seq2seq_decoder_backward" in names
    assert replay(record) == len(names)


def test_dgcnn(cuda_device, record):
    """(M, N, F) = (4, 20, 64): k = 20 of 20 points (tests/test_dgcnn_gpu.py)."""
    from multi_part_assembly_amd.encoder import DGCNN
    torch.manual_seed(21)
    enc = DGCNN(64).to(cuda_device).train()
    pcs = torch.randn(4, 20, 3, device=cuda_device) * 0.2
    out = enc.forward_parts(pcs, torch.ones(4, device=cuda_device))
    (out * torch.randn_like(out)).sum().backward()
    assert _names(record) == ["mpa_dgcnn_forward", "mpa_dgcnn_backward"]
    assert replay(record) == 2


def test_knn_exact(cuda_device, record):
    """One cloud of 20 points in 64 dimensions (tests/test_dgcnn_gpu.py)."""
    from multi_part_assembly_amd.encoder import knn_exact
    torch.manual_seed(7)
    knn_exact(torch.randn(20, 64, device=cuda_device), 1, 20, 64)
    assert _names(record) == ["mpa_knn_exact"]
    assert replay(record) == 1


def test_cloud_grid_chamfer(cuda_device, record):
    """variant 3, the grid-pruned search of two plain clouds, at (B, n1, n2) = (2, 1, 1500) (tests/test_chamfer_gpu.py)."""
    from multi_part_assembly_amd.chamfer import chamfer_forward
    torch.manual_seed(8)
    chamfer_forward(torch.randn(2, 1, 3, device=cuda_device), torch.randn(2, 1500, 3, device=cuda_device), variant=3)
    assert _names(record) == ["mpa_chamfer_forward_variant"]
    assert replay(record) == 1


@pytest.mark.parametrize("kind", ["quat", "rmat"])
def test_assembly_metrics(golden, cuda_device, record, kind):
    """The "small" batch of tests/test_eval_metrics_gpu.py, with the per-part output."""
    from multi_part_assembly_amd import eval_utils
    from multi_part_assembly_amd.rotation import Rotation3D
    z = golden("eval_metrics_v2")
    t = lambda k: torch.from_numpy(z[k].copy()).to(cuda_device)
    pr_r, gt_r = Rotation3D(t(f"small.{kind}.pr_rot"), kind), Rotation3D(t(f"small.{kind}.gt_rot"), kind)
    eval_utils.assembly_metrics(t("small.pcs"), t("small.pr_t"), t("small.gt_t"), pr_r, gt_r, t("small.valids"),
                                ret_per_part=True)
    assert _names(record) == ["mpa_assembly_metrics_rmat" if kind == "rmat" else "mpa_assembly_metrics"]
    assert replay(record) == 1
