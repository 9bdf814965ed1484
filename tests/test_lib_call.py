"""The two helpers every call into libmpa_hip.so goes through (`_lib.query`, `_lib.launch`): what they pass on, which
stream they launch on, what they time and under which name they fail.  The queries are pure host arithmetic and run on
the CPU; the launches are compared bit for bit with the same call written out by hand."""
import ctypes

import pytest
import torch

from multi_part_assembly_amd import _build, _lib

B, P, N = 1, 2, 5  # the pose-apply case: B * P parts of N points


@pytest.fixture(scope="module")
def built():
    return _build.build()


def test_query_agrees_with_the_direct_call(built):
    L = _lib.lib()
    assert _lib.query("mpa_narrow_linear_relu_workspace", 640, 7, 256) == 5 * 256 * 17
    assert _lib.query("mpa_pose_head_workspace", 640, 135) == 640 * 780 + 64 + 2 * (640 + 256) * 192
    nf, ni = ctypes.c_int64(), ctypes.c_int64()
    assert L.mpa_assembly_loss_workspace(2, 3, 40, ctypes.byref(nf), ctypes.byref(ni)) == 0
    pair = _lib.query("mpa_assembly_loss_workspace", 2, 3, 40)
    assert pair == (nf.value, ni.value) and nf.value > 0 and all(type(v) is int for v in pair)
    nb = ctypes.c_int64()
    assert L.mpa_grad_clip_workspace(ctypes.byref(nb)) == 0  # no size argument at all: one out-slot
    assert _lib.query("mpa_grad_clip_workspace") == nb.value


def test_failing_query_names_itself(built):
    with pytest.raises(_lib.MpaError) as err:
        _lib.query("mpa_narrow_linear_relu_workspace", 640, 17, 256)
    assert "mpa_narrow_linear_relu_workspace" in str(err.value) and "K=17" in str(err.value)


# ---- on the device ---------------------------------------------------------------------------------------------------
def _rand(dev, *shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)


@pytest.fixture(scope="module")
def pose(cuda_device):
    """Inputs of mpa_pose_apply_forward and its result from a launch on the default stream."""
    pc, trans = _rand(cuda_device, B * P, N, 3, seed=1), _rand(cuda_device, B * P, 3, seed=2)
    quat = torch.nn.functional.normalize(_rand(cuda_device, B * P, 4, seed=3), dim=-1)
    want = _pose_apply(pc, quat, trans, torch.empty_like(pc))
    torch.cuda.synchronize()
    return pc, quat, trans, want.clone()


def _pose_apply(pc, quat, trans, out):
    _lib.launch("mpa_pose_apply_forward", pc.device, pc, quat, trans, None, 0.0, B * P, N, out)
    return out


@pytest.mark.gpu
def test_launch_reads_the_stream_at_call_time(pose):
    pc, quat, trans, want = pose
    side = torch.cuda.Stream(device=pc.device)
    out = torch.full_like(pc, float("nan"))
    torch.cuda.synchronize()
    # the default stream is kept busy: a launch that went there instead of `side` would not be over when `done` is
    busy = torch.zeros(1 << 27, device=pc.device)
    for _ in range(16):
        busy.add_(1.0)
    with torch.cuda.stream(side):
        _pose_apply(pc, quat, trans, out)
        done = torch.cuda.Event()
        done.record()
        done.synchronize()
        early = out.to("cpu")  # (copied on `side`: does not wait for the default stream)
    side.synchronize()
    late = out.to("cpu")
    torch.cuda.synchronize()
    assert torch.equal(early, late) and torch.equal(late, want.cpu())
    assert float(busy[0]) == 16.0


@pytest.mark.gpu
def test_launch_is_captured_into_a_graph(pose):
    pc, quat, trans, want = pose
    out = torch.empty_like(pc)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _pose_apply(pc, quat, trans, out)
    out.fill_(float("nan"))  # the capture ran nothing; the replay is what writes
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


def _by_hand(name, dev, *args):
    """The call as the wrappers wrote it out before: pointers taken with _lib.ptr / _lib.ptr_array by the caller."""
    with torch.cuda.device(dev):
        st = getattr(_lib.lib(), name)(*args, _lib.current_stream(dev))
    _lib.check(st, name)


@pytest.mark.gpu
def test_launch_maps_none_lists_and_bools_like_the_hand_written_call(cuda_device):
    dev, f32 = cuda_device, torch.float32
    # None -> NULL: the relation head without bias and mask, R = K = 8
    h, w = _rand(dev, 8, 8, seed=4), _rand(dev, 8, seed=5)
    outs = []
    for call in (_lib.launch, _by_hand):
        ws = torch.empty(_lib.query("mpa_relation_head_workspace", 8, 8), dtype=f32, device=dev)
        out = torch.empty(8, dtype=f32, device=dev)
        if call is _lib.launch:
            call("mpa_relation_head_forward", dev, h, w, None, None, 8, 8, ws, out)
        else:
            call("mpa_relation_head_forward", dev, _lib.ptr(h), _lib.ptr(w), None, None, 8, 8, _lib.ptr(ws), _lib.ptr(out))
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and bool(((outs[0] >= 0) & (outs[0] <= 1)).all())

    # a list of tensors -> host pointer array: the pose head's eight parameters, M = 2, F = 8
    from multi_part_assembly_amd.regressor import PoseRegressor
    torch.manual_seed(0)
    head = PoseRegressor(8).to(dev)
    params = [head.fc_layers[0].weight, head.fc_layers[0].bias, head.fc_layers[2].weight, head.fc_layers[2].bias,
              head.rot_head.weight, head.rot_head.bias, head.trans_head.weight, head.trans_head.bias]
    x = _rand(dev, 2, 8, seed=6)
    outs = []
    for call in (_lib.launch, _by_hand):
        ws = torch.empty(_lib.query("mpa_pose_head_workspace", 2, 8), dtype=f32, device=dev)
        rot, trans = torch.empty((2, 4), dtype=f32, device=dev), torch.empty((2, 3), dtype=f32, device=dev)
        if call is _lib.launch:
            call("mpa_pose_head_forward", dev, x, params, 2, 8, ws, rot, trans)
        else:
            call("mpa_pose_head_forward", dev, _lib.ptr(x), _lib.ptr_array(params), 2, 8, _lib.ptr(ws), _lib.ptr(rot),
                 _lib.ptr(trans))
        outs.append((rot, trans))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.allclose(outs[0][0].norm(dim=-1), torch.ones(2, device=dev), atol=1e-5)  # (unit quaternions came out)

    # bool -> int: pair_rows' swap, S = 1, P = 2, F = 4
    a, b = _rand(dev, 1, 2, 4, seed=7), _rand(dev, 1, 2, 4, seed=8)
    got, ref = (torch.empty((1, 2, 2, 8), dtype=f32, device=dev) for _ in range(2))
    _lib.launch("mpa_pair_rows_forward", dev, a, b, 1, 2, 4, True, got)
    _by_hand("mpa_pair_rows_forward", dev, _lib.ptr(a), _lib.ptr(b), 1, 2, 4, 1, _lib.ptr(ref))
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    assert torch.equal(got[0, 0, 1], torch.cat([b[0, 1], a[0, 0]]))  # swapped: [b_j ; a_i]


@pytest.mark.gpu
def test_failing_launch_names_the_entry_point_it_called(cuda_device):
    """65 parts are outside the loss (1 <= P <= 64): refused by argument validation, in front of any launch."""
    from multi_part_assembly_amd.loss import _AssemblyLoss

    dev, parts = cuda_device, 65
    pcs = _rand(dev, 1, parts, N, 3, seed=9)
    valids, trans = torch.ones(1, parts, device=dev), torch.zeros(1, parts, 3, device=dev)
    rmat = torch.eye(3, device=dev).expand(1, parts, 3, 3).contiguous()
    with pytest.raises(_lib.MpaError) as err:
        _AssemblyLoss.apply(pcs, valids, rmat, trans, rmat, trans, True, False, None, 1)
    assert "mpa_assembly_loss_forward_rmat_ordered" in str(err.value)


@pytest.mark.gpu
def test_timer_brackets_only_what_is_wanted(cuda_device, monkeypatch):
    from multi_part_assembly_amd import gnn_ops

    dev = cuda_device
    a, b = _rand(dev, 1, 2, 4, seed=7), _rand(dev, 1, 2, 4, seed=8)
    h, w = _rand(dev, 8, 8, seed=4), _rand(dev, 1, 8, seed=5)
    timer = _lib.KernelTimer(only=("pair_rows_forward",))
    _lib.KernelTimer.active = timer
    try:
        gnn_ops.pair_rows(a, b)
        gnn_ops.relation_head(h, w)
    finally:
        _lib.KernelTimer.active = None
    torch.cuda.synchronize()
    assert list(timer.events) == ["pair_rows_forward[1x2x4]"] and len(timer.events["pair_rows_forward[1x2x4]"]) == 1
    assert timer.summary()["pair_rows_forward[1x2x4]"]["launches"] == 1

    def no_event(*args, **kwargs):
        raise AssertionError("an event was created with no timer active")

    monkeypatch.setattr(torch.cuda, "Event", no_event)
    out = torch.empty((1, 2, 2, 8), dtype=torch.float32, device=dev)
    _lib.launch("mpa_pair_rows_forward", dev, a, b, 1, 2, 4, False, out, timer="pair_rows_forward[1x2x4]")
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert torch.equal(out, gnn_ops.pair_rows(a, b))
