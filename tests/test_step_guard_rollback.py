"""Buffer rollback of the guarded step without a device: the restatement `guard_ref.commit` over hand-written
apply / skip / skip / apply sequences, the layout of `optim.BufferSlab` and its edge cases, the argument refusals
(FusedAdam, Trainer, tools/train.py, and mpa_guard_commit's through `_lib`), and the launches of a step with the switch
off (the parent's) and on (exactly one more, mpa_guard_commit)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

from multi_part_assembly_amd import _lib, guard_ref
from multi_part_assembly_amd.optim import BufferSlab, FlatBuffers, FusedAdam
from tool_loader import load_tool as _tool
from trainer_cases import built, optimizer_presets, record as _record, tiny_cfg as _tiny_cfg  # noqa: F401


def _bytes(n, seed):
    return np.random.RandomState(seed).randint(0, 256, size=n).astype(np.uint8)


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------
def test_commit_direction_is_bitwise_and_returns_new_arrays():
    live, shadow = _bytes(48, 0), _bytes(48, 1)
    keep_live, keep_shadow = live.copy(), shadow.copy()
    a, b = guard_ref.commit(0, live, shadow)  # applied: shadow <- live
    assert np.array_equal(a, keep_live) and np.array_equal(b, keep_live)
    for verdict in (1, 2, 3):                 # every non-zero verdict means skip: live <- shadow
        a, b = guard_ref.commit(verdict, live, shadow)
        assert np.array_equal(a, keep_shadow) and np.array_equal(b, keep_shadow)
    assert np.array_equal(live, keep_live) and np.array_equal(shadow, keep_shadow)  # the inputs are not written
    a, b = guard_ref.commit(1, live[:0], shadow[:0])
    assert a.size == b.size == 0
    # NaN payloads, -0 and an int64 counter pass through as bits
    words = np.array([0x7FC00001, 0xFFC12345, 0x80000000, 0x7F800000], dtype=np.uint32).view(np.uint8)
    counter = np.array([2 ** 40 + 3, -7], dtype=np.int64).view(np.uint8)
    special = np.concatenate([words, counter])
    a, _ = guard_ref.commit(2, np.zeros_like(special), special)
    assert a.tobytes() == special.tobytes()
    with pytest.raises(ValueError, match="multiple of 16"):
        guard_ref.commit(0, live[:40], shadow[:40])
    with pytest.raises(ValueError, match="equal size"):
        guard_ref.commit(0, live, shadow[:32])
    with pytest.raises(ValueError, match="uint8"):
        guard_ref.commit(0, live.view(np.float32), shadow.view(np.float32))


def test_a_slab_carried_through_apply_skip_skip_apply():
    """Each step's forward leaves fresh bytes in the live slab; after a skip the live slab has the bits of the last
    APPLIED step's end, after an apply the shadow equals the live slab."""
    rng = np.random.RandomState(5)
    clean = rng.randn(11).astype(np.float32)
    nan7 = clean.copy()
    nan7[7] = np.nan
    fwd = [_bytes(64, 10 + k) for k in range(4)]
    start = _bytes(64, 9)
    state = (rng.randn(11).astype(np.float32), np.zeros(11, np.float32), np.zeros(11, np.float32))
    hyper, words = guard_ref.new_hyper(), np.zeros(8, dtype=np.int32)
    live, shadow = start.copy(), start.copy()
    seen = []
    # apply, skip (NaN), skip (status word AND NaN: verdict 3), apply
    for k, (grad, status) in enumerate([(clean, None), (nan7, 0), (nan7, 4), (clean, 0)]):
        live, shadow, verdicts = guard_ref.run_steps([(grad, status, fwd[k])], state, live, shadow, hyper=hyper, guard=words)
        seen.append((verdicts[0], live.copy(), shadow.copy()))
    assert [s[0] for s in seen] == [0, 1, 3, 0]
    assert np.array_equal(seen[0][1], fwd[0]) and np.array_equal(seen[0][2], fwd[0])
    for k in (1, 2):  # both skips return to the end of step 1, whatever their own forward wrote
        assert np.array_equal(seen[k][1], fwd[0]) and np.array_equal(seen[k][2], fwd[0])
    assert np.array_equal(seen[3][1], fwd[3]) and np.array_equal(seen[3][2], fwd[3])
    assert words.tolist()[:4] == [0, 2, 2, 0]
    # the status word alone (verdict 2) skips as well, and a first step that is skipped returns to the initial bytes
    live, shadow, verdicts = guard_ref.run_steps([(clean, 1, fwd[1])], state, start.copy(), start.copy())
    assert verdicts == [2] and np.array_equal(live, start) and np.array_equal(shadow, start)
    # the whole sequence in one call gives the same end
    state2 = (np.zeros(11, np.float32), np.zeros(11, np.float32), np.zeros(11, np.float32))
    live, shadow, verdicts = guard_ref.run_steps(
        [(clean, None, fwd[0]), (nan7, 0, fwd[1]), (nan7, 4, fwd[2])], state2, start.copy(), start.copy())
    assert verdicts == [0, 1, 3] and np.array_equal(live, fwd[0]) and np.array_equal(shadow, fwd[0])


# ---- 2. the slab ---------------------------------------------------------------------------------------------------------------
class Block(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = nn.Linear(6, 5)
        self.bn = nn.BatchNorm1d(5)

    def forward(self, x):
        return self.bn(self.fc(x))


class Small(nn.Module):
    """BatchNorm1d and BatchNorm2d, a hand-registered bool buffer, a non-persistent buffer, a zero-size buffer and a
    sub-module that is registered twice."""

    def __init__(self):
        super().__init__()
        self.block = Block()
        self.again = self.block  # shared
        self.conv = nn.Conv2d(1, 3, 1)
        self.bn2 = nn.BatchNorm2d(3)
        self.register_buffer("flags", torch.tensor([True, False, True]))
        self.register_buffer("scratch", torch.arange(7, dtype=torch.float64), persistent=False)
        self.register_buffer("empty", torch.zeros(0))

    def forward(self, x):
        y = self.again(self.block(x) @ torch.ones(5, 6))
        return y.sum() + self.bn2(self.conv(x[:, :4].reshape(-1, 1, 2, 2))).sum()


def _small(seed=0):
    torch.manual_seed(seed)
    m = Small()
    with torch.no_grad():
        m.block.bn.running_mean.copy_(torch.randn(5))
        m.bn2.running_var.copy_(torch.rand(3) + 0.5)
        m.block.bn.num_batches_tracked.fill_(41)
    return m


def test_slab_layout_views_values_and_state_dict():
    m = _small()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    named_before = {k: v.clone() for k, v in m.named_buffers()}
    slab = BufferSlab(m)
    names = [n for n, _ in m.named_buffers()]
    assert slab.names == names and len(names) == len(set(names))
    assert "again.bn.running_mean" not in names and "block.bn.running_mean" in names  # the shared module: one slot
    assert "scratch" in names and "scratch" not in m.state_dict()                    # non-persistent: in the slab
    assert all(off % 16 == 0 for off in slab.offsets) and slab.nbytes % 16 == 0
    assert slab.live.dtype == torch.uint8 and slab.live.numel() == slab.nbytes == slab.shadow.numel()
    assert slab.live.data_ptr() % 16 == 0 and slab.shadow.data_ptr() % 16 == 0
    assert slab.shadow.data_ptr() != slab.live.data_ptr() and torch.equal(slab.shadow, slab.live)
    used = np.zeros(slab.nbytes, dtype=bool)
    for (name, b), off, size in zip(m.named_buffers(), slab.offsets, slab.sizes):
        assert size == b.numel() * b.element_size()
        assert not used[off:off + size].any()  # slots do not overlap
        used[off:off + size] = True
        if b.numel():
            assert b.data_ptr() == slab.live.data_ptr() + off, name
        assert b.dtype == named_before[name].dtype and b.shape == named_before[name].shape
        assert torch.equal(b, named_before[name]), name
    assert not slab.live.numpy()[~used].any()  # the padding is zero
    assert m.again.bn.running_mean is m.block.bn.running_mean
    after = m.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    slab.check()
    # the counters are int64, count under module(x) in training mode, and the statistics move INSIDE the slab
    assert m.block.bn.num_batches_tracked.dtype == torch.int64 and m.flags.dtype == torch.bool
    m.train()
    snapshot = slab.live.clone()
    m(torch.randn(8, 6))
    assert int(m.block.bn.num_batches_tracked) == 43 and int(m.bn2.num_batches_tracked) == 1  # (the shared block ran twice)
    assert not torch.equal(slab.live, snapshot) and torch.equal(slab.shadow, snapshot)
    slab.check()
    # a skip on the host restores every buffer, an apply makes the current bits the shadow
    slab.commit(torch.tensor([2], dtype=torch.int32))
    assert torch.equal(slab.live, snapshot) and int(m.block.bn.num_batches_tracked) == 41
    assert torch.equal(m.block.bn.running_mean, named_before["block.bn.running_mean"])
    m(torch.randn(8, 6))
    moved = slab.live.clone()
    slab.commit(torch.tensor([0], dtype=torch.int32))
    assert torch.equal(slab.live, moved) and torch.equal(slab.shadow, moved)
    # load_state_dict copies in place: the buffers stay views, refresh() takes the loaded bits
    m.load_state_dict(before)
    slab.check()
    assert not torch.equal(slab.shadow, slab.live)
    slab.refresh()
    assert torch.equal(slab.shadow, slab.live) and int(m.block.bn.num_batches_tracked) == 41


def test_slab_edge_cases():
    bare = nn.Sequential(nn.Linear(3, 3), nn.ReLU())
    slab = BufferSlab(bare)
    assert slab.nbytes == 0 and slab.live.numel() == 0 and slab.names == []
    slab.check()
    slab.refresh()
    slab.commit(torch.tensor([1], dtype=torch.int32))  # nothing to do, nothing launched
    m = _small()
    slab = BufferSlab(m)
    m.double()
    with pytest.raises(RuntimeError, match="buffer empty no longer lives"):  # (the first buffer in module order that moved)
        slab.check()
    m = _small()
    slab = BufferSlab(m)
    m.block.double()
    with pytest.raises(RuntimeError, match=r"block\.bn\.running_mean"):
        slab.check()
    m = _small()
    slab = BufferSlab(m)
    m.bn2.register_buffer("running_var", torch.ones(3))  # registered anew: no longer the slab's view
    with pytest.raises(RuntimeError, match=r"bn2\.running_var"):
        slab.check()
    m = _small()
    slab = BufferSlab(m)
    m.register_buffer("late", torch.zeros(2))
    with pytest.raises(RuntimeError, match="late"):
        slab.check()


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------
def test_python_side_refusals_and_the_configuration_key():
    from multi_part_assembly_amd.pn_transformer import build_model
    from multi_part_assembly_amd.trainer import Trainer
    slab = BufferSlab(_small())
    with pytest.raises(ValueError, match="guard=True"):
        FusedAdam(FlatBuffers([nn.Parameter(torch.zeros(4))]), guard=False, guard_state=slab)
    assert FusedAdam(FlatBuffers([nn.Parameter(torch.zeros(4))]), guard=True, guard_state=slab).guard_state is slab
    cfg = _tiny_cfg()
    with pytest.raises(ValueError, match="guard_step"):
        Trainer(build_model(cfg), cfg, guard_buffers=True)
    with pytest.raises(ValueError, match="guard_step"):
        Trainer(build_model(cfg), cfg, guard_step=False, guard_buffers=True)
    off = Trainer(build_model(cfg), cfg, guard_step=True)
    assert off.guard_buffers is False and off.buffer_slab is None and off.optimizer.guard_state is None
    cfg.optimizer.skip_nonfinite = True
    cfg.optimizer.skip_rollback_buffers = True
    on = Trainer(build_model(cfg), cfg)
    assert on.guard_buffers is True and on.optimizer.guard_state is on.buffer_slab and on.buffer_slab.nbytes > 0
    assert all(b.data_ptr() >= on.buffer_slab.live.data_ptr() for b in on.model.buffers())
    assert Trainer(build_model(cfg), cfg, guard_buffers=False).buffer_slab is None  # the argument wins
    on.model.double()
    with pytest.raises(RuntimeError, match="no longer lives in the slab"):
        on.state_dict()
    with_optimizer = optimizer_presets()
    assert len(with_optimizer) >= 10 and all("skip_rollback_buffers" not in c.optimizer for c in with_optimizer)
    # the tool
    tool = _tool("train")
    base = ["--preset", "pn_transformer_everyday", "--synthetic"]
    args = tool.parse_args(base + ["--skip-nonfinite"])
    assert args.rollback_buffers is False and "skip_rollback_buffers" not in tool.configure(args).optimizer
    args = tool.parse_args(base + ["--skip-nonfinite", "--rollback-buffers"])
    made = tool.configure(args)
    assert made.optimizer.skip_rollback_buffers is True and made.optimizer.skip_nonfinite is True
    with pytest.raises(SystemExit):
        tool.parse_args(base + ["--rollback-buffers"])


def test_trainer_load_state_dict_refreshes_the_shadow():
    from multi_part_assembly_amd.pn_transformer import build_model
    from multi_part_assembly_amd.trainer import Trainer
    cfg = _tiny_cfg()
    torch.manual_seed(1)
    t = Trainer(build_model(cfg), cfg, guard_step=True, guard_buffers=True)
    state = {"state_dict": {k: v.clone() for k, v in t.model.state_dict().items()}}
    name = next(n for n, _ in t.model.named_buffers() if n.endswith("running_mean"))
    state["state_dict"][name] += 3.0
    t.load_state_dict(state)
    slab = t.buffer_slab
    assert torch.equal(slab.shadow, slab.live)
    assert torch.equal(dict(t.model.named_buffers())[name], state["state_dict"][name])
    slab.check()


def test_entry_point_is_declared_and_refuses_bad_arguments_without_a_gpu(built):
    assert "mpa_guard_commit" in _lib.declared_functions() and _lib.ABI_VERSION == 10
    P, I64, INT = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert _lib.SIGNATURES["mpa_guard_commit"] == (INT, [P, P, P, I64, P])
    L = _lib.lib()
    a4, live, shadow = 4100, 4096, 8192  # addresses by alignment (never dereferenced: every call below launches nothing)
    commit = lambda *a: L.mpa_guard_commit(*a, None)  # noqa: E731
    assert commit(a4, None, None, 0) == 0                      # nothing to copy: success without a launch
    assert commit(a4, live, shadow, 0) == 0
    assert commit(None, live, shadow, 64) == -1 and b"null" in L.mpa_last_error()
    assert commit(None, None, None, 0) == -1 and b"null" in L.mpa_last_error()
    assert commit(a4 + 2, live, shadow, 64) == -1 and b"misaligned" in L.mpa_last_error()
    assert commit(a4, None, shadow, 64) == -1 and b"null" in L.mpa_last_error()
    assert commit(a4, live, None, 64) == -1 and b"null" in L.mpa_last_error()
    assert commit(a4, live + 8, shadow, 64) == -1 and b"aligned" in L.mpa_last_error()
    assert commit(a4, live, shadow + 4, 64) == -1 and b"aligned" in L.mpa_last_error()
    assert commit(a4, live, shadow, -16) == -1 and b"multiple of 16" in L.mpa_last_error()
    assert commit(a4, live, shadow, 24) == -1 and b"multiple of 16" in L.mpa_last_error()
    assert commit(a4, live, shadow, 1) == -1 and b"multiple of 16" in L.mpa_last_error()
    assert commit(a4, live, live, 64) == -1 and b"overlap" in L.mpa_last_error()
    assert commit(a4, live, live + 48, 64) == -1 and b"overlap" in L.mpa_last_error()
    assert commit(a4, live + 48, live, 64) == -1 and b"overlap" in L.mpa_last_error()
    assert commit(a4, live, shadow - 16, 4096) == -1 and b"overlap" in L.mpa_last_error()


# ---- 4. the launches of a step --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [None, 1.0])
def test_trainer_step_launches_switch_off_are_the_parents_and_on_is_one_more(monkeypatch, built, clip):
    """Recorded on a stub `_lib.launch` (host tensors, nothing runs)."""
    from multi_part_assembly_amd.pn_transformer import build_model
    from multi_part_assembly_amd.trainer import Trainer
    cfg = _tiny_cfg()
    cfg.optimizer.clip_grad = clip
    calls = _record(monkeypatch)
    parent = {False: (["mpa_grad_clip_coef"] if clip else []) + ["mpa_adam_step_dev"],
              True: ["mpa_step_guard", "mpa_adam_step_guarded"]}
    for guard_step, guard_buffers in ((False, None), (False, False), (True, None), (True, False), (True, True)):
        t = Trainer(build_model(cfg), cfg, guard_step=guard_step, guard_buffers=guard_buffers)
        opt = t.optimizer
        opt._hyper_dev = torch.zeros(8)  # (the device buffer of a real step)
        for _ in range(2):
            calls.clear()
            opt.step_dev()
            names = [c[0] for c in calls]
            if not guard_buffers:
                assert names == parent[guard_step], (guard_step, guard_buffers)
            else:
                assert names == parent[True] + ["mpa_guard_commit"]
                slab = t.buffer_slab
                last = calls[-1][1]
                assert last[0] is opt.guard_words() and last[1] is slab.live and last[2] is slab.shadow
                assert last[3] == slab.nbytes and len(last) == 4
                assert calls[0][1][8] is opt.guard_words() and calls[1][1][-1] is opt.guard_words()  # one verdict word


def test_a_model_without_buffers_launches_nothing_more(monkeypatch, built):
    calls = _record(monkeypatch)
    bare = nn.Linear(4, 2)
    slab = BufferSlab(bare)
    opt = FusedAdam(FlatBuffers(bare.parameters()), guard=True, guard_state=slab)
    opt._hyper_dev = torch.zeros(8)
    opt.step_dev()
    assert [c[0] for c in calls] == ["mpa_step_guard", "mpa_adam_step_guarded"]
