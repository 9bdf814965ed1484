"""Gradient accumulation without a device: the restatement `accum_ref` over hand-written windows (overflow, inf - inf,
denormals, -0), the argument refusals of mpa_grad_accumulate through `_lib`, header = `_lib.SIGNATURES`, the launches of a
trainer with the switch at 1 (the parent's) and at K = 3 (one accumulate launch per micro-batch, the tail once per window),
`grad_scale` of early-closed windows, the Python layer's refusals, the checkpoint's window, `fit` with stubs, the tool's
flag and the presets."""
import ctypes
import re

import numpy as np
import pytest
import torch

from multi_part_assembly_amd import _lib, accum_ref
from multi_part_assembly_amd.optim import FlatBuffers, GradAccumulator
from accumulate_cases import (OldStubTrainer, Sampler, WindowStubTrainer, accumulate_modes, host_launches, host_trainer,
                              tail)
from trainer_cases import StubProducer, bits_i32 as _bits, built, optimizer_presets, tiny_cfg  # noqa: F401
from tool_loader import load_tool as _tool

f32 = np.float32


def _words(*bits):
    return np.array(bits, dtype=np.uint32).view(f32)


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------
def test_the_three_modes_by_hand():
    g = np.array([1.0, -2.0, 0.5, 3.0], f32)
    a = np.array([10.0, 20.0, 30.0, 40.0], f32)
    grad, acc = accum_ref.accumulate(accum_ref.FIRST, g, a)
    assert _bits(grad).tolist() == _bits(g).tolist() and _bits(acc).tolist() == _bits(g).tolist()  # a copy: `a` is never read
    grad, acc = accum_ref.accumulate(accum_ref.ADD, g, a)
    assert grad.tolist() == g.tolist() and acc.tolist() == [11.0, 18.0, 30.5, 43.0]
    grad, acc = accum_ref.accumulate(accum_ref.LAST, g, a)
    assert grad.tolist() == [11.0, 18.0, 30.5, 43.0] and acc.tolist() == a.tolist()
    for mode in (3, -1, 7):  # what only a device word can hold: nothing is written
        grad, acc = accum_ref.accumulate(mode, g, a)
        assert grad.tolist() == g.tolist() and acc.tolist() == a.tolist()
    assert grad is not g and acc is not a and g.tolist() == [1.0, -2.0, 0.5, 3.0]  # new arrays, the inputs stay
    assert accum_ref.accumulate(accum_ref.ADD, g[:0], a[:0])[1].size == 0
    for bad in ((g[:3], a[:3]), (g, a[:0]), (g.astype(np.float64), a), (g.reshape(2, 2), a.reshape(2, 2))):
        with pytest.raises(ValueError):
            accum_ref.accumulate(accum_ref.ADD, *bad)


def test_overflow_inf_minus_inf_denormals_and_minus_zero():
    big, inf = f32(3e38), f32(np.inf)
    g0 = np.array([big, inf, big, 0.0], f32)
    g1 = np.array([big, -inf, -big, 0.0], f32)
    g2 = np.array([-big, 1.0, big, 0.0], f32)
    total = accum_ref.window_sum([g0, g1, g2])
    # 3e38 + 3e38 overflows to inf and stays there; inf - inf is a NaN and stays one; (3e38 - 3e38) + 3e38 is exact
    assert np.isposinf(total[0]) and np.isnan(total[1]) and total[2] == big and _bits(total)[3] == 0
    # denormals are neither flushed on the way in nor on the way out; the sum of two is exact
    tiny = _words(0x00000001, 0x00000003, 0x00400000, 0x807FFFFF)
    more = _words(0x00000001, 0x80000001, 0x00400000, 0x00000001)
    got = accum_ref.window_sum([tiny, more]).view(np.uint32).tolist()
    assert got == [0x00000002, 0x00000002, 0x00800000, 0x807FFFFE]
    # -0 + -0 = -0, -0 + +0 = +0 (round to nearest), and FIRST keeps the sign bit and NaN payloads as they are
    zeros = accum_ref.window_sum([_words(0x80000000, 0x80000000, 0, 0), _words(0x80000000, 0, 0x80000000, 0)])
    assert zeros.view(np.uint32).tolist() == [0x80000000, 0, 0, 0]
    payload = _words(0x7FC00001, 0xFFC12345, 0x80000000, 0x7FA00000)
    _, acc = accum_ref.accumulate(accum_ref.FIRST, payload, np.full(4, np.nan, f32))
    assert acc.view(np.uint32).tolist() == payload.view(np.uint32).tolist()


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_window_sum_is_the_chained_accumulate_calls(k):
    rng = np.random.RandomState(k)
    grads = [(rng.randn(64) * 10.0 ** rng.randint(-3, 4)).astype(f32) for _ in range(k)]
    modes = accum_ref.modes(k)
    assert modes == ([None] if k == 1 else [0] + [1] * (k - 2) + [2]) and len(modes) == k
    assert modes == [accum_ref.mode_at(j, j == k - 1) for j in range(k)]
    acc = np.full(64, np.nan, f32)  # whatever the accumulator held: FIRST never reads it
    for g, mode in zip(grads, modes):
        grad = g
        if mode is not None:
            grad, acc = accum_ref.accumulate(mode, g, acc)
    assert _bits(grad).tolist() == _bits(accum_ref.window_sum(grads)).tolist()
    by_hand = grads[0]
    for g in grads[1:]:
        by_hand = (by_hand + g).astype(f32)
    assert _bits(by_hand).tolist() == _bits(accum_ref.window_sum(grads)).tolist()
    with pytest.raises(ValueError):
        accum_ref.window_sum([])
    with pytest.raises(ValueError):
        accum_ref.modes(0)


# ---- 2. the boundary ---------------------------------------------------------------------------------------------------------
def test_header_prototype_is_the_table_entry_and_the_abi_number_stays():
    assert "mpa_grad_accumulate" in _lib.declared_functions() and sorted(_lib.SIGNATURES) == _lib.declared_functions()
    assert _lib.ABI_VERSION == 10
    P, I64, INT = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert _lib.SIGNATURES["mpa_grad_accumulate"] == (INT, [P, P, I64, INT, P, P])
    text = re.sub(r"/\*.*?\*/", "", _lib.HEADER_PATH.read_text(), flags=re.S)
    proto = re.search(r"int\s+mpa_grad_accumulate\s*\(([^)]*)\)\s*;", text).group(1)
    params = [" ".join(p.split()) for p in proto.split(",")]
    assert params == ["float* grad", "float* acc", "int64_t numel", "int mode", "const int32_t* mode_dev", "void* stream"]
    kinds = [P if "*" in p else I64 if p.startswith("int64_t") else INT for p in params]
    assert kinds == _lib.SIGNATURES["mpa_grad_accumulate"][1]
    assert "#define MPA_ABI_VERSION 10" in _lib.HEADER_PATH.read_text()


def test_argument_refusals_need_no_gpu(built):
    L, err = _lib.lib(), _lib.lib().mpa_last_error
    g, a, word = 4096, 8192, 4100  # addresses by alignment (never dereferenced: every call below launches nothing)

    def call(grad=g, acc=a, numel=64, mode=0, mode_dev=None):
        return L.mpa_grad_accumulate(grad, acc, numel, mode, mode_dev, None)

    assert call(numel=0) == 0 and call(None, None, 0) == 0 and call(None, None, 0, 0, word) == 0  # nothing to add
    for numel in (-4, -1, 3, 6, 65):
        assert call(numel=numel) == -1 and b"multiple of 4" in err(), numel
    for kw in (dict(grad=None), dict(acc=None), dict(grad=None, acc=None)):
        assert call(**kw) == -1 and b"null" in err(), kw
    for kw in (dict(grad=g + 4), dict(acc=a + 8), dict(grad=g + 12, acc=a + 12)):
        assert call(**kw) == -1 and b"16-byte aligned" in err(), kw
    for kw in (dict(acc=g), dict(acc=g + 16), dict(acc=g + 240), dict(grad=a + 128), dict(grad=a - 240)):
        assert call(**kw) == -1 and b"overlap" in err(), kw
    for mode in (-1, 3, 4, 1 << 20):
        assert call(mode=mode) == -1 and b"mode must be" in err(), mode
    for off in (1, 2, 3):
        assert call(mode_dev=word + off) == -1 and b"misaligned" in err(), off
        assert call(mode=7, mode_dev=word + off) == -1 and b"misaligned" in err(), off
    # refused whatever else is right, numel = 0 included
    assert call(None, None, 0, 5) == -1 and b"mode must be" in err()
    assert call(None, None, 0, 0, word + 2) == -1 and b"misaligned" in err()


# ---- 3. GradAccumulator on host tensors -----------------------------------------------------------------------------------------
def _flat(n=8):
    return FlatBuffers([torch.nn.Parameter(torch.zeros(n))])


def test_accumulator_follows_the_restatement_on_host_tensors():
    flat = _flat()
    acc = GradAccumulator(flat)
    assert acc.acc.shape == flat.flat_grad.shape and acc.acc.data_ptr() != flat.flat_grad.data_ptr()
    assert acc.mode_word.dtype == torch.int32 and acc.mode_word.tolist() == [GradAccumulator.IDLE] and acc.window == 0
    rng = np.random.RandomState(0)
    for sizes in ((3, 2, 1, 4), (1, 1), (2,)):  # the second window reuses the accumulator through FIRST
        for k in sizes:
            grads = [rng.randn(8).astype(f32) for _ in range(k)]
            acc.acc.fill_(float("nan"))
            for j, g in enumerate(grads):
                flat.flat_grad.copy_(torch.from_numpy(g))
                assert acc.window == j
                size = acc.add(closing=j == k - 1)
                assert size == (k if j == k - 1 else None)
            assert acc.window == 0
            assert _bits(flat.flat_grad.numpy()).tolist() == _bits(accum_ref.window_sum(grads)).tolist()
    flat.flat_grad.fill_(1.0)
    acc.add(False)
    assert acc.window == 1
    acc.drop()
    assert acc.window == 0


# ---- 4. the launches of a trainer -------------------------------------------------------------------------------------------------
CASES = [(False, False), (True, False), (True, True)]


@pytest.mark.parametrize("clip", [None, 1.0])
@pytest.mark.parametrize("decay", [None, 0.99])
@pytest.mark.parametrize("guard_step,guard_buffers", CASES)
def test_switch_at_one_gives_the_parents_launches(monkeypatch, built, guard_step, guard_buffers, decay, clip):
    calls = host_launches(monkeypatch)
    made = []
    for kw in ({}, {"accumulate": 1}):
        t = host_trainer(guard_step=guard_step, guard_buffers=guard_buffers, ema_decay=decay, **kw)
        t.optimizer.clip_grad = clip
        assert t.accumulate == 1 and t.accumulator is None and t.window == 0 and t.reducer.enabled
        per_step = []
        for k in range(3):
            calls.clear()
            t.train_step({"k": k}, close_window=(None, True, False)[k])  # (means nothing to this trainer)
            per_step.append([c[0] for c in calls])
            assert t.window == 0 and t.optimizer.step_count == k + 1 and t.optimizer.grad_scale == 1.0
        made.append(per_step)
    want = tail(guard_step, guard_buffers, clip, decay is not None)
    assert made[0] == made[1] == [want] * 3


@pytest.mark.parametrize("clip", [None, 1.0])
@pytest.mark.parametrize("decay", [None, 0.99])
@pytest.mark.parametrize("guard_step,guard_buffers", CASES)
def test_three_micro_batches_one_accumulate_launch_each_and_one_tail(monkeypatch, built, guard_step, guard_buffers, decay, clip):
    calls = host_launches(monkeypatch)
    t = host_trainer(grads=[1.0, 2.0, 4.0, 8.0, 16.0, 32.0], guard_step=guard_step, guard_buffers=guard_buffers,
                     ema_decay=decay, accumulate=3)
    t.optimizer.clip_grad = clip
    assert t.accumulate == 3 and t.window == 0 and not t.reducer.enabled
    want_tail = tail(guard_step, guard_buffers, clip, decay is not None)
    for window in range(2):
        for j in range(3):
            calls.clear()
            loss = t.train_step({"k": j})
            names = [c[0] for c in calls]
            assert float(loss) == 3 * window + j  # the micro-batch's own loss
            assert names[0] == "mpa_grad_accumulate" and accumulate_modes(calls) == [j]
            a = calls[0][1]
            assert a[0] is t.flat.flat_grad and a[1] is t.accumulator.acc and a[2] == t.flat.numel and a[4] is None and len(a) == 5
            assert names[1:] == (want_tail if j == 2 else []), (window, j)
            assert t.window == (j + 1) % 3 and t.optimizer.step_count == window + (j == 2)
        assert t.optimizer.grad_scale == 1.0 / 3
        # the flat gradient the tail saw: ((g0 + g1) + g2)
        assert t.flat.flat_grad.unique().tolist() == [7.0 * 8 ** window]
    assert t.micro_batches == 6


def test_early_closed_windows_scale_by_their_own_size_and_a_window_of_one_launches_nothing(monkeypatch, built):
    calls = host_launches(monkeypatch)
    t = host_trainer(grads=[1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0], accumulate=3)
    t.train_step({}, close_window=True)                      # a window closed at its first micro-batch
    assert [c[0] for c in calls] == ["mpa_adam_step_dev"] and t.optimizer.grad_scale == 1.0 and t.window == 0
    assert t.flat.flat_grad.unique().tolist() == [1.0]
    calls.clear()
    t.train_step({})
    t.train_step({}, close_window=True)                      # a window of two
    assert [c[0] for c in calls] == ["mpa_grad_accumulate", "mpa_grad_accumulate", "mpa_adam_step_dev"]
    assert accumulate_modes(calls) == [0, 2] and t.optimizer.grad_scale == 0.5 and t.window == 0
    assert t.flat.flat_grad.unique().tolist() == [6.0]
    calls.clear()
    for close in (None, False, None):                        # a full one: close_window=False does not keep it open
        t.train_step({}, close_window=close)
    assert accumulate_modes(calls) == [0, 1, 2] and t.optimizer.grad_scale == 1.0 / 3 and t.optimizer.step_count == 3
    assert t.flat.flat_grad.unique().tolist() == [56.0]
    calls.clear()
    t.train_step({}, close_window=True)
    assert [c[0] for c in calls] == ["mpa_adam_step_dev"] and t.optimizer.grad_scale == 1.0


def test_an_unguarded_trainer_drops_the_window_at_a_failed_launch_and_a_guarded_one_keeps_looking_away(monkeypatch, built):
    from multi_part_assembly_amd import trainer as trainer_mod
    host_launches(monkeypatch)
    looked = []

    def failing(device=None, synchronize=False):
        looked.append(synchronize)
        raise RuntimeError("gru: a launch of csrc/gru.hip gave up")

    t = host_trainer(accumulate=3)
    t.train_step({})
    assert t.window == 1
    monkeypatch.setattr(trainer_mod._gru, "raise_if_failed", failing)
    with pytest.raises(RuntimeError, match="gave up"):
        t.train_step({})
    assert t.window == 0 and t.optimizer.step_count == 0 and t._failed  # dropped: no later step applies the sum
    guarded = host_trainer(accumulate=3, guard_step=True)
    looked.clear()
    guarded.train_step({})
    guarded.train_step({})
    guarded.check_health()  # (what `fit` calls behind every micro-batch)
    assert looked == [] and guarded.window == 2  # the word stays raised until the window's verdict
    with pytest.raises(RuntimeError, match="gave up"):
        guarded.train_step({})  # the closing micro-batch: the tail looks, as a step does
    assert looked == [False] and guarded.window == 0


# ---- 5. the Python layer's refusals, the configuration key ------------------------------------------------------------------------
def test_argument_and_configuration():
    from multi_part_assembly_amd.pn_transformer import build_model
    from multi_part_assembly_amd.trainer import Trainer
    for bad in (0, -1, 2.5, 2.0, "2", True):
        with pytest.raises(ValueError, match="accumulate"):
            host_trainer(accumulate=bad)
    cfg = tiny_cfg()
    assert "accumulate_grad_batches" not in cfg.optimizer and Trainer(build_model(cfg), cfg).accumulate == 1
    cfg.optimizer.accumulate_grad_batches = 4
    assert Trainer(build_model(cfg), cfg).accumulate == 4
    assert Trainer(build_model(cfg), cfg, accumulate=2).accumulate == 2  # the argument wins
    cfg.optimizer.accumulate_grad_batches = 0
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        Trainer(build_model(cfg), cfg)
    presets = optimizer_presets()
    assert len(presets) >= 10 and all("accumulate_grad_batches" not in c.optimizer for c in presets)


# ---- 6. checkpoints ---------------------------------------------------------------------------------------------------------------
def test_checkpoint_carries_the_open_window(monkeypatch, built, tmp_path):
    host_launches(monkeypatch)
    plain = host_trainer()
    assert plain.state_dict()["accumulate"] == {"every": 1, "window": 0, "grad": None}
    t = host_trainer(grads=[1.0, 2.0, 4.0, 8.0], accumulate=3)
    assert t.state_dict()["accumulate"] == {"every": 3, "window": 0, "grad": None}
    t.train_step({})
    t.train_step({})
    state = t.state_dict()
    entry = state["accumulate"]
    assert set(entry) == {"every", "window", "grad"} and entry["every"] == 3 and entry["window"] == 2
    assert entry["grad"].unique().tolist() == [3.0] and entry["grad"].data_ptr() != t.accumulator.acc.data_ptr()  # a copy
    torch.save(state, tmp_path / "open.pt")
    state = torch.load(tmp_path / "open.pt", weights_only=False)
    other = host_trainer(grads=[4.0, 1.0, 1.0], accumulate=3)
    other.load_state_dict(state)
    assert other.window == 2 and torch.equal(other.accumulator.acc, t.accumulator.acc)
    other.train_step({})  # closes the loaded window: (1 + 2) + 4
    assert other.window == 0 and other.flat.flat_grad.unique().tolist() == [7.0] and other.optimizer.grad_scale == 1.0 / 3
    # an open window saved under another K is refused, and the trainer stays as it was
    for kw in ({"accumulate": 4}, {"accumulate": 2}, {}):
        wrong = host_trainer(**kw)
        before = wrong.flat.flat_param.clone()
        with pytest.raises(RuntimeError, match="open window of 2"):
            wrong.load_state_dict(state)
        assert wrong.window == 0 and torch.equal(wrong.flat.flat_param, before)
    # an empty window loads under any K; a missing key means an empty window
    other.load_state_dict(plain.state_dict())
    assert other.window == 0
    other.train_step({})
    assert other.window == 1
    other.load_state_dict({k: v for k, v in state.items() if k != "accumulate"})
    assert other.window == 0
    plain.load_state_dict(other.state_dict())
    other.train_step({})
    other.load_state_dict({"state_dict": state["model"]})  # Lightning-style: weights only, no window
    assert other.window == 0


# ---- 7. fit -----------------------------------------------------------------------------------------------------------------------
def test_fit_closes_the_window_on_each_epochs_last_batch_and_on_no_other():
    from multi_part_assembly_amd import fit as _fit
    t = WindowStubTrainer(2)
    records = []
    history = _fit.fit(t, StubProducer(), Sampler(3), epochs=2, log_every=1, on_log=records.append)
    assert t.calls == [(1, False), (2, False), (3, True)] * 2 and t.window == 0
    assert t.steps == 4  # optimiser steps: windows of 2 + 1 per epoch
    assert [r["step"] for r in records if "step" in r] == [1, 2, 3, 1, 2, 3]  # log_every counts micro-batches
    assert [h["train/loss"] for h in history] == [1.0, 1.0]
    # an epoch that is a multiple of K long: its last batch is passed closing all the same
    t = WindowStubTrainer(2)
    _fit.fit(t, StubProducer(), Sampler(4), epochs=1, log_every=0)
    assert t.calls == [(1, False), (2, False), (3, False), (4, True)] and t.steps == 2


def test_fit_calls_a_trainer_without_the_attribute_with_one_argument():
    from multi_part_assembly_amd import fit as _fit
    t = OldStubTrainer()
    _fit.fit(t, StubProducer(), Sampler(3), epochs=1, log_every=0)
    assert [(len(a), kw) for a, kw in t.calls] == [(1, {})] * 3
    one = WindowStubTrainer(1)  # the switch at 1: as before too
    one.train_step = lambda *a, **kw: (one.calls.append((a, kw)), torch.tensor(1.0))[1]
    _fit.fit(one, StubProducer(), Sampler(3), epochs=1, log_every=0)
    assert [(len(a), kw) for a, kw in one.calls] == [(1, {})] * 3


def test_fit_stopped_inside_a_window_writes_the_window(monkeypatch, built, tmp_path):
    from multi_part_assembly_amd import fit as _fit
    host_launches(monkeypatch)
    t = host_trainer(grads=[1.0, 2.0, 4.0, 8.0, 16.0, 32.0], accumulate=2)
    t.fit(StubProducer(), Sampler(3), epochs=2, log_every=0, ckpt_dir=str(tmp_path), max_steps=4)
    # micro-batches 1, 2 | 3 close windows in epoch 0; micro-batch 4 opens one in epoch 1 and the run stops there
    assert t.optimizer.step_count == 2 and t.window == 1
    state = torch.load(tmp_path / _fit.LAST, weights_only=False)
    assert state["accumulate"]["every"] == 2 and state["accumulate"]["window"] == 1
    assert state["accumulate"]["grad"].unique().tolist() == [8.0]
    assert state["fit"]["sampler"]["next_step"] == 1 and state["fit"]["next_epoch"] == 1
    fresh = host_trainer(grads=[16.0, 32.0], accumulate=2)
    assert fresh.resume(str(tmp_path)) == 1 and fresh.window == 1
    fresh.fit(StubProducer(), Sampler(3), epochs=2, log_every=0, ckpt_dir=str(tmp_path))
    assert fresh.window == 0 and fresh.optimizer.step_count == 4  # 2 loaded + (4, 5) + (6 alone)
    assert fresh.flat.flat_grad.unique().tolist() == [32.0]
    assert torch.load(tmp_path / _fit.LAST, weights_only=False)["accumulate"]["window"] == 0


# ---- 8. the tool ------------------------------------------------------------------------------------------------------------------
def test_train_tool_flag():
    tool = _tool("train")
    base = ["--preset", "pn_transformer_everyday", "--synthetic"]
    args = tool.parse_args(base)
    assert args.accumulate is None and "accumulate_grad_batches" not in tool.configure(args).optimizer
    assert tool.configure(tool.parse_args(base + ["--accumulate", "4"])).optimizer.accumulate_grad_batches == 4
    assert tool.configure(tool.parse_args(base + ["--accumulate", "1"])).optimizer.accumulate_grad_batches == 1
    for bad in (["--accumulate", "0"], ["--accumulate", "-2"], ["--accumulate", "2.5"], ["--accumulate"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)


def test_rate_tool_imports_by_path_and_measures_on_the_shared_rig():
    import os
    import sys
    from trainer_cases import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rate_rig as rig
    tool = _tool("accumulate_rate")
    assert callable(tool.main) and tool.rig is rig and tool.KS == (1, 2, 4)
    assert [(name, mode, per_param) for name, mode, per_param in tool.MODES] == [("first", 0, 8), ("add", 1, 12), ("last", 2, 12)]
    assert not any(hasattr(tool, name) for name in ("window", "_window", "alternate", "report"))  # no private rig
