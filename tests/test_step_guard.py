"""The guarded optimiser step without a device: the header and the signature table, the argument refusals, the numpy
restatement (`guard_ref`, the specification the kernels are tested against in tests/test_step_guard_gpu.py) over
hand-written sequences, the configuration key and the tool's flags, `fit`'s records / `skip_limit` / checkpoint round trip
with a stub trainer, and the launches `FusedAdam.step_dev` issues with the guard off (today's) and on."""
import ctypes

import numpy as np
import pytest
import torch

from multi_part_assembly_amd import _lib, fit as fit_mod, guard_ref
from multi_part_assembly_amd.optim import FlatBuffers, FusedAdam
from multi_part_assembly_amd.sampler import EpochSampler
from tool_loader import load_tool as _tool
from trainer_cases import StubProducer, StubTrainer, bits_i32 as _bits, built, optimizer_presets, record, tiny_cfg  # noqa: F401

NEW = ("mpa_step_guard_workspace", "mpa_step_guard", "mpa_adam_step_guarded", "mpa_guard_mark")


# ---- 1. the boundary ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_four_entry_points_and_the_abi_number_stays():
    declared = _lib.declared_functions()
    assert all(name in declared and name in _lib.SIGNATURES for name in NEW)
    assert sorted(_lib.SIGNATURES) == declared
    assert _lib.ABI_VERSION == 10
    P, I64, F32, INT = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_int
    assert _lib.SIGNATURES["mpa_step_guard"] == (INT, [P, I64, F32, P, F32, P, P, P, P, F32, F32, P])
    assert _lib.SIGNATURES["mpa_adam_step_guarded"] == (INT, [P, P, P, P, I64, P, F32, F32, F32, F32, INT, P, P, P])
    assert _lib.SIGNATURES["mpa_guard_mark"] == (INT, [P, P, I64, P])


def test_argument_refusals_need_no_gpu(built):
    L = _lib.lib()
    n = ctypes.c_int64()
    assert L.mpa_step_guard_workspace(ctypes.byref(n)) == 0 and n.value == guard_ref.BLOCKS * (8 + 4)
    assert L.mpa_step_guard_workspace(None) == -1 and b"null" in L.mpa_last_error()
    a16, a8, a4 = 4096, 4104, 4100  # addresses by alignment (never dereferenced: every call below is refused)
    guard = lambda *a: L.mpa_step_guard(*a, 0.9, 0.999, None)  # noqa: E731
    assert guard(a16, -1, 1.0, None, 1.0, None, a8, a4, a4) == -1 and b"numel" in L.mpa_last_error()
    assert guard(a16, 1 << 31, 1.0, None, 1.0, None, a8, a4, a4) == -1 and b"2^31" in L.mpa_last_error()
    assert guard(None, 4, 1.0, None, 1.0, None, a8, a4, a4) == -1 and b"null" in L.mpa_last_error()
    assert guard(a16, 4, 1.0, None, 1.0, None, None, a4, a4) == -1 and b"null" in L.mpa_last_error()
    assert guard(a16, 4, 1.0, None, 1.0, None, a8, None, a4) == -1 and b"null" in L.mpa_last_error()
    assert guard(a16, 4, 1.0, None, 1.0, None, a8, a4, None) == -1 and b"null" in L.mpa_last_error()
    assert guard(a8, 4, 1.0, None, 1.0, None, a8, a4, a4) == -1 and b"misaligned" in L.mpa_last_error()
    assert guard(a16, 4, 1.0, None, 1.0, None, a4, a4, a4) == -1 and b"misaligned" in L.mpa_last_error()
    assert guard(a16, 4, 1.0, None, 1.0, a4 + 1, a8, a4, a4) == -1 and b"misaligned" in L.mpa_last_error()
    assert guard(a16, 4, 1.0, None, 1.0, None, a8, a4 + 2, a4) == -1 and b"misaligned" in L.mpa_last_error()
    upd = lambda *a: L.mpa_adam_step_guarded(*a, None)  # noqa: E731
    assert upd(a16, a16, a16, a16, -1, a4, 0.9, 0.999, 1e-8, 0.0, 0, None, a4) == -1 and b"numel" in L.mpa_last_error()
    assert upd(None, None, None, None, 0, None, 0.9, 0.999, 1e-8, 0.0, 0, None, None) == 0  # nothing to update
    assert upd(a16, a16, a16, a16, 4, a4, 0.9, 0.999, 1e-8, 0.0, 0, None, None) == -1 and b"null" in L.mpa_last_error()
    assert upd(a16, a16, a16, a16, 4, None, 0.9, 0.999, 1e-8, 0.0, 0, None, a4) == -1 and b"null" in L.mpa_last_error()
    assert upd(a16, a8, a16, a16, 4, a4, 0.9, 0.999, 1e-8, 0.0, 0, None, a4) == -1 and b"aligned" in L.mpa_last_error()
    assert upd(a16, a16, a16, a16, 4, a4, 0.9, 0.999, 1e-8, 0.0, 0, None, a4 + 2) == -1 and b"misaligned" in L.mpa_last_error()
    assert L.mpa_guard_mark(a4, a4, 0, None) == -1 and b"numel" in L.mpa_last_error()
    assert L.mpa_guard_mark(None, a4, 4, None) == -1 and b"null" in L.mpa_last_error()
    assert L.mpa_guard_mark(a4, None, 4, None) == -1 and b"null" in L.mpa_last_error()
    assert L.mpa_guard_mark(a4 + 1, a4, 4, None) == -1 and b"misaligned" in L.mpa_last_error()


# ---- 2. the restatement ------------------------------------------------------------------------------------------------------
def _grad(n, seed=0):
    return np.random.RandomState(seed).randn(n).astype(np.float32)


def test_reference_words_over_a_hand_written_sequence():
    """apply, skip (NaN at 7), skip (-inf at 2 and +inf at 9), apply, status-only skip, apply."""
    hyper, words = guard_ref.new_hyper(), np.zeros(8, dtype=np.int32)
    clean = _grad(11)
    nan7 = clean.copy()
    nan7[7] = np.nan
    two = clean.copy()
    two[9], two[2] = np.inf, -np.inf
    seq = [(clean, None), (nan7, 0), (two, None), (clean, 0), (clean, 5), (clean, 0)]
    want = [  # verdict applied skipped in-a-row first-bad attempt or reserved
        [0, 1, 0, 0, 0, 0, 0, 0],
        [1, 1, 1, 1, 7, 2, 1, 0],
        [1, 1, 2, 2, 2, 3, 1, 0],
        [0, 2, 2, 0, 2, 3, 1, 0],
        [2, 2, 3, 1, -1, 5, 3, 0],
        [0, 3, 3, 0, -1, 5, 3, 0],
    ]
    steps = [1, 1, 1, 2, 2, 3]
    for (g, status), w, step in zip(seq, want, steps):
        before = _bits(hyper)
        verdict = guard_ref.step_guard(g, 0.0, 1.0, status, hyper, words)
        assert words.tolist() == w and verdict == w[0]
        assert int(hyper[4:5].view(np.int32)[0]) == step
        if verdict:  # the step count and both bias corrections keep their bits
            assert np.array_equal(_bits(hyper)[[1, 2, 4]], before[[1, 2, 4]])
        else:
            assert np.array_equal(_bits(hyper)[[1, 2]], _bits(guard_ref.new_hyper(step=step))[[1, 2]])
    assert guard_ref.describe(words) == dict(zip(guard_ref.WORDS, want[-1]))


def test_reference_sum_follows_the_two_stage_order_and_is_close_to_the_plain_sum():
    for n in (0, 1, 3, 4, 5, 1023, 1025, 524291):
        g = _grad(n, seed=n)
        s = guard_ref.sum_of_squares(g)
        assert s == pytest.approx(float((g.astype(np.float64) ** 2).sum()), rel=1e-13)
    # order: 8 elements = two float4 of threads 0 and 1; the tree adds thread 1's term to thread 0's
    g = np.float32([1e8, 1, 1, 1, 1, 1, 1, 1e-8])
    t0 = ((np.float64(1e16) + 1) + 1) + 1
    t1 = ((np.float64(1) + 1) + 1) + np.float64(np.float32(1e-8)) ** 2
    assert guard_ref.sum_of_squares(g) == t0 + t1


@pytest.mark.parametrize("n", [1, 4, 7, 1025])
def test_reference_extremes_do_not_trip_and_every_nonfinite_position_does(n):
    hyper, words = guard_ref.new_hyper(), np.zeros(8, dtype=np.int32)
    big = np.full(n, 3e38, dtype=np.float32)
    big[::2] *= -1
    assert guard_ref.step_guard(big, 0.0, 1.0, None, hyper, words) == 0  # (the NORM may exceed a float: not a verdict)
    assert words.tolist() == [0, 1, 0, 0, 0, 0, 0, 0] and hyper[5] == 1.0
    tiny = np.full(n, 1e-45, dtype=np.float32)  # denormals
    assert guard_ref.step_guard(tiny, 0.0, 1.0, None, hyper, words) == 0
    for bad in (np.nan, np.inf, -np.inf):
        for pos in range(n) if n <= 7 else (0, 1, 511, 1020, 1023, 1024):
            g = _grad(n)
            g[pos] = bad
            words[:] = 0
            assert guard_ref.step_guard(g, 1.0, 1.0, None, hyper, words) == guard_ref.NONFINITE
            assert words[4] == pos and hyper[5] == 1.0 and np.isposinf(hyper[6])


def test_reference_coefficient_and_empty_gradient():
    g = np.float32([3, 4, 0, 0, 12])  # norm 13
    hyper, words = guard_ref.new_hyper(), np.zeros(8, dtype=np.int32)
    guard_ref.step_guard(g, 6.5, 1.0, None, hyper, words)
    assert hyper[6] == 13.0 and hyper[5] == np.float32(6.5 / (13.0 + 1e-6))
    guard_ref.step_guard(g, 20.0, 1.0, None, hyper, words)  # within the bound: no clipping
    assert hyper[6] == 13.0 and hyper[5] == 1.0
    guard_ref.step_guard(g, 6.5, 0.5, None, hyper, words)   # the norm is the SCALED gradient's
    assert hyper[6] == 6.5 and hyper[5] == np.float32(6.5 / (6.5 + 1e-6))
    for off in (0.0, -1.0):
        guard_ref.step_guard(g, off, 1.0, None, hyper, words)
        assert hyper[6] == 13.0 and hyper[5] == 1.0
    empty = np.zeros(0, dtype=np.float32)
    assert guard_ref.step_guard(empty, 1.0, 1.0, None, hyper, words) == 0
    assert guard_ref.step_guard(empty, 1.0, 1.0, 0, hyper, words) == 0
    assert guard_ref.step_guard(empty, 1.0, 1.0, 1, hyper, words) == guard_ref.LAUNCH_FAILED and words[4] == -1


def test_reference_skipped_update_is_the_identity_and_an_applied_one_is_adam():
    rng = np.random.RandomState(3)
    p, m, v = (rng.randint(-2 ** 31, 2 ** 31 - 1, size=9, dtype=np.int64).astype(np.int32).view(np.float32) for _ in range(3))
    g = _grad(9)
    hyper, words = guard_ref.new_hyper(), np.zeros(8, dtype=np.int32)
    words[0] = 1
    before = [_bits(x) for x in (p, m, v, hyper)]
    guard_ref.adam_step_guarded(p, g, m, v, hyper, words, weight_decay=0.1, decoupled=True)
    assert all(np.array_equal(_bits(x), b) for x, b in zip((p, m, v, hyper), before))
    # one applied step from zero moments against torch.optim.Adam
    p = _grad(9, seed=5)
    m, v = np.zeros_like(p), np.zeros_like(p)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    tp.grad = torch.from_numpy(g.copy())
    torch.optim.Adam([tp], lr=1e-3).step()
    assert guard_ref.step_guard(g, 0.0, 1.0, None, hyper, words) == 0
    guard_ref.adam_step_guarded(p, g, m, v, hyper, words)
    assert np.allclose(p, tp.detach().numpy(), rtol=0, atol=1e-7)
    marked = g.copy()
    guard_ref.guard_mark(0, marked)
    assert np.array_equal(_bits(marked), _bits(g))
    guard_ref.guard_mark(3, marked)
    assert np.isnan(marked[0]) and np.array_equal(_bits(marked)[1:], _bits(g)[1:])


# ---- 3. configuration and tool ---------------------------------------------------------------------------------------------
def test_no_preset_sets_the_key_and_it_reads_false_by_default():
    cfgs = optimizer_presets()
    assert len(cfgs) >= 10
    for cfg in cfgs:
        assert "skip_nonfinite" not in cfg.optimizer
        assert cfg.optimizer.get("skip_nonfinite", False) is False


def test_train_tool_flags():
    tool = _tool("train")
    base = ["--preset", "pn_transformer_everyday", "--synthetic"]
    args = tool.parse_args(base)
    assert args.skip_nonfinite is False and args.skip_limit == -1
    assert "skip_nonfinite" not in tool.configure(args).optimizer
    args = tool.parse_args(base + ["--skip-nonfinite", "--skip-limit", "7"])
    assert args.skip_nonfinite is True and args.skip_limit == 7
    assert tool.configure(args).optimizer.skip_nonfinite is True
    with pytest.raises(SystemExit):
        tool.parse_args(base + ["--skip-limit", "7"])


def test_trainer_reads_the_key_with_a_default():
    from multi_part_assembly_amd.pn_transformer import build_model
    from multi_part_assembly_amd.trainer import Trainer
    cfg = tiny_cfg()
    off = Trainer(build_model(cfg), cfg)
    assert off.guard_step is False and off.optimizer.guard is False and off.reducer.before_reduce is None
    cfg.optimizer.skip_nonfinite = True
    on = Trainer(build_model(cfg), cfg)
    assert on.guard_step is True and on.optimizer.guard is True
    assert Trainer(build_model(cfg), cfg, guard_step=False).guard_step is False  # the argument wins


# ---- 4. fit with a stub trainer ---------------------------------------------------------------------------------------------
def test_fit_records_carry_the_guard_figures(tmp_path):
    trainer, logged = StubTrainer(skip={2, 3, 5}), []
    fit_mod.fit(trainer, StubProducer(), EpochSampler(12, 2, device="cpu"), epochs=1, log_every=2, on_log=logged.append,
                ckpt_dir=str(tmp_path))
    steps = [r for r in logged if "step" in r]
    assert [set(r) for r in steps] == [{"epoch", "step", "lr", "train/loss", "grad_norm", "skipped", "skipped_in_a_row"}] * 3
    assert [(r["grad_norm"], r["skipped"], r["skipped_in_a_row"]) for r in steps] == [(float("inf"), 1, 1), (4.0, 2, 0),
                                                                                      (6.0, 3, 0)]
    assert all(type(r["skipped"]) is int and type(r["grad_norm"]) is float for r in steps)
    # the words survive the checkpoint: a fresh trainer resumes with them
    fresh = StubTrainer(skip=())  # (an empty script: guarded, no step skipped; without `skip` the stub is unguarded)
    assert fit_mod.resume(fresh, str(tmp_path)) == 1
    assert fresh.optimizer.words.tolist() == [0, 3, 3, 0, 0, 0, 0, 0]


def test_an_unguarded_trainer_keeps_the_record_keys_and_refuses_a_skip_limit():
    trainer, logged = StubTrainer(skip=()), []  # (built guarded, as above; switched off on the next line)
    trainer.guard_step = False
    fit_mod.fit(trainer, StubProducer(), EpochSampler(4, 2, device="cpu"), epochs=1, log_every=1, on_log=logged.append)
    assert [set(r) for r in logged if "step" in r] == [{"epoch", "step", "lr", "train/loss"}] * 2
    with pytest.raises(ValueError, match="skip_limit"):
        fit_mod.fit(trainer, StubProducer(), EpochSampler(4, 2, device="cpu"), epochs=1, skip_limit=2)


def test_skip_limit_raises_at_the_log_read_with_the_report():
    trainer = StubTrainer(skip={3, 4, 5, 6})
    with pytest.raises(RuntimeError, match=r"3 optimiser steps skipped in a row \(skip_limit 3\).*stub report: 3 skipped"):
        fit_mod.fit(trainer, StubProducer(), EpochSampler(20, 2, device="cpu"), epochs=1, log_every=1, skip_limit=3)
    assert trainer.steps == 5  # two applied, then the third skip in a row stops the run
    quiet = StubTrainer(skip={3, 4, 6, 7})  # never three in a row
    fit_mod.fit(quiet, StubProducer(), EpochSampler(20, 2, device="cpu"), epochs=1, log_every=1, skip_limit=3)
    assert quiet.steps == 10


def test_fused_adam_state_carries_the_words_and_loads_checkpoints_without_them():
    params = [torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(2, 3))]
    opt = FusedAdam(FlatBuffers(params), guard=True)
    opt.guard_words().copy_(torch.tensor([1, 4, 2, 1, 6, 6, 1, 0], dtype=torch.int32))
    state = opt.state_dict()
    assert state["guard"].tolist() == [1, 4, 2, 1, 6, 6, 1, 0]
    fresh = FusedAdam(FlatBuffers([torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(2, 3))]), guard=True)
    fresh.load_state_dict(state)
    assert fresh.guard_words().tolist() == [1, 4, 2, 1, 6, 6, 1, 0]
    old = {k: v for k, v in state.items() if k != "guard"}
    fresh.load_state_dict(old)
    assert fresh.guard_words().tolist() == [0] * 8
    plain = FusedAdam(FlatBuffers([torch.nn.Parameter(torch.zeros(5))]))
    assert "guard" not in plain.state_dict()
    with pytest.raises(RuntimeError, match="guard=False"):
        plain.guard_words()


def test_guard_report_names_the_owning_parameter():
    params = [torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(2, 3)), torch.nn.Parameter(torch.zeros(1))]
    opt = FusedAdam(FlatBuffers(params), guard=True)  # offsets 0, 8, 16 (every tensor starts 16-byte aligned)
    assert opt.flat.offsets == [0, 8, 16]
    assert opt.guard_report()["text"] == "0 steps applied, none skipped"
    opt.guard_words().copy_(torch.tensor([1, 4, 2, 1, 11, 6, 1, 0], dtype=torch.int32))
    rep = opt.guard_report()
    assert (rep["parameter"], rep["shape"], rep["element"]) == (1, (2, 3), 3)
    assert "parameter 1" in rep["text"] and "flat index 11" in rep["text"] and "2 skipped" in rep["text"]
    opt.guard_words().copy_(torch.tensor([2, 4, 3, 1, -1, 7, 3, 0], dtype=torch.int32))
    rep = opt.guard_report()
    assert rep["parameter"] is None and "status word alone" in rep["text"]


# ---- 5. the launches of a step --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [None, 1.0])
def test_step_dev_launches_with_the_guard_off_are_todays(monkeypatch, built, clip):
    """Recorded on a stub `_lib.launch` (host tensors, nothing runs): guard off = the launches and arguments of before;
    guard on = pass + verdict in front of the guarded update, the status word passed through."""
    calls = record(monkeypatch)
    params = [torch.nn.Parameter(torch.zeros(6))]
    status = torch.zeros(1, dtype=torch.int32)
    for guard in (False, True):
        opt = FusedAdam(FlatBuffers(params), clip_grad=clip, weight_decay=0.01, guard=guard, launch_status=status)
        opt._hyper_dev = torch.zeros(8)  # (the device buffer of a real step)
        calls.clear()
        opt.step_dev()
        names = [c[0] for c in calls]
        if guard:
            assert names == ["mpa_step_guard", "mpa_adam_step_guarded"]
            g = calls[0][1]
            assert g[0] is opt.flat_grad and g[1] == 8 and g[2] == (clip or 0.0) and g[5] is status
            assert g[3] == opt._hyper_dev.data_ptr() + 12 and g[7] is opt._hyper_dev and g[8] is opt.guard_words()
            assert calls[1][1][-1] is opt.guard_words()
        else:
            assert names == (["mpa_grad_clip_coef"] if clip else []) + ["mpa_adam_step_dev"]
            upd = calls[-1][1]
            assert upd[:5] == (opt.flat_param, opt.flat_grad, opt.exp_avg, opt.exp_avg_sq, 8) and upd[5] is opt._hyper_dev
            assert upd[6:] == (0.9, 0.999, 1e-8, 0.01, 1, None)
            if clip:
                c = calls[0][1]
                assert c[:3] == (opt.flat_grad, 8, 1.0) and c[3] == opt._hyper_dev.data_ptr() + 12
                assert c[4] == 1.0 and c[6] == opt._hyper_dev.data_ptr() + 20
