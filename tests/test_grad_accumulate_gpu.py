"""Gradient accumulation on the device (csrc/grad_accumulate.hip: mpa_grad_accumulate; optim.GradAccumulator;
Trainer(accumulate=K)).

The kernel against the restatement `accum_ref`, bit for bit, on random bit patterns (NaNs, infinities and denormals among
them) between sentinel-filled guard zones, at the unit, wave, block and sweep boundaries of 2048 blocks x 256 lanes x 4
elements and at zero; by value and from the device word; eager and captured.  NaN results: IEEE 754 leaves the payload of
a NaN an addition PRODUCES to the implementation, so where the restatement gives a NaN the kernel must give a NaN, and
everywhere else the same 32 bits; bits the kernel only moves (FIRST, the buffer a mode does not write) are compared as
bits.

Then the trainer on pn_transformer and dgl at B = 2, P = 3, N = 64: a window of K micro-batches equals a hand-built twin
(one forward / backward per batch, `accum_ref.window_sum`, ONE Adam step with grad_scale = 1 / k), eager and captured;
K = 1 is the trainer without the argument; a poisoned micro-batch skips the whole window; checkpoints carry the open
window; two ranks issue one collective per window; one card with K = 2 takes the step of two ranks; the tool runs."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from multi_part_assembly_amd import _lib, accum_ref
from accumulate_cases import assert_same, loss_bits, state, twin_window
from trainer_cases import (ROOT, Zoned, batch as _batch, batches as _batches, i32, random_bytes as _random_bytes, rank_setup,
                           run_two_ranks, trainer as _trainer)

pytestmark = pytest.mark.gpu

SWEEP = accum_ref.BLOCKS * accum_ref.THREADS * 4  # elements one pass of the full grid covers
SIZES = [0, 4, 252, 256, 260, 1020, 1024, 1028, SWEEP - 4, SWEEP, SWEEP + 4]


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------
def _launch(dev, grad, acc, mode=0, word=None):
    _lib.launch("mpa_grad_accumulate", dev, grad.mid, acc.mid, grad.n // 4, mode, word)


def _assert_same_floats(got, want, what):
    """Byte arrays of float32 words: a NaN where the restatement has a NaN, the same 32 bits everywhere else."""
    g, w = got.view(np.uint32), want.view(np.uint32)
    nan = np.isnan(want.view(np.float32))
    assert np.array_equal(np.isnan(got.view(np.float32)), nan), what
    assert np.array_equal(g[~nan], w[~nan]), what


def test_sizes_are_the_boundaries_of_the_launch():
    assert SWEEP == 2097152 and SIZES[-3:] == [2097148, 2097152, 2097156]


@pytest.mark.parametrize("n", SIZES)
def test_kernel_equals_the_restatement_bit_for_bit(cuda_device, n):
    dev = cuda_device
    grad_h, acc_h = _random_bytes(4 * n, n % 89), _random_bytes(4 * n, n % 89 + 1)
    grad, acc = Zoned(grad_h, dev), Zoned(acc_h, dev)
    pristine = (grad.buf.clone(), acc.buf.clone())
    word = torch.zeros(1, dtype=torch.int32, device=dev)

    def run(mode, from_word):
        grad.buf.copy_(pristine[0]), acc.buf.copy_(pristine[1])
        if from_word:
            word.fill_(mode)
            _launch(dev, grad, acc, 1 if mode == 0 else 0, word)  # (the value is ignored beside a word)
        else:
            _launch(dev, grad, acc, mode)
        torch.cuda.synchronize()
        assert grad.zones_intact() and acc.zones_intact(), (n, mode, from_word)
        return grad.bytes().copy(), acc.bytes().copy()

    nans = 0
    for mode in (accum_ref.FIRST, accum_ref.ADD, accum_ref.LAST):
        want_grad, want_acc = accum_ref.accumulate(mode, grad_h.view(np.float32), acc_h.view(np.float32))
        nans += int(np.isnan(want_grad).sum()) + int(np.isnan(want_acc).sum())
        got = run(mode, False)
        if mode == accum_ref.LAST:
            _assert_same_floats(got[0], want_grad.view(np.uint8), (n, mode))
            assert got[1].tobytes() == acc_h.tobytes()    # the accumulator is read only
        else:
            _assert_same_floats(got[1], want_acc.view(np.uint8), (n, mode))
            assert got[0].tobytes() == grad_h.tobytes()   # the gradient is read only
        if mode == accum_ref.FIRST:
            assert got[1].tobytes() == grad_h.tobytes()   # a copy: NaN payloads, denormals and -0 as they are
        again, by_word = run(mode, False), run(mode, True)
        for other in (again, by_word):  # run to run, and by value = from the device word: every bit, NaN payloads included
            assert other[0].tobytes() == got[0].tobytes() and other[1].tobytes() == got[1].tobytes(), (n, mode)
    for idle in (3, -1):  # a word outside 0..2 writes nothing
        got = run(idle, True)
        assert got[0].tobytes() == grad_h.tobytes() and got[1].tobytes() == acc_h.tobytes(), (n, idle)
    assert int(word.item()) == -1  # the word is read only
    # FIRST over an accumulator full of NaN bits gives the gradient's bits
    acc.mid.view(torch.int32).fill_(0x7FC00000)
    grad.buf.copy_(pristine[0])
    _launch(dev, grad, acc, accum_ref.FIRST)
    torch.cuda.synchronize()
    assert acc.bytes().tobytes() == grad_h.tobytes() and acc.zones_intact()
    if n >= 1024:
        assert nans > 0  # the random bits did hold NaNs


def test_refusals_on_device_pointers_launch_nothing(cuda_device):
    dev = cuda_device
    grad, acc = Zoned(_random_bytes(1024, 1), dev), Zoned(_random_bytes(1024, 2), dev)
    before = (grad.buf.clone(), acc.buf.clone())
    for args, why in (((grad.mid[4:1012], acc.mid[:1008], 252, 0, None), "aligned"),
                      ((grad.mid, grad.mid[16:], 252, 0, None), "overlap"), ((grad.mid, None, 256, 0, None), "null"),
                      ((grad.mid, acc.mid, 255, 0, None), "multiple of 4"), ((grad.mid, acc.mid, 256, 3, None), "mode must be")):
        with pytest.raises(_lib.MpaError, match=why):
            _lib.launch("mpa_grad_accumulate", dev, *args)
    torch.cuda.synchronize()
    assert torch.equal(grad.buf, before[0]) and torch.equal(acc.buf, before[1])


def test_a_captured_launch_follows_the_device_word(cuda_device):
    dev = cuda_device
    n = 1024 + 12
    rng = np.random.RandomState(3)
    grads = [rng.randn(n).astype(np.float32) for _ in range(3)]
    nan = np.full(n, np.nan, np.float32).view(np.uint8)
    eager = (Zoned(grads[0].view(np.uint8), dev), Zoned(nan, dev))
    graph = (Zoned(grads[0].view(np.uint8), dev), Zoned(nan, dev))
    word = torch.full((1,), 3, dtype=torch.int32, device=dev)
    _launch(dev, graph[0], graph[1], 0, word)  # (idle: the code object loads outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        _launch(dev, graph[0], graph[1], 0, word)
    acc_want = nan.view(np.float32)
    for k, mode in enumerate((accum_ref.FIRST, accum_ref.ADD, accum_ref.LAST)):
        for pair in (eager, graph):
            pair[0].mid.copy_(torch.from_numpy(grads[k].view(np.uint8)))
        word.fill_(mode)
        g.replay()
        _launch(dev, eager[0], eager[1], mode)
        torch.cuda.synchronize()
        grad_want, acc_want = accum_ref.accumulate(mode, grads[k], acc_want)
        for pair in (graph, eager):
            assert pair[0].bytes().tobytes() == grad_want.tobytes() and pair[1].bytes().tobytes() == acc_want.tobytes(), (k, mode)
            assert pair[0].zones_intact() and pair[1].zones_intact()
    assert grad_want.tobytes() == accum_ref.window_sum(grads).tobytes()


# ---- 2. the trainer against a hand-built twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,use_graph", [("pn", False), ("pn", True), ("dgl", False), ("dgl", True)])
def test_windows_equal_a_hand_built_twin(cuda_device, family, use_graph):
    """graph: the first micro-batch is the eager warm-up, the second is captured and replayed, the others are replays.
    Windows of 3, 3 (the accumulator reused through FIRST) and an early-closed one of 2."""
    dev = cuda_device
    t = _trainer(dev, family, accumulate=3, use_graph=use_graph, graph_warmup=1)
    twin = _trainer(dev, family)
    assert t.accumulate == 3 and twin.accumulate == 1 and t.window == 0
    seed = 60
    for size, close in ((3, None), (3, None), (2, True)):
        window = [_batch(dev, seed + j) for j in range(size)]
        seed += size
        losses = []
        for j, b in enumerate(window):
            before = t.optimizer.step_count
            losses.append(t.train_step(b, close_window=close if j == size - 1 else None).clone())
            assert t.window == (j + 1) % size and t.optimizer.step_count == before + (j == size - 1)
        assert t.optimizer.grad_scale == 1.0 / size
        assert loss_bits(losses) == loss_bits(twin_window(twin, window))
        assert_same(state(t), state(twin), (family, use_graph, seed))
    assert state(t)["count"] == 3 and t.micro_batches == 8
    assert (t._graph is not None) == t.use_graph and t._graph_b is None
    if family == "pn":
        assert t.use_graph == use_graph
    counters = [b for name, b in t.model.named_buffers() if name.endswith("num_batches_tracked")]
    assert counters and all(int(c) == 8 for c in counters)  # BatchNorm moves per micro-batch


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_switch_at_one_is_the_trainer_without_the_argument(cuda_device, use_graph):
    dev = cuda_device
    one = _trainer(dev, accumulate=1, use_graph=use_graph, graph_warmup=1)
    plain = _trainer(dev, use_graph=use_graph, graph_warmup=1)
    for k in range(3):
        b = _batch(dev, 60 + k)
        a = one.train_step(b, close_window=(None, True, False)[k]).clone()
        assert loss_bits([a]) == loss_bits([plain.train_step(b).clone()])
        assert_same(state(one), state(plain), k)
    assert one.accumulator is None and (one._graph is not None) == use_graph and state(one)["count"] == 3


# ---- 3. the guard ----------------------------------------------------------------------------------------------------------------
def _average(t):
    torch.cuda.synchronize()
    return t.average.ema_param.cpu().numpy().tobytes(), t.average.ema_state.cpu().numpy().tobytes()


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("guard_buffers", [True, False], ids=["rollback", "no_rollback"])
def test_a_poisoned_micro_batch_skips_the_whole_window(cuda_device, guard_buffers, use_graph):
    dev = cuda_device
    kw = dict(accumulate=3, guard_step=True, guard_buffers=guard_buffers, ema_decay=0.9)
    t = _trainer(dev, use_graph=use_graph, graph_warmup=1, **kw)
    window, _ = _batches(dev)  # clean, poisoned (a NaN in part_trans), clean: ONE window
    before, average = state(t), _average(t)
    for b in window:
        t.train_step(b)
    after = state(t)
    assert t.window == 0 and t.optimizer.guard_words().tolist()[:4] == [1, 0, 1, 1]  # verdict, applied, skipped, in a row
    assert_same(after, before, "skipped", buffers=guard_buffers)  # parameters, moments and the count keep their bits
    assert _average(t) == average
    if not guard_buffers:  # without the rollback the statistics carry the window's three micro-batches
        assert any(not torch.equal(after["buffers"][k], before["buffers"][k]) for k in before["buffers"])
    clean = [_batch(dev, 63 + j) for j in range(3)]
    for b in clean:
        t.train_step(b)
    assert t.optimizer.guard_words().tolist()[:4] == [0, 1, 1, 0] and (t._graph is not None) == use_graph
    twin = _trainer(dev, **kw)  # never saw the skipped window
    for b in clean:
        twin.train_step(b)
    assert_same(state(t), state(twin), "the window behind the skipped one", buffers=guard_buffers)
    assert state(t)["count"] == 1
    if guard_buffers:
        assert _average(t) == _average(twin)
    else:
        assert _average(t)[0] == _average(twin)[0]
    t.state_dict()  # finite: not refused


# ---- 4. checkpoints ---------------------------------------------------------------------------------------------------------------
def test_a_checkpoint_with_an_open_window_continues_bit_equal(cuda_device, tmp_path):
    dev = cuda_device
    t = _trainer(dev, accumulate=3)
    data = [_batch(dev, 60 + j) for j in range(6)]
    for b in data[:2]:
        t.train_step(b)
    saved = t.state_dict()
    assert saved["accumulate"]["every"] == 3 and saved["accumulate"]["window"] == 2
    assert torch.equal(i32(saved["accumulate"]["grad"]), i32(t.accumulator.acc))
    torch.save(saved, tmp_path / "open.pt")
    fresh = _trainer(dev, accumulate=3)
    fresh.accumulator.acc.fill_(float("nan"))
    fresh.load_state_dict(torch.load(tmp_path / "open.pt", map_location=dev, weights_only=False))
    assert fresh.window == 2
    for b in data[2:]:
        t.train_step(b), fresh.train_step(b)
    assert t.window == fresh.window == 0 and state(t)["count"] == 2
    assert_same(state(fresh), state(t), "continued")
    with pytest.raises(RuntimeError, match="open window of 2"):
        _trainer(dev, accumulate=2).load_state_dict(saved)


def test_a_run_stopped_inside_a_window_and_resumed_equals_the_uninterrupted_run(cuda_device, tmp_path):
    from test_fit_gpu import Geometry, assert_same_state, sampler_for, state_of, trainer_for
    from multi_part_assembly_amd.sampler import EpochSampler
    setup, dev = Geometry(), cuda_device  # 3 micro-batches per epoch: windows of 2 + 1
    whole = trainer_for(setup, dev, accumulate=2)
    history = whole.fit(setup.producer(dev), sampler_for(setup, dev), log_every=0)
    assert whole.optimizer.step_count == 6 and whole.micro_batches == 9 and whole.window == 0
    first = trainer_for(setup, dev, accumulate=2)
    first.fit(setup.producer(dev), sampler_for(setup, dev), log_every=0, ckpt_dir=str(tmp_path), max_steps=4)
    assert first.window == 1 and first.optimizer.step_count == 2
    last = torch.load(tmp_path / "last.pt", weights_only=False)
    assert last["accumulate"]["window"] == 1 and last["accumulate"]["every"] == 2
    fresh = trainer_for(setup, dev, accumulate=2)
    assert fresh.resume(str(tmp_path)) == 1 and fresh.window == 1
    resumed = fresh.fit(setup.producer(dev), EpochSampler(setup.S, setup.B, seed=0, device=dev), log_every=0,
                        ckpt_dir=str(tmp_path))
    assert_same_state(state_of(fresh), state_of(whole))
    assert [h["epoch"] for h in resumed] == [h["epoch"] for h in history] == [0, 1, 2]
    assert fresh.optimizer.step_count == 6 and fresh.window == 0


# ---- 5. two ranks -----------------------------------------------------------------------------------------------------------------
def _rank_main(rank, port, out_dir):
    """One rank of the two-rank run (started as a program, under its own time limit)."""
    import torch.distributed as dist
    dev = rank_setup(rank, port)
    collectives = []
    real = dist.all_reduce

    def counted(tensor, *args, **kw):
        collectives.append(tensor.numel())
        return real(tensor, *args, **kw)

    dist.all_reduce = counted
    out = {}
    for guard in (False, True):  # K = 2: two windows on different shards
        t = _trainer(dev, accumulate=2, guard_step=guard)
        collectives.clear()
        per_micro = []
        for k in range(4):
            t.train_step(_batch(dev, 70 + 10 * k + rank))
            per_micro.append(len(collectives))
        out[guard] = {"state": state(t), "collectives": per_micro, "sizes": list(collectives), "numel": t.flat.numel,
                      "words": t.optimizer.guard_words().tolist() if guard else None}
    # what one card with accumulate = 2 stands in for: two ranks, one batch each per step, accumulate = 1
    t = _trainer(dev)
    for k in range(2):
        t.train_step(_batch(dev, 70 + 10 * k + rank))
    out["plain"] = state(t)
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks(cuda_device):
    return run_two_ranks(__file__, weights_only=False)


@pytest.mark.parametrize("guard", [False, True], ids=["unguarded", "guarded"])
def test_two_ranks_issue_one_collective_per_window_and_agree(two_ranks, guard):
    a, b = two_ranks[0][guard], two_ranks[1][guard]
    for rank in (a, b):
        assert rank["collectives"] == [0, 1, 1, 2]  # none behind a micro-batch that leaves its window open
        assert rank["sizes"] == [rank["numel"]] * 2  # the whole flat gradient, in one call
        assert rank["state"]["count"] == 2
    assert_same(a["state"], b["state"], "ranks", buffers=False)  # (each rank keeps its own statistics)
    if guard:
        assert a["words"][:4] == b["words"][:4] == [0, 2, 0, 0]


def test_one_card_with_two_micro_batches_takes_the_step_of_two_ranks(cuda_device, two_ranks):
    """The rig's pn model draws nothing per step (dropout off, noise_dim 0) and a sum of two floats does not depend on
    its order, so parameters and moments are equal bit for bit; the buffers are not compared (per-rank statistics)."""
    t = _trainer(cuda_device, accumulate=2)
    for k in range(2):
        for rank in range(2):
            t.train_step(_batch(cuda_device, 70 + 10 * k + rank))
    for rank in range(2):
        assert_same(state(t), two_ranks[rank]["plain"], f"rank {rank}", buffers=False)


# ---- 6. the tool ------------------------------------------------------------------------------------------------------------------
def test_train_tool_accumulates(cuda_device):
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "train.py"), "--synthetic",
                          "--preset", "pn_transformer_everyday", "--synthetic-shapes", "16", "--batch-size", "4",
                          "--accumulate", "2", "--epochs", "2", "--log-every", "1"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    done = re.search(r"done: 2 epochs in the history; (\d+) micro-batches in (\d+) optimiser steps", run.stdout)
    assert done is not None, run.stdout
    assert (int(done.group(1)), int(done.group(2))) == (8, 4)


if __name__ == "__main__":
    _rank_main(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3])
