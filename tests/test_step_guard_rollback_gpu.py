"""Buffer rollback of the guarded step on the device (csrc/adam.hip: mpa_guard_commit; optim.BufferSlab;
Trainer(guard_buffers=True)).

Kernel against `guard_ref.commit`, bit for bit as int32 words, over the sizes at which the copy changes its path (one
unit, both sides of a wave, of the 256-thread block and of the 512 x 256 grid-stride sweep), for the verdict words 0..3,
on random bits between sentinel-filled guard zones; a captured launch replayed while the verdict word is rewritten.
Then the trainer: a poisoned batch between two clean ones leaves EVERY buffer, the parameters, both moments and the step
count equal to those of a twin that never saw the batch, eager and captured, for two model families — and not so with
the switch off; a statistic that went non-finite in a skipped step is undone; a raised status word rolls back; a loaded
checkpoint is what a skipped step returns to; two gloo ranks roll back their own statistics on the common verdict."""
import os
import sys

import numpy as np
import pytest
import torch

from multi_part_assembly_amd import _lib, guard_ref
from trainer_cases import (BT, NT, PT, Zoned, batches as _batches, buffers as _buffers, opt_state, random_bytes as _random_bytes,
                           rank_setup, run_two_ranks, trainer as _trainer, u8 as _bits)

pytestmark = pytest.mark.gpu

UNIT = guard_ref.COMMIT_UNIT
BLOCK = guard_ref.THREADS * UNIT                  # bytes one block copies per sweep
SWEEP = guard_ref.COMMIT_BLOCKS * BLOCK           # bytes one sweep of the full grid covers
SIZES = [16, 32, 16 * 63, 16 * 64, 16 * 65, BLOCK - UNIT, BLOCK, BLOCK + UNIT, SWEEP - UNIT, SWEEP, SWEEP + UNIT,
         2 * SWEEP + BLOCK + UNIT]


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------
def _commit(dev, word, live, shadow, n):
    _lib.launch("mpa_guard_commit", dev, word, live, shadow, n)


@pytest.mark.parametrize("n", SIZES)
def test_commit_equals_the_restatement_bit_for_bit(cuda_device, n):
    live_h, shadow_h = _random_bytes(n, n % 89), _random_bytes(n, n % 89 + 1)
    word = torch.zeros(8, dtype=torch.int32, device=cuda_device)
    for verdict in (0, 1, 2, 3):
        want_live, want_shadow = guard_ref.commit(verdict, live_h, shadow_h)
        word[0] = verdict
        runs = []
        for _ in range(2):
            live, shadow = Zoned(live_h, cuda_device), Zoned(shadow_h, cuda_device)
            _commit(cuda_device, word, live.mid, shadow.mid, n)
            torch.cuda.synchronize()
            got = (live.words(), shadow.words())
            assert np.array_equal(got[0], want_live.view(np.int32)), (n, verdict, "live")
            assert np.array_equal(got[1], want_shadow.view(np.int32)), (n, verdict, "shadow")
            assert live.zones_intact() and shadow.zones_intact(), (n, verdict)
            runs.append(got)
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
        assert int(word[0].item()) == verdict  # the verdict word is read only


def test_commit_of_zero_bytes_succeeds_without_a_launch_and_touches_nothing(cuda_device):
    word = torch.ones(8, dtype=torch.int32, device=cuda_device)
    host = _random_bytes(64, 3)
    live, shadow = Zoned(host, cuda_device), Zoned(_random_bytes(64, 4), cuda_device)
    before = (live.buf.clone(), shadow.buf.clone())
    _commit(cuda_device, word, None, None, 0)              # NULL ranges
    _commit(cuda_device, word, live.mid, shadow.mid, 0)  # and real ones
    torch.cuda.synchronize()
    assert torch.equal(live.buf, before[0]) and torch.equal(shadow.buf, before[1])
    # refusals on real device pointers: nothing is launched, nothing is written
    for args, why in (((live.mid[8:], shadow.mid, 16), "aligned"), ((live.mid, live.mid[16:], 32), "overlap"),
                      ((live.mid, shadow.mid, 24), "multiple of 16"), ((live.mid, None, 16), "null")):
        with pytest.raises(_lib.MpaError, match=why):
            _commit(cuda_device, word, *args)
    with pytest.raises(_lib.MpaError, match="null"):
        _commit(cuda_device, None, live.mid, shadow.mid, 16)
    torch.cuda.synchronize()
    assert torch.equal(live.buf, before[0]) and torch.equal(shadow.buf, before[1])


def test_a_captured_commit_takes_the_direction_of_the_word_at_each_replay(cuda_device):
    n = BLOCK + 3 * UNIT
    start = _random_bytes(n, 11)
    forwards = [_random_bytes(n, 20 + k) for k in range(3)]  # what each step's forward leaves in the live slab
    word = torch.zeros(8, dtype=torch.int32, device=cuda_device)
    eager = (Zoned(start, cuda_device), Zoned(start, cuda_device))
    graph = (Zoned(start, cuda_device), Zoned(start, cuda_device))
    _commit(cuda_device, word, eager[0].mid, eager[1].mid, n)  # (the code object loads outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        _commit(cuda_device, word, graph[0].mid, graph[1].mid, n)
    ref_live, ref_shadow = start.copy(), start.copy()
    for fwd, verdict in zip(forwards, (0, 1, 0)):
        word[0] = verdict
        for live, _ in (eager, graph):
            live.mid.copy_(torch.from_numpy(fwd))
        g.replay()
        _commit(cuda_device, word, eager[0].mid, eager[1].mid, n)
        torch.cuda.synchronize()
        ref_live, ref_shadow = guard_ref.commit(verdict, fwd, ref_shadow)
        for k, want in enumerate((ref_live, ref_shadow)):
            assert np.array_equal(graph[k].words(), want.view(np.int32)), (verdict, k)
            assert np.array_equal(eager[k].words(), graph[k].words())
            assert graph[k].zones_intact()
    assert np.array_equal(ref_live, forwards[2]) and np.array_equal(ref_shadow, forwards[2])


# ---- 2. the trainer -------------------------------------------------------------------------------------------------------------
def _opt_state(trainer):
    return opt_state(trainer, _bits)  # (bytes)


def _assert_buffers_equal(got, want, what=""):
    assert list(got) == list(want) and len(got) > 0
    for name in want:
        assert torch.equal(got[name], want[name]), (what, name)


def _counters(trainer):
    return [int(b) for n, b in trainer.model.named_buffers() if n.endswith("num_batches_tracked")]


def _make_twin(dev, family):
    """An unguarded trainer that takes the first and the third step ONLY: it never sees the second batch."""
    (b1, _, b3), _ = _batches(dev)
    t = _trainer(dev, family)
    t.train_step(b1)
    t.train_step(b3)
    assert set(_counters(t)) == {2}
    return {"buffers": _buffers(t), "opt": _opt_state(t)}


@pytest.fixture(scope="module")
def twin(cuda_device):
    return _make_twin(cuda_device, "pn")


def _assert_equals_twin(t, twin):
    state, step = _opt_state(t)
    assert step == 2 == twin["opt"][1]
    for name, x, y in zip(("parameters", "exp_avg", "exp_avg_sq"), state, twin["opt"][0]):
        assert torch.equal(x, y), name
    _assert_buffers_equal(_buffers(t), twin["buffers"])
    counters = _counters(t)
    assert len(counters) >= 5 and set(counters) == {2}
    assert all(b.dtype == torch.int64 for n, b in t.model.named_buffers() if n.endswith("num_batches_tracked"))


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_a_skipped_step_leaves_the_whole_model_equal_to_a_twin_that_never_saw_the_batch(cuda_device, twin, use_graph):
    batches, _ = _batches(cuda_device)
    # graph: the first step is the eager warm-up step, the poisoned one is captured and replayed, the third is a replay
    t = _trainer(cuda_device, guard_step=True, guard_buffers=True, use_graph=use_graph, graph_warmup=1)
    for b in batches:
        loss = t.train_step(b)
    assert use_graph == (t._graph is not None)
    _assert_equals_twin(t, twin)
    assert bool(torch.isfinite(loss))
    assert t.optimizer.guard_words().tolist()[:4] == [0, 2, 1, 0]
    slab = t.buffer_slab
    assert slab.nbytes > 0 and torch.equal(slab.shadow, slab.live)  # the third step was committed
    slab.check()
    t.state_dict()


def test_control_without_the_switch_the_skipped_batch_stays_in_the_buffers(cuda_device, twin):
    """The same sequence with guard_buffers=False: optimiser state equals the twin's (training-mode BatchNorm uses batch
    statistics), the running statistics carry batch 2 and the counters read 3 — the positive assertions above fail."""
    batches, _ = _batches(cuda_device)
    t = _trainer(cuda_device, guard_step=True, guard_buffers=False)
    assert t.buffer_slab is None
    for b in batches:
        t.train_step(b)
    state, step = _opt_state(t)
    assert step == 2 and all(torch.equal(x, y) for x, y in zip(state, twin["opt"][0]))
    got = _buffers(t)
    assert set(_counters(t)) == {3}
    stats = [n for n in got if n.endswith("running_mean") or n.endswith("running_var")]
    assert stats and all(not torch.equal(got[n], twin["buffers"][n]) for n in stats)
    with pytest.raises(AssertionError):
        _assert_equals_twin(t, twin)


def _poison_statistics_after_encoder(t, armed):
    """The part encoder's BatchNorm layers are parameter holders: the fused encoder kernel updates their running
    statistics, and no sub-module's `forward` runs, so a forward hook on one of them would never fire.  The encoder's own
    entry is wrapped instead: right behind it (that is, right behind the layer's forward and its statistics update) a
    hand-written device store puts a NaN into element 0 of one layer's running_mean, while `armed` holds True."""
    enc = t.model.encoder
    name, buf = next((n, b) for n, b in t.model.named_buffers() if n.endswith("running_mean"))
    inner = enc.forward_parts

    def forward_parts(*args, **kw):
        out = inner(*args, **kw)
        if armed[0]:
            buf[0] = float("nan")
        return out

    enc.forward_parts = forward_parts
    return name, buf


@pytest.mark.parametrize("guard_buffers", [True, False], ids=["rollback", "control"])
def test_a_statistic_that_went_nonfinite_in_the_skipped_step(cuda_device, guard_buffers):
    from multi_part_assembly_amd import synthetic
    batches, _ = _batches(cuda_device)
    t = _trainer(cuda_device, guard_step=True, guard_buffers=guard_buffers)
    armed = [False]
    name, buf = _poison_statistics_after_encoder(t, armed)
    t.train_step(batches[0])
    before = _buffers(t)
    armed[0] = True
    t.train_step(batches[1])
    armed[0] = False
    assert t.optimizer.guard_words().tolist()[:4] == [1, 1, 1, 1]
    if not guard_buffers:  # the control: the NaN is in the running statistics for good and every checkpoint is refused
        assert bool(torch.isnan(buf[0]))
        with pytest.raises(RuntimeError, match=name.replace(".", r"\.")):
            t.state_dict()
        return
    _assert_buffers_equal(_buffers(t), before, "after the skipped step")
    assert bool(torch.isfinite(buf).all())
    t.state_dict()  # does not refuse
    clean = synthetic.make_batch(BT, PT, NT, preset="everyday", seed=62, device=cuda_device)
    res = t.evaluate([clean])
    assert res and all(np.isfinite(v) for v in res.values()), res
    t.train_step(batches[2])  # and the run goes on
    assert set(_counters(t)) == {2} and bool(torch.isfinite(t.flat.flat_param).all())


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_a_raised_status_word_rolls_the_buffers_back(cuda_device, use_graph):
    """The word is raised by hand in front of a step, as a launch that gave up would leave it."""
    from multi_part_assembly_amd import gru
    batches, clean2 = _batches(cuda_device)
    t = _trainer(cuda_device, guard_step=True, guard_buffers=True, use_graph=use_graph, graph_warmup=1)
    word, host = gru.prepare(cuda_device)
    try:
        t.train_step(batches[0])
        t.train_step(clean2)
        before, (opt_before, step) = _buffers(t), _opt_state(t)
        assert set(_counters(t)) == {2}
        word.fill_(1)
        t.train_step(batches[2])
        after, (opt_after, step_after) = _buffers(t), _opt_state(t)
        assert step == step_after == 2 and all(torch.equal(x, y) for x, y in zip(opt_before, opt_after))
        _assert_buffers_equal(after, before)
        assert t.optimizer.guard_words().tolist() == [2, 2, 1, 1, -1, 3, 2, 0]
        assert "status word alone" in t.optimizer.guard_report(t.flat)["text"]
        word.zero_()
        t.train_step(batches[2])  # the same batch with the word clear is applied and committed
        assert set(_counters(t)) == {3} and torch.equal(t.buffer_slab.shadow, t.buffer_slab.live)
    finally:
        word.zero_()
        host.zero_()
        torch.cuda.synchronize()


def test_a_skipped_step_returns_to_the_loaded_checkpoint_not_to_the_fresh_model(cuda_device):
    batches, _ = _batches(cuda_device)
    t = _trainer(cuda_device, guard_step=True, guard_buffers=True)
    t.train_step(batches[0])
    ckpt = t.state_dict()
    want = _buffers(t)
    fresh = _trainer(cuda_device, guard_step=True, guard_buffers=True)
    initial = _buffers(fresh)
    assert any(not torch.equal(initial[n], want[n]) for n in want)
    fresh.load_state_dict(ckpt)
    assert torch.equal(fresh.buffer_slab.shadow, fresh.buffer_slab.live)
    fresh.train_step(batches[1])  # poisoned
    assert fresh.optimizer.guard_words().tolist()[0] == 1
    _assert_buffers_equal(_buffers(fresh), want, "after load + skipped step")
    assert set(_counters(fresh)) == {1}


def test_a_second_model_family_dgl(cuda_device):
    twin = _make_twin(cuda_device, "dgl")
    batches, _ = _batches(cuda_device)
    t = _trainer(cuda_device, "dgl", guard_step=True, guard_buffers=True)
    for b in batches:
        t.train_step(b)
    _assert_equals_twin(t, twin)
    assert t.optimizer.guard_words().tolist()[:4] == [0, 2, 1, 0]


# ---- 3. two ranks -----------------------------------------------------------------------------------------------------------------
def _rank_main(rank, port, out_dir):
    """One rank of the two-rank run (started as a program, under its own time limit): per mode, two clean steps on both
    ranks, then the status word raised on rank 1 ONLY in front of the next step."""
    import torch.distributed as dist
    from multi_part_assembly_amd import gru, synthetic
    dev = rank_setup(rank, port)
    out = {}
    for mode, use_graph in (("eager", False), ("graph", True)):
        t = _trainer(dev, guard_step=True, guard_buffers=True, use_graph=use_graph, graph_warmup=1)
        word, _ = gru.prepare(dev)
        shard = lambda seed: {k: v for k, v in synthetic.make_batch(  # noqa: E731
            BT, PT, NT, preset="everyday", seed=seed + rank, device=dev).items() if k != "num_parts"}
        t.train_step(shard(70))
        first = _buffers(t)
        t.train_step(shard(80))  # (graph: the capture and the first replay)
        before = _buffers(t)
        committed = bool(torch.equal(t.buffer_slab.shadow, t.buffer_slab.live))
        if rank == 1:
            word.fill_(1)
        t.train_step(shard(90))
        skipped = _buffers(t)
        word.zero_()
        t.train_step(shard(100))  # and the run goes on, in lock-step
        out[mode] = {"first": first, "before": before, "skipped": skipped, "after": _buffers(t), "committed": committed,
                     "graph": t._graph is not None, "words": t.optimizer.guard_words().tolist(), "counters": _counters(t)}
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_roll_back_their_own_buffers_on_the_common_verdict(cuda_device):
    got = run_two_ranks(__file__)
    for mode in ("eager", "graph"):
        a, b = got[0][mode], got[1][mode]
        assert a["graph"] == b["graph"] == (mode == "graph")
        assert a["words"][1:4] == b["words"][1:4] == [3, 1, 0], (a["words"], b["words"])
        stats = [n for n in a["before"] if n.endswith("running_mean")]
        for r in (a, b):
            assert r["committed"] and any(not torch.equal(r["first"][n], r["before"][n]) for n in stats)  # step 2 committed
            _assert_buffers_equal(r["skipped"], r["before"], mode)  # this rank's own pre-step bits
            assert set(r["counters"]) == {3} and any(not torch.equal(r["after"][n], r["before"][n]) for n in stats)
        # per-rank BatchNorm: the two ranks saw different shards, so their statistics differ — each kept its own
        assert any(not torch.equal(a["before"][n], b["before"][n]) for n in stats)


if __name__ == "__main__":
    _rank_main(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3])
