"""The weight average on the device (csrc/weight_average.hip: mpa_ema_update, mpa_ema_swap; optim.WeightAverage;
Trainer(ema_decay=...)).

Kernels against the restatement `ema_ref`, bit for bit, on random bit patterns (NaNs, infinities and denormals among
them) between sentinel-filled guard zones.  The sizes come from the kernels' launch constants: UNIT = 16 bytes per lane
and access, WAVE = 64 lanes x 16 B, BLOCK = kThreads (256) x 16 B, SWEEP = kEmaBlocks (2048) x BLOCK = what one pass of
the full grid covers; both sides of each, and zero.  The slab travels in the same launch with a mixed segment table
(float32, int64, uint8, a 4-byte buffer in a 16-byte slot, a segment longer than one block's stride, an empty one, a
gap), and once with more segments than the grid has blocks.

NaN results: IEEE 754 leaves the payload of a NaN an operation PRODUCES to the implementation, so where the restatement
gives a NaN the kernel must give a NaN, and everywhere else the same 32 bits.  Bits the kernels only move (kind-0
segments, padding, mpa_ema_swap, a skipped update) are compared as bits, NaN payloads included.

Then the trainer on pn_transformer and dgl at B = 2, P = 3, N = 64: the average follows the restatement over the recorded
trajectory (eager and captured), a skipped step leaves it alone, evaluation with the averaged weights leaves the run
alone, checkpoints and `resume` carry it, two ranks agree, and the tools run end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multi_part_assembly_amd import _lib, ema_ref
from trainer_cases import (BT, NT, PT, ROOT, SENTINEL, Zoned, batch as _batch, model as _model, random_bytes as _random_bytes,
                           rank_setup, run_two_ranks, trainer as _trainer)

pytestmark = pytest.mark.gpu

UNIT = ema_ref.UNIT
WAVE = 64 * UNIT
BLOCK = ema_ref.THREADS * UNIT
SWEEP = ema_ref.BLOCKS * BLOCK
SIZES = [0, UNIT, 2 * UNIT, WAVE - UNIT, WAVE, WAVE + UNIT, BLOCK - UNIT, BLOCK, BLOCK + UNIT, SWEEP - UNIT, SWEEP, SWEEP + UNIT]
STEPS = (1, 9, 10, 1000)
K0, K1 = ema_ref.KIND_COPY, ema_ref.KIND_F32
# float32 (20 B in a 32 B slot), int64, uint8 x 3, one float in a 16 B slot, an empty buffer, a gap of 32 bytes nobody
# owns, a float32 segment of one block's stride + 1 unit + 1 word, a kind-0 segment longer than a block's stride
MIXED = [(0, 20, K1), (32, 8, K0), (48, 3, K0), (64, 4, K1), (80, 0, K1), (112, BLOCK + UNIT + 4, K1),
         (112 + BLOCK + 2 * UNIT, BLOCK + 40, K0)]
MIXED_BYTES = 112 + BLOCK + 2 * UNIT + BLOCK + 48


# ---- 1. the kernels --------------------------------------------------------------------------------------------------------------
def _slab_bytes(segments, nbytes, seed):
    """Random bits inside the segments, zero padding (BufferSlab's layout), SENTINEL in bytes no slot owns."""
    s = np.full(nbytes, SENTINEL, dtype=np.uint8)
    rng = np.random.RandomState(seed)
    for off, size, _ in segments:
        s[off:off + (size + UNIT - 1) // UNIT * UNIT] = 0
        s[off:off + size] = rng.randint(0, 256, size=size)
    return s


def _tables(segments, dev):
    import ctypes
    words = [w for s in segments for w in s]
    if not words:
        return None, None
    return (ctypes.c_int64 * len(words))(*words), torch.tensor(words, dtype=torch.int64, device=dev)


def _hyper(dev, t):
    h = torch.zeros(8, dtype=torch.float32, device=dev)
    h[4:5].view(torch.int32).fill_(t)
    return h


def _update(dev, param, ema, live, state, segments, tables, hyper, decay, warmup, guard):
    _lib.launch("mpa_ema_update", dev, param.mid, ema.mid, param.n // 4, live.mid, state.mid, live.n, tables[0], tables[1],
                len(segments), hyper, decay, int(warmup), guard)


def _assert_same_floats(got, want, what):
    """Byte arrays of float32 words: a NaN where the restatement has a NaN, the same 32 bits everywhere else."""
    g, w = got.view(np.uint32), want.view(np.uint32)
    nan = np.isnan(want.view(np.float32))
    assert np.array_equal(np.isnan(got.view(np.float32)), nan), what
    assert np.array_equal(g[~nan], w[~nan]), what


def _assert_state(got, want, segments, what):
    """The averaged slab: float32 words of kind-1 segments as floats, every other byte (kind 0, padding, gaps) as bits."""
    moved = np.ones(got.size, dtype=bool)
    for off, size, kind in segments:
        if kind == K1:
            _assert_same_floats(got[off:off + size], want[off:off + size], what)
            moved[off:off + size] = False
    assert np.array_equal(got[moved], want[moved]), what


@pytest.mark.parametrize("n", SIZES)
def test_update_equals_the_restatement_bit_for_bit(cuda_device, n):
    dev = cuda_device
    param_h, ema_h = _random_bytes(n, n % 89), _random_bytes(n, n % 89 + 1)
    live_h, state_h = _slab_bytes(MIXED, MIXED_BYTES, 5), _slab_bytes(MIXED, MIXED_BYTES, 6)
    param, live = Zoned(param_h, dev), Zoned(live_h, dev)
    ema, state = Zoned(ema_h, dev), Zoned(state_h, dev)
    pristine = (ema.buf.clone(), state.buf.clone())
    tables = _tables(MIXED, dev)
    guard = torch.zeros(8, dtype=torch.int32, device=dev)
    nans = 0
    for t in STEPS:
        hyper = _hyper(dev, t)
        for warmup in (True, False):
            want = ema_ref.update(0, t, 0.75, warmup, param_h.view(np.float32), ema_h.view(np.float32), live_h, state_h, MIXED)
            nans += int(np.isnan(want[0]).sum())
            for verdict in (0, 1, 2, 3):
                guard[0] = verdict
                runs = []
                for _ in range(2 if verdict == 0 else 1):
                    ema.buf.copy_(pristine[0]), state.buf.copy_(pristine[1])
                    _update(dev, param, ema, live, state, MIXED, tables, hyper, 0.75, warmup, guard)
                    torch.cuda.synchronize()
                    if verdict != 0:  # a skipped update leaves every bit of the average (and of the zones)
                        assert torch.equal(ema.buf, pristine[0]) and torch.equal(state.buf, pristine[1]), (n, t, verdict)
                        continue
                    got = (ema.bytes(), state.bytes())
                    _assert_same_floats(got[0], want[0].view(np.uint8), (n, t, warmup, "parameters"))
                    _assert_state(got[1], want[1], MIXED, (n, t, warmup, "slab"))
                    assert ema.zones_intact() and state.zones_intact(), (n, t, warmup)
                    runs.append(got)
                if runs:  # bit-identical from run to run, NaN payloads included
                    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    # guard = NULL applies
    ema.buf.copy_(pristine[0]), state.buf.copy_(pristine[1])
    _update(dev, param, ema, live, state, MIXED, tables, _hyper(dev, 10), 0.75, True, None)
    torch.cuda.synchronize()
    want = ema_ref.update(0, 10, 0.75, True, param_h.view(np.float32), ema_h.view(np.float32), live_h, state_h, MIXED)
    _assert_same_floats(ema.bytes(), want[0].view(np.uint8), (n, "no guard"))
    _assert_state(state.bytes(), want[1], MIXED, (n, "no guard"))
    assert np.array_equal(param.bytes(), param_h) and np.array_equal(live.bytes(), live_h)  # the sources are read only
    assert param.zones_intact() and live.zones_intact()
    assert int(guard[0].item()) == 3 and _hyper(dev, 10)[4:5].view(torch.int32).item() == 10  # the words are read only
    if n >= BLOCK:
        assert nans > 0  # the random bits did hold NaNs


def test_update_without_a_slab_and_with_more_segments_than_blocks(cuda_device):
    dev = cuda_device
    none = np.zeros(0, np.uint8)
    param_h, ema_h = _random_bytes(WAVE + UNIT, 1), _random_bytes(WAVE + UNIT, 2)
    param, ema, live, state = (Zoned(h, dev) for h in (param_h, ema_h, none, none))
    _lib.launch("mpa_ema_update", dev, param.mid, ema.mid, param.n // 4, None, None, 0, None, None, 0, _hyper(dev, 3), 0.5, 1, None)
    torch.cuda.synchronize()
    want, _ = ema_ref.update(0, 3, 0.5, True, param_h.view(np.float32), ema_h.view(np.float32), none, none, [])
    _assert_same_floats(ema.bytes(), want.view(np.uint8), "state_bytes = 0")
    assert ema.zones_intact()
    # numel = 0 and ema_ref.BLOCKS + 3 segments of one unit each, alternating kinds: blocks 0..2 walk two segments
    count = ema_ref.BLOCKS + 3
    segments = [(UNIT * k, (12, 16, 5)[k % 3], K1 if k % 3 < 2 else K0) for k in range(count)]
    live_h, state_h = _slab_bytes(segments, UNIT * count, 7), _slab_bytes(segments, UNIT * count, 8)
    live, state = Zoned(live_h, dev), Zoned(state_h, dev)
    _lib.launch("mpa_ema_update", dev, None, None, 0, live.mid, state.mid, live.n, *_tables(segments, dev), count,
                _hyper(dev, 1000), 0.9, 0, None)
    torch.cuda.synchronize()
    _, want = ema_ref.update(0, 1000, 0.9, False, np.zeros(0, np.float32), np.zeros(0, np.float32), live_h, state_h, segments)
    _assert_state(state.bytes(), want, segments, "many segments")
    assert state.zones_intact() and np.array_equal(live.bytes(), live_h)
    # refusals on real device pointers: nothing is launched, nothing is written
    before = state.buf.clone()
    for args, why in (((live.mid[8:], state.mid[8:]), "aligned"), ((live.mid, live.mid[16:]), "overlap"),
                      ((live.mid, None), "null")):
        with pytest.raises(_lib.MpaError, match=why):
            _lib.launch("mpa_ema_update", dev, None, None, 0, args[0], args[1], 32, *_tables([(0, 16, K1)], dev), 1,
                        _hyper(dev, 1), 0.9, 0, None)
    with pytest.raises(_lib.MpaError, match="decay"):
        _lib.launch("mpa_ema_update", dev, None, None, 0, live.mid, state.mid, 32, *_tables([(0, 16, K1)], dev), 1,
                    _hyper(dev, 1), 1.0, 0, None)
    torch.cuda.synchronize()
    assert torch.equal(state.buf, before)


@pytest.mark.parametrize("n", [0, UNIT, WAVE + UNIT, BLOCK - UNIT, BLOCK + UNIT, SWEEP - UNIT, SWEEP + UNIT])
def test_swap_twice_is_the_identity(cuda_device, n):
    dev = cuda_device
    for m in (0, MIXED_BYTES):  # without and with the second pair
        hosts = [_random_bytes(n, 1), _random_bytes(n, 2), _random_bytes(m, 3), _random_bytes(m, 4)]
        a, b, c, d = (Zoned(h, dev) for h in hosts)
        swap = lambda: _lib.launch("mpa_ema_swap", dev, a.mid if n else None, b.mid if n else None, n,  # noqa: E731
                                   c.mid if m else None, d.mid if m else None, m)
        swap()
        torch.cuda.synchronize()
        for got, want in ((a, hosts[1]), (b, hosts[0]), (c, hosts[3]), (d, hosts[2])):
            assert got.bytes().tobytes() == want.tobytes() and got.zones_intact(), (n, m)
        assert a.bytes().tobytes() == ema_ref.swap(hosts[0], hosts[1])[0].tobytes()
        swap()
        torch.cuda.synchronize()
        for got, want in zip((a, b, c, d), hosts):
            assert got.bytes().tobytes() == want.tobytes() and got.zones_intact(), (n, m)


def test_a_captured_update_follows_the_device_step_word(cuda_device):
    dev = cuda_device
    n = BLOCK + 3 * UNIT
    rng = np.random.RandomState(3)
    params = [rng.randn(n // 4).astype(np.float32) for _ in range(3)]
    lives = [_slab_bytes(MIXED, MIXED_BYTES, 30 + k) for k in range(3)]
    for l in lives:  # finite statistics: the sequence is compared bit for bit
        for off, size, kind in MIXED:
            if kind == K1:
                l[off:off + size] = rng.randn(size // 4).astype(np.float32).view(np.uint8)
    ema_h, state_h = params[0] * np.float32(0.5), lives[0].copy()
    param, live = Zoned(params[0].view(np.uint8), dev), Zoned(lives[0], dev)
    eager = (Zoned(ema_h.view(np.uint8), dev), Zoned(state_h, dev))
    graph = (Zoned(ema_h.view(np.uint8), dev), Zoned(state_h, dev))
    tables, hyper = _tables(MIXED, dev), _hyper(dev, 0)
    guard = torch.zeros(8, dtype=torch.int32, device=dev)
    warm = (Zoned(ema_h.view(np.uint8), dev), Zoned(state_h, dev))
    _update(dev, param, warm[0], live, warm[1], MIXED, tables, hyper, 0.9, True, guard)  # (the code object loads outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        _update(dev, param, graph[0], live, graph[1], MIXED, tables, hyper, 0.9, True, guard)
    want = (ema_h, state_h)
    t = 0
    for k, verdict in enumerate((0, 1, 0)):  # applied, skipped, applied: the count advances with the applied steps only
        t += verdict == 0
        hyper[4:5].view(torch.int32).fill_(t)
        guard[0] = verdict
        param.mid.copy_(torch.from_numpy(params[k].view(np.uint8)))
        live.mid.copy_(torch.from_numpy(lives[k]))
        g.replay()
        _update(dev, param, eager[0], live, eager[1], MIXED, tables, hyper, 0.9, True, guard)
        torch.cuda.synchronize()
        want = ema_ref.update(verdict, t, 0.9, True, params[k], want[0], lives[k], want[1], MIXED)
        for got in (graph, eager):
            assert got[0].bytes().tobytes() == want[0].tobytes() and got[1].bytes().tobytes() == want[1].tobytes(), (k, verdict)
            assert got[0].zones_intact() and got[1].zones_intact()
    assert t == 2


# ---- 2. the trainer -------------------------------------------------------------------------------------------------------------
DECAY = 0.9


def _average(t):
    torch.cuda.synchronize()
    return t.average.ema_param.cpu().numpy().copy(), t.average.ema_state.cpu().numpy().copy()


def _live(t):
    torch.cuda.synchronize()
    return t.flat.flat_param.detach().cpu().numpy().copy(), t.buffer_slab.live.cpu().numpy().copy()


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("family,use_graph", [("pn", False), ("pn", True), ("dgl", False), ("dgl", True)])
def test_the_average_follows_the_restatement_over_the_recorded_trajectory(cuda_device, family, use_graph):
    """graph: the first step is the eager warm-up step, the second is captured and replayed, the others are replays."""
    t = _trainer(cuda_device, family, ema_decay=DECAY, use_graph=use_graph, graph_warmup=1)
    want = _average(t)
    assert _same(want, _live(t))  # the average starts as the weights
    for k in range(4):
        loss = t.train_step(_batch(cuda_device, 60 + k))
        param, live = _live(t)
        want = ema_ref.update(0, k + 1, DECAY, True, param, want[0], live, want[1], t.average.segments)
        assert _same(_average(t), want), (family, use_graph, k)
    assert bool(torch.isfinite(loss)) and (t._graph is not None) == t.use_graph
    if family == "pn":
        assert t.use_graph == use_graph
    assert not _same(_average(t), _live(t))
    counters = [n for n in t.buffer_slab.names if n.endswith("num_batches_tracked")]
    sd = t.average.averaged_state_dict(t.model)
    assert counters and all(int(sd[n]) == 4 for n in counters if n in sd)  # copied, not averaged
    t.buffer_slab.check()


@pytest.fixture(scope="module")
def twin(cuda_device):
    """An unguarded averaging trainer that takes the first and the third step ONLY."""
    t = _trainer(cuda_device, ema_decay=DECAY)
    t.train_step(_batch(cuda_device, 60))
    t.train_step(_batch(cuda_device, 62))
    return _average(t), _live(t)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("guard_buffers", [True, False], ids=["rollback", "no_rollback"])
def test_a_skipped_step_leaves_the_average_alone(cuda_device, twin, guard_buffers, use_graph):
    t = _trainer(cuda_device, ema_decay=DECAY, guard_step=True, guard_buffers=guard_buffers, use_graph=use_graph,
                 graph_warmup=1)
    poisoned = _batch(cuda_device, 61)
    poisoned["part_trans"][1, 0, 1] = float("nan")
    t.train_step(_batch(cuda_device, 60))
    after_first = _average(t)
    t.train_step(poisoned)
    assert t.optimizer.guard_words().tolist()[:4] == [1, 1, 1, 1]
    assert _same(_average(t), after_first)  # every bit, parameters and buffers
    t.train_step(_batch(cuda_device, 62))
    assert t.optimizer.guard_words().tolist()[:4] == [0, 2, 1, 0] and (t._graph is not None) == use_graph
    got = _average(t)
    assert got[0].tobytes() == twin[0][0].tobytes()  # the averaged parameters of a run that never saw the batch
    assert _live(t)[0].tobytes() == twin[1][0].tobytes()
    if guard_buffers:  # ... and the averaged buffers, once the skipped step's statistics are rolled back
        assert got[1].tobytes() == twin[0][1].tobytes()
        assert t.optimizer.guard_state is t.buffer_slab
    else:              # without the rollback the live statistics carry batch 2, and the third step averages those
        assert got[1].tobytes() != twin[0][1].tobytes() and t.optimizer.guard_state is None
    t.state_dict()  # finite: not refused


@pytest.mark.parametrize("family", ["pn", "dgl"])
def test_evaluating_the_average_leaves_the_run_alone(cuda_device, family):
    from multi_part_assembly_amd import synthetic
    from multi_part_assembly_amd.evaluate import Evaluator
    val = [synthetic.make_batch(BT, PT, NT, preset="everyday", seed=90 + k, device=cuda_device) for k in range(2)]
    plain = _trainer(cuda_device, family, ema_decay=DECAY)
    t = _trainer(cuda_device, family, ema_decay=DECAY)
    for tr in (plain, t):
        tr.train_step(_batch(cuda_device, 60))
        tr.train_step(_batch(cuda_device, 61))
    ptrs = [p.data_ptr() for p in t.model.parameters()] + [b.data_ptr() for b in t.model.buffers()]
    before = (_average(t), _live(t))
    ema = t.evaluate(val, weights="ema")
    assert not t.average.swapped and _same(_average(t), before[0]) and _same(_live(t), before[1])
    assert ptrs == [p.data_ptr() for p in t.model.parameters()] + [b.data_ptr() for b in t.model.buffers()]
    live = t.evaluate(val)
    assert list(ema) == list(live) and all(np.isfinite(v) for v in ema.values()) and ema != live
    # the metrics are those of a fresh model that loaded the averaged state dict
    fresh, _ = _model(cuda_device, family)
    fresh.load_state_dict(t.average.averaged_state_dict(t.model))
    assert Evaluator(fresh).run(val) == ema
    fresh.load_state_dict(t.model.state_dict())
    assert Evaluator(fresh).run(val) == live
    with pytest.raises(RuntimeError, match="averaging"):
        _trainer(cuda_device, family).evaluate(val, weights="ema")
    for tr in (plain, t):
        tr.train_step(_batch(cuda_device, 62))
    assert _same(_average(t), _average(plain)) and _same(_live(t), _live(plain))
    assert torch.equal(t.optimizer.exp_avg, plain.optimizer.exp_avg)


def test_a_nonfinite_average_is_refused_at_a_guarded_checkpoint(cuda_device):
    t = _trainer(cuda_device, ema_decay=DECAY, guard_step=True)
    t.train_step(_batch(cuda_device, 60))
    t.state_dict()
    t.average.ema_param[5] = float("inf")
    with pytest.raises(RuntimeError, match="the weight average of parameter 0"):
        t.state_dict()
    t.average.reset()
    name = next(n for n in t.buffer_slab.names if n.endswith("running_var"))
    off = t.buffer_slab.offsets[t.buffer_slab.names.index(name)]
    t.average.ema_state[off:off + 4].view(torch.float32).fill_(float("nan"))
    with pytest.raises(RuntimeError, match="weight average of buffer " + name.replace(".", r"\.")):
        t.state_dict()


def test_checkpoint_round_trip_and_resume_inside_a_run(cuda_device, tmp_path):
    from test_fit_gpu import Geometry, sampler_for, trainer_for
    from multi_part_assembly_amd.sampler import EpochSampler
    setup, dev = Geometry(), cuda_device
    val = setup.producer(dev, setup.val_store)
    val_batches = lambda: [val.batch([0, 1, 2], batch_counter=0), val.batch([3, 4], batch_counter=1)]  # noqa: E731
    whole = trainer_for(setup, dev, ema_decay=DECAY)
    history = whole.fit(setup.producer(dev), sampler_for(setup, dev), val_batches=val_batches, val_every=1, log_every=0)
    assert [h["val/weights"] for h in history] == ["ema"] * 3
    # validation saw the averaged weights: the last record equals an evaluation with them, not with the live ones
    assert {k: v for k, v in history[-1].items() if k.startswith("val/") and k != "val/weights"} == \
        whole.evaluate(val_batches(), weights="ema")
    assert whole.evaluate(val_batches(), weights="ema") != whole.evaluate(val_batches())
    # round trip through a file
    torch.save(whole.state_dict(), tmp_path / "whole.pt")
    other = trainer_for(setup, dev, ema_decay=DECAY)
    other.load_state_dict(torch.load(tmp_path / "whole.pt", map_location=dev, weights_only=False))
    assert _same(_average(other), _average(whole)) and _same(_live(other), _live(whole))
    # 4 steps = inside epoch 1, then everything built afresh, `resume`, and the rest of the run
    first = trainer_for(setup, dev, ema_decay=DECAY)
    first.fit(setup.producer(dev), sampler_for(setup, dev), val_batches=val_batches, val_every=1, log_every=0,
              ckpt_dir=str(tmp_path / "run"), max_steps=4)
    assert "ema" in torch.load(tmp_path / "run" / "last.pt", weights_only=False)
    fresh = trainer_for(setup, dev, ema_decay=DECAY)
    assert fresh.resume(str(tmp_path / "run")) == 1
    resumed = fresh.fit(setup.producer(dev), EpochSampler(setup.S, setup.B, seed=0, device=dev), val_batches=val_batches,
                        val_every=1, log_every=0, ckpt_dir=str(tmp_path / "run"))
    assert _same(_average(fresh), _average(whole)) and _same(_live(fresh), _live(whole))
    assert [h.get("val/part_acc") for h in resumed] == [h.get("val/part_acc") for h in history]


# ---- 3. two ranks -----------------------------------------------------------------------------------------------------------------
def _rank_main(rank, port, out_dir):
    """One rank of the two-rank run (started as a program, under its own time limit): three steps on different shards."""
    import torch.distributed as dist
    dev = rank_setup(rank, port)
    out = {}
    for mode, use_graph in (("eager", False), ("graph", True)):
        t = _trainer(dev, ema_decay=DECAY, use_graph=use_graph, graph_warmup=1)
        for k in range(3):
            t.train_step(_batch(dev, 70 + 10 * k + rank))
        out[mode] = {"average": _average(t), "live": _live(t), "graph": t._graph is not None,
                     "offsets": (t.buffer_slab.names, t.buffer_slab.offsets, t.buffer_slab.sizes, t.average.segments)}
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_end_with_identical_averaged_parameters(cuda_device):
    got = run_two_ranks(__file__, weights_only=False)  # (numpy arrays among the results)
    for mode in ("eager", "graph"):
        a, b = got[0][mode], got[1][mode]
        assert a["graph"] == b["graph"] == (mode == "graph")
        # the parameters are common (one reduced gradient), so their averages are identical on both ranks
        assert a["live"][0].tobytes() == b["live"][0].tobytes() and a["average"][0].tobytes() == b["average"][0].tobytes()
        assert a["average"][0].tobytes() != a["live"][0].tobytes()
        # per-rank BatchNorm statistics (the reference's DDP semantics): each rank averages its own, from the common start
        names, offsets, sizes, segments = a["offsets"]
        for name, off, size, seg in zip(names, offsets, sizes, segments):
            if name.endswith("num_batches_tracked"):
                assert a["average"][1][off:off + size].tobytes() == b["average"][1][off:off + size].tobytes()
                assert int(a["average"][1][off:off + size].view(np.int64)[0]) == 3
    assert got[0]["eager"]["average"][0].tobytes() == got[0]["graph"]["average"][0].tobytes()


# ---- 4. the tools ------------------------------------------------------------------------------------------------------------------
def test_train_tool_with_ema_then_evaluate_tool_with_the_averaged_weights(cuda_device, tmp_path):
    from multi_part_assembly_amd import assemble, synthetic
    ckpt = tmp_path / "ckpt"
    train = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "train.py"), "--synthetic",
                            "--preset", "pn_transformer_everyday", "--synthetic-shapes", "16", "--batch-size", "8", "--ema",
                            "0.99", "--epochs", "2", "--val-every", "1", "--ckpt-dir", str(ckpt), "--log-every", "1"],
                           capture_output=True, text=True)
    assert train.returncode == 0, train.stdout + train.stderr
    assert "done: 2 epochs" in train.stdout and "val/weights: ema" in train.stdout
    state = torch.load(ckpt / "last.pt", weights_only=False)
    assert state["ema"]["decay"] == 0.99 and state["ema"]["warmup"] is True and list(state["ema"]["model"]) == list(state["model"])
    assert any(not torch.equal(state["ema"]["model"][k], state["model"][k]) for k in state["model"])
    shapes = synthetic.make_fracture_meshes(7, 3, [2, 3, 2], 40)
    folders = []
    for s, parts in enumerate(shapes):
        rel = os.path.join("everyday", "Bottle", f"shape{s}", "fractured_0")
        os.makedirs(tmp_path / "data" / rel)
        for k, (v, f) in enumerate(parts):
            assemble.write_obj(tmp_path / "data" / rel / f"piece_{k}.obj", v[f])
        folders.append(os.path.dirname(rel))
    (tmp_path / "data" / "val.txt").write_text("\n".join(folders) + "\n")
    results = {}
    for weights in ("ema", "live"):
        run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "evaluate.py"), "--preset",
                              "pn_transformer_everyday", "--weight", str(ckpt / "last.pt"), "--weights", weights, "--data-dir",
                              str(tmp_path / "data"), "--data-fn", "val.txt", "--max-num-part", "4"],
                             capture_output=True, text=True)
        assert run.returncode == 0, run.stdout + run.stderr
        results[weights] = next(line for line in run.stdout.splitlines() if "test/part_acc" in line)
    assert results["ema"] != results["live"]  # (a checkpoint without the entry: tests/test_weight_average.py, no process needed)


if __name__ == "__main__":
    _rank_main(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3])
