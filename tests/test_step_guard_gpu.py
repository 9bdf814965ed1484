"""The guarded optimiser step on the device (csrc/adam.hip: mpa_step_guard, mpa_adam_step_guarded, mpa_guard_mark).

Kernel against the numpy restatement (`guard_ref`), words and coefficient bit for bit, over the sizes at which the pass
changes its path (the float4 tail, the 256-thread block, both sides of the 512 x 256 x 4 grid stride); the update against
`mpa_adam_step_dev`, bit for bit; a skipped step is the identity on random bits; a captured pair equals the eager calls.
Then the trainer: a poisoned batch between two clean ones leaves parameters, moments and step count equal to those of a
twin that never took the poisoned optimiser step, eager and captured; a raised status word skips the step; a checkpoint
refuses non-finite state; two gloo ranks reach one verdict from a status word raised on one of them."""
import os
import sys

import numpy as np
import pytest
import torch

from multi_part_assembly_amd import _lib, guard_ref
from trainer_cases import (BT, NT, PT, batches as _batches, i32 as _i32, model as _model, opt_state, rank_setup, run_two_ranks,
                           trainer as _trainer)

pytestmark = pytest.mark.gpu

STRIDE = guard_ref.BLOCKS * guard_ref.THREADS * 4  # elements one sweep of the pass covers
SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1025, STRIDE - 1, STRIDE, STRIDE + 1, STRIDE + 3, 2 * STRIDE + 1]
B1, B2 = 0.9, 0.999


# ---- calling the library ---------------------------------------------------------------------------------------------------------
class Guard:
    """Hyper buffer, guard words and workspace of one optimiser on the device, with their numpy twins."""

    def __init__(self, dev, lr=1e-3, scale=1.0):
        self.dev = dev
        self.hyper = torch.from_numpy(guard_ref.new_hyper(lr=lr, grad_scale=scale)).to(dev)
        self.words = torch.zeros(8, dtype=torch.int32, device=dev)
        self.ws = torch.empty(_lib.query("mpa_step_guard_workspace") // 4, dtype=torch.int32, device=dev)
        self.ref_hyper = guard_ref.new_hyper(lr=lr, grad_scale=scale)
        self.ref_words = np.zeros(8, dtype=np.int32)

    def run(self, grad, max_norm=0.0, scale=1.0, scale_dev=None, status=None):
        _lib.launch("mpa_step_guard", self.dev, grad if grad.numel() else None, grad.numel(), float(max_norm), scale_dev,
                    float(scale), status, self.ws, self.hyper, self.words, B1, B2)

    def run_ref(self, grad, max_norm=0.0, scale=1.0, status=None):
        return guard_ref.step_guard(grad, max_norm, scale, status, self.ref_hyper, self.ref_words, B1, B2)

    def assert_equals_ref(self, what=""):
        assert self.words.cpu().numpy().tolist() == self.ref_words.tolist(), what
        got, want = self.hyper.cpu().numpy().view(np.int32), self.ref_hyper.view(np.int32)
        assert got.tolist() == want.tolist(), (what, self.hyper.cpu().numpy(), self.ref_hyper)


def clip_coef(grad, max_norm, scale=1.0, scale_dev=None):
    """(coefficient, norm) bits from mpa_grad_clip_coef."""
    dev = grad.device
    ws = torch.empty(_lib.query("mpa_grad_clip_workspace") // 8, dtype=torch.float64, device=dev)
    coef = torch.zeros(2, dtype=torch.float32, device=dev)
    _lib.launch("mpa_grad_clip_coef", dev, grad, grad.numel(), float(max_norm), scale_dev, float(scale), ws, coef)
    return coef.cpu().numpy().view(np.int32).tolist()


def _grad(n, seed=0):
    return np.random.RandomState(1000 + seed).randn(n).astype(np.float32)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def finite(cuda_device):
    """One finite gradient per size with its norm, made once: {n: (host, device, norm)}."""
    out = {}
    for n in SIZES:
        g = _grad(n, seed=n % 97)
        out[n] = (g, _dev(g, cuda_device), float(np.sqrt(guard_ref.sum_of_squares(g))))
    return out


# ---- 1. the pass and the verdict against the restatement ------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_finite_gradient_words_and_coefficient_equal_the_restatement_and_the_clip_kernel(cuda_device, finite, n):
    g, gd, norm = finite[n]
    guard = Guard(cuda_device)
    half = torch.full((1,), 0.5, dtype=torch.float32, device=cuda_device)
    cases = [dict(max_norm=0.5 * norm), dict(max_norm=2.0 * norm + 1.0), dict(max_norm=0.0), dict(max_norm=-1.0),
             dict(max_norm=0.25 * norm, scale=0.5), dict(max_norm=0.25 * norm, scale=0.5, device_scale=True)]
    for case in cases:
        on_dev = case.pop("device_scale", False)
        if n == 0 and case["max_norm"] == 0.5 * norm:
            case["max_norm"] = 1.0
        guard.run(gd, scale_dev=half if on_dev else None, **({**case, "scale": 99.0} if on_dev else case))
        assert guard.run_ref(g, **case) == 0
        guard.assert_equals_ref(case)
        if case["max_norm"] > 0 and n > 0:  # the exact bits of the unguarded clipping
            got = guard.hyper[5:7].cpu().numpy().view(np.int32).tolist()
            assert got == clip_coef(gd, case["max_norm"], case.get("scale", 1.0))
    assert guard.words.tolist()[:4] == [0, len(cases), 0, 0]
    assert int(guard.hyper[4:5].view(torch.int32).item()) == len(cases)  # every verdict-0 call advanced the step count


def _bad_positions(n):
    """Element 0, the last element, the tail, and both sides of the block / sweep boundaries that exist at this size."""
    pos = {0, n - 1, n - 2, n // 4 * 4, n // 4 * 4 - 1, 1023, 1024, STRIDE - 1, STRIDE, STRIDE + 2, 2 * STRIDE - 1, 2 * STRIDE}
    return sorted(p for p in pos if 0 <= p < n)


@pytest.mark.parametrize("n", [1, 3, 5, 1025, STRIDE + 3, 2 * STRIDE + 1])
def test_one_nonfinite_element_anywhere_trips_and_is_found(cuda_device, finite, n):
    g, gd, norm = finite[n]
    guard = Guard(cuda_device)
    work = gd.clone()
    for k, pos in enumerate(_bad_positions(n)):
        bad = (np.nan, np.inf, -np.inf)[k % 3] if n > 5 else None
        for value in ((bad,) if bad is not None else (np.nan, np.inf, -np.inf)):
            work.copy_(gd)
            work[pos] = float(value)
            poisoned = g.copy()
            poisoned[pos] = value
            guard.run(work, max_norm=0.5 * norm)
            assert guard.run_ref(poisoned, max_norm=0.5 * norm) == guard_ref.NONFINITE
            guard.assert_equals_ref((pos, value))
            assert int(guard.words[4].item()) == pos
    assert int(guard.hyper[4:5].view(torch.int32).item()) == 0  # never advanced
    guard.run(gd, max_norm=0.5 * norm)                          # and a clean gradient behind them is applied
    guard.run_ref(g, max_norm=0.5 * norm)
    guard.assert_equals_ref("clean")
    assert guard.words.tolist()[0] == 0 and guard.words.tolist()[3] == 0


@pytest.mark.parametrize("n", [5, 2 * STRIDE + 1])
def test_two_bad_elements_report_the_smaller_index_and_two_runs_agree(cuda_device, finite, n):
    g, gd, _ = finite[n]
    pairs = [(4, 1)] if n == 5 else [(STRIDE + 5, 7), (2 * STRIDE, STRIDE - 1), (1030, 1020), (n - 1, n - 2)]
    for hi, lo in pairs:  # (hi is written first and lies in another thread, block or sweep than lo)
        work, poisoned = gd.clone(), g.copy()
        work[hi], work[lo] = float("inf"), float("nan")
        poisoned[hi], poisoned[lo] = np.inf, np.nan
        runs = []
        for _ in range(2):
            guard = Guard(cuda_device)
            guard.run(work, max_norm=1.0)
            guard.run_ref(poisoned, max_norm=1.0)
            guard.assert_equals_ref((hi, lo))
            runs.append((guard.words.tolist(), _i32(guard.hyper).tolist()))
        assert runs[0] == runs[1] and runs[0][0][4] == lo


@pytest.mark.parametrize("n", [1, 4, 7, 1025, STRIDE + 3])
def test_extreme_finite_values_do_not_trip(cuda_device, n):
    guard = Guard(cuda_device)
    big = np.full(n, 3e38, dtype=np.float32)
    big[::2] *= -1
    tiny = np.full(n, 1e-45, dtype=np.float32)  # denormals
    tiny[::3] *= -1
    mixed = _grad(n)
    mixed[0], mixed[-1] = 3e38, -1e-45
    for g in (big, tiny, mixed):
        guard.run(_dev(g, cuda_device))
        assert guard.run_ref(g) == 0
        guard.assert_equals_ref()
    assert guard.words.tolist()[:3] == [0, 3, 0]


def test_status_word_zero_raised_and_null(cuda_device, finite):
    g, gd, norm = finite[1025]
    guard = Guard(cuda_device)
    status = torch.zeros(1, dtype=torch.int32, device=cuda_device)
    nan = g.copy()
    nan[77] = np.nan
    nand = _dev(nan, cuda_device)
    empty = torch.zeros(0, dtype=torch.float32, device=cuda_device)
    # (gradient host, device, status value or None = NULL)
    seq = [(g, gd, 0), (g, gd, 3), (nan, nand, -1), (g, gd, None), (nan, nand, 0), (g[:0], empty, 0), (g[:0], empty, 9),
           (g[:0], empty, None), (g, gd, 1), (g, gd, 0)]
    verdicts = []
    for host, dev_g, st in seq:
        if st is not None:
            status.fill_(st)
        guard.run(dev_g, max_norm=0.5 * norm, status=status if st is not None else None)
        verdicts.append(guard.run_ref(host, max_norm=0.5 * norm, status=st))
        guard.assert_equals_ref(st)
    assert verdicts == [0, 2, 3, 0, 1, 0, 2, 0, 2, 0]
    assert guard.words.tolist() == [0, 5, 5, 0, -1, 9, 3, 0]


# ---- 2. the update -----------------------------------------------------------------------------------------------------------
N_UPD = 4 * 1300 + 3  # six blocks of the update and a three-element tail

CONFIGS = {"adam": dict(wd=0.0, decoupled=0, mask=False), "adam_l2": dict(wd=0.01, decoupled=0, mask=False),
           "adamw_mask": dict(wd=0.01, decoupled=1, mask=True)}


class State:
    """param / exp_avg / exp_avg_sq / hyper of one optimiser; `unguarded` = [mpa_grad_clip_coef +] mpa_adam_step_dev."""

    def __init__(self, dev, cfg, clip, seed=0, random_bits=False):
        rng = np.random.RandomState(seed)
        self.dev, self.cfg, self.clip = dev, cfg, clip
        if random_bits:
            bits = [rng.randint(-2 ** 31, 2 ** 31, size=N_UPD, dtype=np.int64).astype(np.int32) for _ in range(3)]
            self.p, self.m, self.v = (_dev(b, dev).view(torch.float32) for b in bits)
        else:
            self.p = _dev(rng.randn(N_UPD).astype(np.float32), dev)
            self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.mask = _dev((rng.rand(N_UPD) < 0.7).astype(np.float32), dev) if cfg["mask"] else None
        self.guard = Guard(dev, lr=1e-2, scale=0.5)
        self.hyper = self.guard.hyper
        self.clip_ws = torch.empty(_lib.query("mpa_grad_clip_workspace") // 8, dtype=torch.float64, device=dev)

    def _tail(self):
        return (B1, B2, 1e-8, self.cfg["wd"], self.cfg["decoupled"], self.mask)

    def guarded(self, grad, status=None):
        self.guard.run(grad, max_norm=self.clip or 0.0, scale_dev=self.hyper.data_ptr() + 12, status=status)
        _lib.launch("mpa_adam_step_guarded", self.dev, self.p, grad, self.m, self.v, N_UPD, self.hyper, *self._tail(),
                    self.guard.words)

    def unguarded(self, grad):
        if self.clip:
            _lib.launch("mpa_grad_clip_coef", self.dev, grad, N_UPD, float(self.clip), self.hyper.data_ptr() + 12, 1.0,
                        self.clip_ws, self.hyper.data_ptr() + 20)
        _lib.launch("mpa_adam_step_dev", self.dev, self.p, grad, self.m, self.v, N_UPD, self.hyper, *self._tail())

    def bits(self, hyper_words=7):
        return [_i32(self.p), _i32(self.m), _i32(self.v), _i32(self.hyper)[:hyper_words]]


def _assert_same(a, b, what=""):
    for name, x, y in zip(("param", "exp_avg", "exp_avg_sq", "hyper"), a, b):
        assert torch.equal(x, y), (what, name)


@pytest.fixture(scope="module")
def step_grads(cuda_device):
    """Five finite gradients (norm about sqrt(N_UPD) = 72: a clip at 10 bites, scaled by 0.5) and a poisoned one."""
    grads = [_dev(_grad(N_UPD, seed=s), cuda_device) for s in range(5)]
    bad = grads[1].clone()
    bad[N_UPD - 2] = float("nan")
    return grads, bad


@pytest.mark.parametrize("clip", [None, 10.0], ids=["noclip", "clip"])
@pytest.mark.parametrize("kind", list(CONFIGS))
def test_five_guarded_steps_equal_five_unguarded_steps(cuda_device, step_grads, kind, clip):
    grads, _ = step_grads
    a, b = State(cuda_device, CONFIGS[kind], clip), State(cuda_device, CONFIGS[kind], clip)
    for k, g in enumerate(grads):
        a.guarded(g)
        b.unguarded(g)
        # hyper[6] (the norm, information only) is written by the guard alone when clipping is off
        _assert_same(a.bits(7 if clip else 6), b.bits(7 if clip else 6), k)
    assert a.guard.words.tolist() == [0, 5, 0, 0, 0, 0, 0, 0]
    assert int(a.hyper[4:5].view(torch.int32).item()) == 5 and bool(torch.isfinite(a.p).all())


@pytest.mark.parametrize("why", ["nan", "status"])
def test_a_skipped_step_leaves_every_buffer_bit_unchanged(cuda_device, step_grads, why):
    grads, bad = step_grads
    s = State(cuda_device, CONFIGS["adamw_mask"], 10.0, seed=3, random_bits=True)
    s.hyper[1:3] = torch.tensor([0.271, 0.0547], device=cuda_device)  # some step's corrections: they must survive
    s.hyper[4:5].view(torch.int32).fill_(3)
    before = s.bits(8)
    status = torch.ones(1, dtype=torch.int32, device=cuda_device)
    s.guarded(bad if why == "nan" else grads[0], status=status if why == "status" else None)
    after = s.bits(8)
    _assert_same(before[:3], after[:3], why)
    assert torch.equal(before[3][[0, 1, 2, 3, 4, 7]], after[3][[0, 1, 2, 3, 4, 7]])
    assert s.guard.words.tolist() == ([1, 0, 1, 1, N_UPD - 2, 1, 1, 0] if why == "nan" else [2, 0, 1, 1, -1, 1, 2, 0])


def test_the_step_after_a_skip_is_the_step_of_an_optimiser_that_never_saw_it(cuda_device, step_grads):
    grads, bad = step_grads
    a, b = State(cuda_device, CONFIGS["adam_l2"], 10.0), State(cuda_device, CONFIGS["adam_l2"], 10.0)
    for g in (grads[0], bad, grads[2], bad, bad, grads[3]):
        a.guarded(g)
    for g in (grads[0], grads[2], grads[3]):
        b.unguarded(g)
    _assert_same(a.bits(), b.bits())
    assert a.guard.words.tolist() == [0, 3, 3, 0, N_UPD - 2, 5, 1, 0]


def test_a_captured_pair_replayed_over_apply_skip_apply_equals_the_eager_calls(cuda_device, step_grads):
    grads, bad = step_grads
    eager, graph = State(cuda_device, CONFIGS["adamw_mask"], 10.0), State(cuda_device, CONFIGS["adamw_mask"], 10.0)
    static = grads[0].clone()
    status = torch.zeros(1, dtype=torch.int32, device=cuda_device)
    State(cuda_device, CONFIGS["adamw_mask"], 10.0).guarded(static, status=status)  # (code objects load outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        graph.guarded(static, status=status)
    seq = [(grads[0], 0), (bad, 0), (grads[2], 0), (grads[3], 4), (grads[4], 0)]
    for grad, st in seq:
        static.copy_(grad)
        status.fill_(st)
        g.replay()
        eager.guarded(grad, status=status)
        _assert_same(eager.bits(), graph.bits(), st)
        assert eager.guard.words.tolist() == graph.guard.words.tolist()
    assert graph.guard.words.tolist() == [0, 3, 2, 0, -1, 4, 3, 0]


def test_guard_mark_writes_element_zero_only_and_only_when_raised(cuda_device, finite):
    _, gd, _ = finite[1025]
    work = gd.clone()
    status = torch.zeros(1, dtype=torch.int32, device=cuda_device)
    _lib.launch("mpa_guard_mark", cuda_device, status, work, work.numel())
    assert torch.equal(_i32(work), _i32(gd))
    status.fill_(-5)
    _lib.launch("mpa_guard_mark", cuda_device, status, work, work.numel())
    got = _i32(work)
    assert got[0].item() == 0x7FC00000 and torch.equal(got[1:], _i32(gd)[1:])
    want = gd.cpu().numpy().copy()
    guard_ref.guard_mark(-5, want)
    assert np.isnan(want[0]) and bool(torch.isnan(work[0]))


# ---- 3. the trainer -------------------------------------------------------------------------------------------------------------
def _opt_state(trainer):
    return opt_state(trainer, _i32)  # (int32 words)


@pytest.fixture(scope="module")
def twin(cuda_device):
    """An unguarded trainer that takes the first step, runs forward and backward of the CLEAN second batch without an
    optimiser step (the forward-side state — BatchNorm statistics — moves as in the poisoned step) and takes the third."""
    (b1, _, b3), clean2 = _batches(cuda_device)
    t = _trainer(cuda_device)
    t.train_step(b1)
    t.model.train()
    t._fwd_bwd(clean2)
    t.train_step(b3)
    return _opt_state(t)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_a_poisoned_step_is_skipped_and_the_run_equals_the_twin(cuda_device, twin, use_graph):
    batches, _ = _batches(cuda_device)
    # graph: the first step is the eager warm-up step, the poisoned one is captured and replayed, the third is a replay
    t = _trainer(cuda_device, guard_step=True, use_graph=use_graph, graph_warmup=1)
    for b in batches:
        loss = t.train_step(b)
    assert use_graph == (t._graph is not None)
    state, step = _opt_state(t)
    assert step == 2 == twin[1]
    for name, x, y in zip(("parameters", "exp_avg", "exp_avg_sq"), state, twin[0]):
        assert torch.equal(x, y), name
    assert bool(torch.isfinite(t.flat.flat_param).all()) and bool(torch.isfinite(loss))
    rep = t.optimizer.guard_report(t.flat)
    assert (rep["applied"], rep["skipped"], rep["skipped_in_a_row"], rep["verdicts_or"]) == (2, 1, 0, 1)
    assert rep["last_skipped_attempt"] == 2
    k = rep["parameter"]
    assert 0 <= k < len(t.flat.params) and 0 <= rep["element"] < t.flat.params[k].numel()
    assert rep["shape"] == tuple(t.flat.params[k].shape) and f"parameter {k}" in rep["text"]
    # the checkpoint: "step" is the device's count of APPLIED steps, the words travel, a fresh trainer takes both
    ckpt = t.state_dict()
    assert ckpt["optimizer"]["step"] == 2 and t.optimizer.step_count == 3
    assert ckpt["optimizer"]["guard"].tolist()[1:4] == [2, 1, 0]
    fresh = _trainer(cuda_device, guard_step=True)
    fresh.load_state_dict(ckpt)
    assert fresh.optimizer.step_count == 2 and fresh.optimizer.guard_words().tolist() == t.optimizer.guard_words().tolist()
    assert torch.equal(_i32(fresh.flat.flat_param), state[0]) and torch.equal(_i32(fresh.optimizer.exp_avg), state[1])


def test_the_same_sequence_without_the_guard_ends_in_nonfinite_parameters(cuda_device):
    batches, _ = _batches(cuda_device)
    t = _trainer(cuda_device)
    assert t.guard_step is False
    for b in batches:
        t.train_step(b)
    assert not bool(torch.isfinite(t.flat.flat_param).all())


def test_an_unguarded_trainer_step_is_mpa_adam_step_dev_on_the_same_gradient(cuda_device):
    """The guard-off path is the parent's: one train_step equals forward + backward on a twin model followed by a direct
    mpa_adam_step_dev call with a hand-made hyper buffer."""
    from multi_part_assembly_amd.dp import ordered_parameters
    from multi_part_assembly_amd.gradsink import GradSink
    from multi_part_assembly_amd.optim import FlatBuffers
    (b1, _, _), _ = _batches(cuda_device)
    t = _trainer(cuda_device)
    t.train_step(b1)
    model, cfg = _model(cuda_device)
    flat = FlatBuffers(ordered_parameters(model))
    model.train()
    with GradSink():
        model.training_step(b1, 0).backward()
    hyper = torch.from_numpy(guard_ref.new_hyper(lr=float(t.optimizer.lr), grad_scale=1.0)).to(cuda_device)
    m, v = torch.zeros_like(flat.flat_param), torch.zeros_like(flat.flat_param)
    assert cfg.optimizer.weight_decay == 0 and not cfg.optimizer.clip_grad  # (no decay mask, no clipping in the hand-made call)
    _lib.launch("mpa_adam_step_dev", cuda_device, flat.flat_param, flat.flat_grad, m, v, flat.numel, hyper, B1, B2, 1e-8,
                0.0, 0, None)
    assert torch.equal(_i32(t.flat.flat_param), _i32(flat.flat_param))
    assert torch.equal(_i32(t.optimizer.exp_avg), _i32(m)) and torch.equal(_i32(t.optimizer.exp_avg_sq), _i32(v))
    assert torch.equal(_i32(t.optimizer._hyper_dev)[:6], _i32(hyper)[:6])


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_a_raised_status_word_skips_the_step_and_check_health_reports_it(cuda_device, use_graph):
    """The word is raised by hand in front of a step, as a launch that gave up would leave it; its pinned copy arrives
    later (here: copied by hand behind the step), so the step itself runs — and must not touch the parameters."""
    from multi_part_assembly_amd import gru
    batches, clean2 = _batches(cuda_device)
    t = _trainer(cuda_device, guard_step=True, use_graph=use_graph, graph_warmup=1)
    word, host = gru.prepare(cuda_device)
    try:
        t.train_step(batches[0])
        t.train_step(clean2)
        before, step = _opt_state(t)
        word.fill_(1)
        t.train_step(batches[2])
        after, step_after = _opt_state(t)
        assert step == step_after == 2
        for x, y in zip(before, after):
            assert torch.equal(x, y)
        assert t.optimizer.guard_words().tolist() == [2, 2, 1, 1, -1, 3, 2, 0]
        assert "status word alone" in t.optimizer.guard_report(t.flat)["text"]
        host.copy_(word)
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match="gave up"):
            t.check_health()
        with pytest.raises(RuntimeError, match="earlier check_health"):  # sticky, as before
            t.state_dict()
    finally:
        word.zero_()
        host.zero_()
        torch.cuda.synchronize()


def test_a_guarded_checkpoint_refuses_nonfinite_buffers_and_parameters(cuda_device):
    batches, _ = _batches(cuda_device)
    t = _trainer(cuda_device, guard_step=True)
    t.train_step(batches[0])
    assert t.state_dict()["optimizer"]["step"] == 1
    name, buf = next((n, b) for n, b in t.model.named_buffers() if n.endswith("running_mean"))
    keep = buf.clone()
    buf[0] = float("nan")
    with pytest.raises(RuntimeError, match=name.replace(".", r"\.")):
        t.state_dict()
    buf.copy_(keep)
    t.state_dict()
    k = len(t.flat.params) // 2
    with torch.no_grad():
        t.flat.params[k].view(-1)[0] = float("inf")
    with pytest.raises(RuntimeError, match=f"parameter {k} "):
        t.state_dict()
    unguarded = _trainer(cuda_device)  # (the refusal is the guarded trainer's: nothing changes for the others)
    with torch.no_grad():
        unguarded.flat.params[0].view(-1)[0] = float("nan")
    unguarded.state_dict()


# ---- 4. two ranks -----------------------------------------------------------------------------------------------------------------
def _rank_main(rank, port, out_dir):
    """One rank of the two-rank run (started as a program, under its own time limit): per mode, one clean step on both
    ranks, then the status word raised on rank 1 ONLY in front of the next step."""
    import torch.distributed as dist
    from multi_part_assembly_amd import gru, synthetic
    dev = rank_setup(rank, port)
    out = {}
    for mode, use_graph in (("eager", False), ("graph", True)):
        t = _trainer(dev, guard_step=True, use_graph=use_graph, graph_warmup=1)
        word, _ = gru.prepare(dev)
        shard = lambda seed: {k: v for k, v in synthetic.make_batch(  # noqa: E731
            BT, PT, NT, preset="everyday", seed=seed + rank, device=dev).items() if k != "num_parts"}
        t.train_step(shard(70))
        t.train_step(shard(80))  # (graph: the capture and the first replay)
        torch.cuda.synchronize()
        before = t.flat.flat_param.cpu().clone()
        if rank == 1:
            word.fill_(1)
        t.train_step(shard(90))
        torch.cuda.synchronize()
        skipped = t.flat.flat_param.cpu().clone()
        word.zero_()
        t.train_step(shard(100))  # and the run goes on, in lock-step
        torch.cuda.synchronize()
        out[mode] = {"before": before, "skipped": skipped, "graph": t._graph is not None}
        out[mode]["words"] = t.optimizer.guard_words().tolist()
        out[mode]["after"] = t.flat.flat_param.cpu().clone()
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_reach_one_verdict_from_a_status_word_raised_on_one(cuda_device):
    got = run_two_ranks(__file__)
    for mode in ("eager", "graph"):
        a, b = got[0][mode], got[1][mode]
        assert a["graph"] == b["graph"] == (mode == "graph")
        # both ranks skipped the third step and nothing else; rank 1 also saw its own word
        assert a["words"][1:4] == b["words"][1:4] == [3, 1, 0], (a["words"], b["words"])
        assert a["words"][5] == b["words"][5] == 3 and a["words"][6] == 1 and b["words"][6] == 3
        assert torch.equal(a["before"], b["before"]) and torch.equal(a["after"], b["after"])
        assert torch.equal(a["skipped"], a["before"]) and torch.equal(b["skipped"], b["before"])  # unchanged, bit for bit
        assert bool(torch.isfinite(a["after"]).all()) and not torch.equal(a["after"], a["before"])


def test_two_rank_skip_leaves_the_parameters_unchanged(cuda_device):
    """One process, the collective stood in for by hand: the reduced gradient of a step whose first element a rank marked
    is non-finite, so the guarded step behind it is the identity (what each of the two ranks above does)."""
    batches, _ = _batches(cuda_device)
    t = _trainer(cuda_device, guard_step=True)
    t.train_step(batches[0])
    before, _ = _opt_state(t)
    word = t.optimizer.launch_status
    t.optimizer.launch_status = None  # the rank whose own word is clear ...
    try:
        t.model.train()
        t._fwd_bwd(batches[2])
        other = torch.ones(1, dtype=torch.int32, device=cuda_device)
        _lib.launch("mpa_guard_mark", cuda_device, other, t.flat.flat_grad, t.flat.numel)  # ... receives the other's mark
        t.optimizer.prepare_hyper()
        t.optimizer.step_dev()
    finally:
        t.optimizer.launch_status = word
    after, step = _opt_state(t)
    assert step == 1 and all(torch.equal(x, y) for x, y in zip(before, after))
    assert t.optimizer.guard_words().tolist()[:5] == [1, 1, 1, 1, 0]


if __name__ == "__main__":
    _rank_main(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3])
