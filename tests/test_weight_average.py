"""The weight average without a device: the restatement `ema_ref` (coefficient table, hand-written apply / skip sequences,
segment kinds, swap), `optim.WeightAverage` on host tensors, the argument refusals of mpa_ema_update / mpa_ema_swap
through `_lib` and of the Python layer, the launches of a step with the switch off (the parent's) and on (exactly one
more, mpa_ema_update, last), `fit`'s `val_weights`, the checkpoint rules and the three tools' flags."""
import ctypes
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

from multi_part_assembly_amd import _lib, ema_ref
from multi_part_assembly_amd.optim import BufferSlab, FlatBuffers, FusedAdam, WeightAverage
from trainer_cases import (StubProducer, StubSampler, StubTrainer, bits_bytes as _bits, built, cpu_trainer as _trainer,  # noqa: F401
                           optimizer_presets, record as _record, tiny_cfg as _tiny_cfg)
from tool_loader import load_tool as _tool

f32 = np.float32


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------
def test_coefficient_table():
    c = ema_ref.coefficient
    assert c(1, 0.999, True).dtype == np.float32
    assert c(1, 0.999, True) == f32(1.0) - f32(2.0) / f32(11.0)        # t = 1: d = 2/11 as float32
    assert c(9, 0.999, True) == f32(1.0) - f32(10.0) / f32(19.0)
    # the crossover: q = (1 + t) / (10 + t) passes decay = 0.9 between t = 80 (q = 0.9 exactly in reals) and t = 81
    for t in (1, 50, 79):
        assert c(t, 0.9, True) == f32(1.0) - (f32(1.0) + f32(t)) / (f32(10.0) + f32(t)) and c(t, 0.9, True) > c(t, 0.9, False)
    for t in (81, 1000, 10 ** 6):
        assert c(t, 0.9, True) == c(t, 0.9, False) == f32(1.0) - f32(0.9)
    assert c(80, 0.9, True) == f32(1.0) - np.fmin(f32(0.9), f32(81.0) / f32(90.0))
    # warmup = 0: the decay from the first step; decay = 0: the average IS the weights (c = 1)
    assert c(1, 0.999, False) == f32(1.0) - f32(0.999)
    assert c(1, 0.0, True) == c(12345, 0.0, False) == f32(1.0)
    # (float)t rounds at and beyond 2^24: 2^24 + 1 is not a float32 (ties to even: 2^24), 2^24 + 3 becomes 2^24 + 4
    for t, a in ((2 ** 24, 2 ** 24), (2 ** 24 + 1, 2 ** 24), (2 ** 24 + 3, 2 ** 24 + 4), (2 ** 31 - 1, 2 ** 31)):
        q = (f32(1.0) + f32(a)) / (f32(10.0) + f32(a))
        assert c(t, 0.99999994, True) == f32(1.0) - np.fmin(f32(0.99999994), q), t
    assert c(2 ** 24 + 1, 0.99999994, True) == c(2 ** 24, 0.99999994, True)


SEGMENTS = [(0, 20, ema_ref.KIND_F32), (32, 8, ema_ref.KIND_COPY), (48, 4, ema_ref.KIND_F32), (64, 3, ema_ref.KIND_COPY)]
STATE_BYTES = 80


def _state(seed):
    """A slab in BufferSlab's layout for SEGMENTS: five floats, an int64 counter, one float in a 16-byte slot, three flag
    bytes; zero padding."""
    rng = np.random.RandomState(seed)
    s = np.zeros(STATE_BYTES, dtype=np.uint8)
    s[0:20] = rng.randn(5).astype(f32).view(np.uint8)
    s[32:40] = np.array([rng.randint(1, 2 ** 40)], dtype=np.int64).view(np.uint8)
    s[48:52] = rng.randn(1).astype(f32).view(np.uint8)
    s[64:67] = rng.randint(0, 2, size=3).astype(np.uint8)
    return s


def _padding_mask():
    used = np.zeros(STATE_BYTES, dtype=bool)
    for off, size, _ in SEGMENTS:
        used[off:off + size] = True
    return ~used


def test_update_over_apply_skip_skip_apply_by_hand():
    rng = np.random.RandomState(0)
    params = [rng.randn(8).astype(f32) for _ in range(4)]
    lives = [_state(10 + k) for k in range(4)]
    ema, state = params[0].copy() * f32(0.5), _state(3)
    start = (ema.copy(), state.copy())
    t, seen = 0, []
    for k, verdict in enumerate((0, 1, 3, 0)):  # applied, skipped (NaN), skipped (NaN and status word), applied
        t += verdict == 0                       # the guarded step advances the count only when it applies
        keep = (ema.copy(), state.copy())
        ema, state = ema_ref.update(verdict, t, 0.9, True, params[k], ema, lives[k], state, SEGMENTS)
        if verdict:
            assert _bits(ema) == _bits(keep[0]) and _bits(state) == _bits(keep[1])
        seen.append((ema.copy(), state.copy()))
    # by hand, float32 operation by operation: step 1 with t = 1, step 4 with t = 2
    c1, c2 = f32(1) - f32(2) / f32(11), f32(1) - f32(3) / f32(12)
    e1 = start[0] + c1 * (params[0] - start[0])
    assert _bits(seen[0][0]) == _bits(e1) == _bits(seen[1][0]) == _bits(seen[2][0])
    e4 = e1 + c2 * (params[3] - e1)
    assert _bits(seen[3][0]) == _bits(e4)
    f = lambda s, a, b: s[a:b].view(f32)  # noqa: E731
    s1 = seen[0][1]
    assert _bits(f(s1, 0, 20)) == _bits(f(start[1], 0, 20) + c1 * (f(lives[0], 0, 20) - f(start[1], 0, 20)))
    assert _bits(f(s1, 48, 52)) == _bits(f(start[1], 48, 52) + c1 * (f(lives[0], 48, 52) - f(start[1], 48, 52)))
    assert _bits(s1[32:40]) == _bits(lives[0][32:40]) and _bits(s1[64:67]) == _bits(lives[0][64:67])  # kind 0: copied
    s4 = seen[3][1]
    assert _bits(s4[32:40]) == _bits(lives[3][32:40])  # the counter of the last APPLIED step, not of a skipped one
    assert _bits(f(s4, 0, 20)) == _bits(f(s1, 0, 20) + c2 * (f(lives[3], 0, 20) - f(s1, 0, 20)))
    for _, s in seen:
        assert not s[_padding_mask()].any()  # padding stays zero
    # the inputs are never written
    assert _bits(params[0]) == _bits(np.random.RandomState(0).randn(8).astype(f32))


@pytest.mark.parametrize("verdict", [0, 1, 2, 3])
def test_verdicts_leave_the_bits_alone_exactly_when_nonzero(verdict):
    rng = np.random.RandomState(verdict)
    p, e = rng.randn(12).astype(f32), rng.randn(12).astype(f32)
    live, state = _state(1), _state(2)
    got_e, got_s = ema_ref.update(verdict, 5, 0.5, False, p, e, live, state, SEGMENTS)
    same = _bits(got_e) == _bits(e) and _bits(got_s) == _bits(state)
    assert same == (verdict != 0)
    assert got_e is not e and got_s is not state  # new arrays either way


def test_update_edge_cases_and_refusals():
    p, e = np.ones(4, f32), np.zeros(4, f32)
    none = np.zeros(0, np.uint8)
    got, s = ema_ref.update(0, 1, 0.0, False, p, e, none, none, [])  # a model without buffers; decay 0: e = p
    assert _bits(got) == _bits(p) and s.size == 0
    got, _ = ema_ref.update(0, 1, 0.5, False, p[:0], e[:0], none, none, [])
    assert got.size == 0
    # non-finite values propagate as IEEE says
    p2 = np.array([np.inf, np.nan, 1.0, -np.inf], f32)
    got, _ = ema_ref.update(0, 3, 0.5, False, p2, np.array([1.0, 1.0, np.nan, np.inf], f32), none, none, [])
    assert np.isposinf(got[0]) and np.isnan(got[1]) and np.isnan(got[2]) and np.isnan(got[3])
    # denormals are neither flushed on the way in nor on the way out
    tiny = np.array([1, 3, 0x00400000, 0x807FFFFF], dtype=np.uint32).view(f32)
    got, _ = ema_ref.update(0, 1, 0.5, False, tiny, np.zeros(4, f32), none, none, [])
    assert got.view(np.uint32).tolist() == [0, 2, 0x00200000, 0x80400000]  # halves, ties to even
    live = _state(0)
    for bad, why in (([(8, 4, 1)], "16-byte"), ([(64, 17, 0)], "leaves"), ([(0, 20, 1), (16, 4, 1)], "overlaps"),
                     ([(0, 6, 1)], "kind"), ([(0, 4, 2)], "kind"), ([(96, 0, 0)], "leaves")):
        with pytest.raises(ValueError, match=why):
            ema_ref.update(0, 1, 0.5, True, p, e, live, live.copy(), bad)
    for decay in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            ema_ref.update(0, 1, decay, True, p, e, none, none, [])
    with pytest.raises(ValueError, match="multiple of 16"):
        ema_ref.update(0, 1, 0.5, True, p, e, live[:40], live[:40].copy(), [])


def test_swap_twice_is_the_identity_on_random_bits():
    rng = np.random.RandomState(4)
    a, b = rng.randint(0, 256, 64).astype(np.uint8), rng.randint(0, 256, 64).astype(np.uint8)
    a[:8].view(np.uint32)[:] = [0x7FC00001, 0xFFC12345]  # NaN payloads
    x, y = ema_ref.swap(a, b)
    assert _bits(x) == _bits(b) and _bits(y) == _bits(a)
    x, y = ema_ref.swap(x, y)
    assert _bits(x) == _bits(a) and _bits(y) == _bits(b)
    assert ema_ref.swap(a[:0], b[:0])[0].size == 0
    with pytest.raises(ValueError, match="multiple of 16"):
        ema_ref.swap(a[:24], b[:24])
    with pytest.raises(ValueError, match="equal size"):
        ema_ref.swap(a, b[:32])


# ---- 2. WeightAverage on host tensors -------------------------------------------------------------------------------------------
def _hyper(step):
    h = torch.zeros(8)
    h[4:5].view(torch.int32).fill_(step)
    return h


@pytest.mark.parametrize("preset", ["pn_transformer_everyday", "dgl_everyday"])
def test_averaged_state_dict_has_the_models_keys(preset):
    from multi_part_assembly_amd.pn_transformer import build_model
    torch.manual_seed(0)
    model = build_model(_tiny_cfg(preset))
    frozen_key, frozen = next((k, p) for k, p in model.named_parameters() if p.dim() > 1)
    frozen.requires_grad_(False)
    want = {k: v.clone() for k, v in model.state_dict().items()}
    flat, slab = FlatBuffers(model.parameters()), BufferSlab(model)
    avg = WeightAverage(flat, slab, 0.5, warmup=False)
    sd = avg.averaged_state_dict(model)
    assert list(sd) == list(model.state_dict()) and len(sd) > 10
    for k, v in sd.items():  # a fresh average is the model
        assert torch.equal(v, want[k]) and v.dtype == want[k].dtype and v.shape == want[k].shape, k
        assert v.data_ptr() != model.state_dict()[k].data_ptr() or v.numel() == 0  # clones
    assert any(v.dtype == torch.int64 for v in sd.values())  # num_batches_tracked is there
    # the model moves; the average follows by c = 0.5, counters are copied, the frozen parameter comes from the model
    with torch.no_grad():
        flat.flat_param.add_(1.0)
        frozen.add_(7.0)
        for name, b in model.named_buffers():
            b.add_(2)
    avg.update(_hyper(1))
    sd = avg.averaged_state_dict(model)
    for k, v in sd.items():
        if k == frozen_key:
            assert torch.equal(v, want[k] + 7.0)
        elif v.dtype == torch.int64:
            assert torch.equal(v, want[k] + 2)
        elif k in dict(model.named_buffers()):
            assert torch.equal(v, want[k] + (want[k] + 2 - want[k]) * 0.5), k
        else:
            assert torch.equal(v, want[k] + (want[k] + 1.0 - want[k]) * 0.5), k
    # a skipped step changes nothing; round trip through load_averaged_state_dict; reset; swap
    before = (avg.ema_param.clone(), avg.ema_state.clone())
    avg.update(_hyper(2), torch.tensor([1, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32))
    assert torch.equal(avg.ema_param, before[0]) and torch.equal(avg.ema_state, before[1])
    avg.reset()
    assert torch.equal(avg.ema_param, flat.flat_param) and torch.equal(avg.ema_state, slab.live)
    avg.load_averaged_state_dict(sd, model)
    assert all(torch.equal(v, sd[k]) for k, v in avg.averaged_state_dict(model).items())
    # (what a state dict does not carry keeps the reset's value: the flat buffer's alignment padding, non-persistent buffers)
    avg.ema_param.copy_(before[0]), avg.ema_state.copy_(before[1])
    with pytest.raises(KeyError, match="missing"):
        avg.load_averaged_state_dict({k: v for k, v in sd.items() if not k.endswith("running_mean")}, model)
    live = (flat.flat_param.clone(), slab.live.clone())
    ptrs = [p.data_ptr() for p in model.parameters()]
    avg.swap()
    assert avg.swapped and torch.equal(flat.flat_param, before[0]) and torch.equal(avg.ema_param, live[0])
    assert torch.equal(slab.live, before[1]) and [p.data_ptr() for p in model.parameters()] == ptrs  # views stay put
    for what in (avg.reset, lambda: avg.update(_hyper(3)), lambda: avg.averaged_state_dict(model)):
        with pytest.raises(RuntimeError, match="swapped in"):
            what()
    avg.swap()
    assert not avg.swapped and torch.equal(flat.flat_param, live[0]) and torch.equal(slab.live, live[1])
    slab.check()


def test_a_model_without_buffers_and_bad_decays():
    bare = nn.Sequential(nn.Linear(3, 3), nn.ReLU())
    flat, slab = FlatBuffers(bare.parameters()), BufferSlab(bare)
    avg = WeightAverage(flat, slab, 0.0)
    assert avg.segments == [] and avg.ema_state.numel() == 0
    with torch.no_grad():
        flat.flat_param.mul_(2.0)
    avg.update(_hyper(100))  # decay 0: the average is the weights
    assert torch.equal(avg.ema_param, flat.flat_param)
    assert list(avg.averaged_state_dict(bare)) == list(bare.state_dict())
    avg.swap(), avg.swap()
    for decay in (1.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            WeightAverage(flat, slab, decay)


# ---- 3. the entry points' refusals, without a GPU ---------------------------------------------------------------------------------
def test_entry_points_are_declared_and_refuse_bad_arguments_without_a_gpu(built):
    assert {"mpa_ema_update", "mpa_ema_swap"} <= set(_lib.declared_functions()) and _lib.ABI_VERSION == 10
    P, I64, INT, F32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    assert _lib.SIGNATURES["mpa_ema_update"] == (INT, [P, P, I64, P, P, I64, P, P, I64, P, F32, INT, P, P])
    assert _lib.SIGNATURES["mpa_ema_swap"] == (INT, [P, P, I64, P, P, I64, P])
    L = _lib.lib()
    # addresses by alignment (never dereferenced: every call below launches nothing); only the host table is read
    p, e, live, st, hyper, guard, tab_dev = 4096, 8192, 16384, 20480, 4100, 4104, 32768
    table = lambda *segs: (ctypes.c_int64 * (3 * len(segs)))(*[w for s in segs for w in s])  # noqa: E731
    good = table((0, 20, 1), (32, 8, 0))

    def update(param=p, ema=e, numel=64, live=live, state=st, nbytes=48, host=good, dev=tab_dev, nseg=2, hyper=hyper,
               decay=0.5, warmup=1, guard=guard):
        return L.mpa_ema_update(param, ema, numel, live, state, nbytes, host, dev, nseg, hyper, decay, warmup, guard, None)

    err = L.mpa_last_error
    assert update(numel=0, nbytes=0, nseg=0, param=None, ema=None, live=None, state=None, host=None, dev=None) == 0
    assert update(numel=0, nbytes=0, nseg=0, guard=None) == 0            # nothing to average: success without a launch
    assert update(numel=0, nbytes=32, nseg=1, host=table((16, 0, 0))) == 0  # only a zero-size segment
    for kw in (dict(param=None), dict(ema=None), dict(live=None), dict(state=None), dict(hyper=None), dict(host=None),
               dict(dev=None)):
        assert update(**kw) == -1 and b"null" in err(), kw
    for kw in (dict(param=p + 4), dict(ema=e + 8), dict(live=live + 4), dict(state=st + 12)):
        assert update(**kw) == -1 and b"aligned" in err(), kw
    for kw in (dict(hyper=hyper + 2), dict(guard=guard + 1), dict(dev=tab_dev + 4)):
        assert update(**kw) == -1 and b"misaligned" in err(), kw
    for numel in (-4, 3, 6):
        assert update(numel=numel) == -1 and b"multiple of 4" in err()
    for nbytes in (-16, 8, 40):
        assert update(nbytes=nbytes) == -1 and b"multiple of 16" in err()
    for decay in (1.0, 1.5, -0.25, float("nan"), float("inf")):
        assert update(decay=decay) == -1 and b"decay" in err(), decay
    assert update(ema=p + 64) == -1 and b"overlap" in err()
    assert update(state=live + 32) == -1 and b"overlap" in err()
    for host, nseg, why in ((table((8, 4, 1)), 1, b"16-byte boundary"), (table((0, 20, 1), (40, 8, 0)), 2, b"16-byte boundary"),
                            (table((32, 17, 0)), 1, b"leaves the slab"), (table((48, 0, 0), (64, 0, 0)), 2, b"leaves the slab"),
                            (table((0, 64, 0)), 1, b"leaves the slab"), (table((-16, 4, 1)), 1, b"16-byte boundary"),
                            (table((0, -4, 1)), 1, b"leaves the slab"), (table((0, 20, 1), (16, 4, 1)), 2, b"overlaps"),
                            (table((16, 4, 1), (0, 4, 1)), 2, b"overlaps"), (table((0, 6, 1)), 1, b"kind"),
                            (table((0, 4, 2)), 1, b"kind")):
        assert update(host=host, nseg=nseg) == -1 and why in err(), err()
    assert update(nseg=-1) == -1 and b"segment count" in err()
    assert update(nbytes=0, live=None, state=None) == -1 and b"leaves the slab" in err()  # segments without a slab

    def swap(a=p, b=e, ab=64, c=live, d=st, cd=32):
        return L.mpa_ema_swap(a, b, ab, c, d, cd, None)

    assert swap(ab=0, cd=0) == 0 and swap(None, None, 0, None, None, 0) == 0  # zero bytes: success without a launch
    for kw in (dict(a=None), dict(b=None), dict(c=None), dict(d=None)):
        assert swap(**kw) == -1 and b"null" in err()
    for kw in (dict(a=p + 8), dict(b=e + 4), dict(c=live + 8), dict(d=st + 2)):
        assert swap(**kw) == -1 and b"aligned" in err()
    for kw in (dict(ab=24), dict(cd=8), dict(ab=-16), dict(cd=-32)):
        assert swap(**kw) == -1 and b"multiples of 16" in err()
    for kw in (dict(b=p), dict(b=p + 48), dict(a=e + 16), dict(d=live), dict(d=live + 16), dict(c=p + 32), dict(d=e),
               dict(c=e + 48, d=st)):
        assert swap(**kw) == -1 and b"overlap" in err(), kw


# ---- 4. the Python layer's refusals, the configuration keys ---------------------------------------------------------------------------
def test_trainer_switch_configuration_and_refusals():
    from multi_part_assembly_amd.pn_transformer import build_model
    from multi_part_assembly_amd.trainer import Trainer
    off, cfg = _trainer()
    assert off.average is None and off.buffer_slab is None and off.optimizer.average is None and off.ema_decay is None
    with pytest.raises(RuntimeError, match="averaging"):
        off.evaluate([], weights="ema")
    with pytest.raises(RuntimeError, match="averaging is off"):
        with off.averaged_weights():
            pass
    with pytest.raises(ValueError, match="'live' or 'ema'"):
        off.evaluate([], weights="best")
    assert "ema" not in off.state_dict()
    on, _ = _trainer(ema_decay=0.9)
    assert on.average.decay == 0.9 and on.average.warmup is True and on.optimizer.average is on.average
    assert on.buffer_slab is not None and on.average.slab is on.buffer_slab
    assert on.guard_buffers is False and on.optimizer.guard_state is None  # the slab is NOT handed over for a rollback
    assert torch.equal(on.average.ema_param, on.flat.flat_param) and torch.equal(on.average.ema_state, on.buffer_slab.live)
    both, _ = _trainer(ema_decay=0.5, ema_warmup=False, guard_step=True, guard_buffers=True)
    assert both.optimizer.guard_state is both.buffer_slab is both.average.slab and both.average.warmup is False
    cfg.optimizer.ema_decay, cfg.optimizer.ema_warmup = 0.25, False
    from_cfg = Trainer(build_model(cfg), cfg)
    assert from_cfg.average.decay == 0.25 and from_cfg.average.warmup is False
    assert Trainer(build_model(cfg), cfg, ema_decay=0.75, ema_warmup=True).average.decay == 0.75  # the argument wins
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError, match="ema_decay"):
            _trainer(ema_decay=bad)
    # while the average is in front of the model: no step, no checkpoint; an exception inside the block swaps back
    live = on.flat.flat_param.clone()
    with torch.no_grad():
        on.average.ema_param.add_(1.0)
    with on.averaged_weights() as model:
        assert model is on.model and on.average.swapped and torch.equal(on.flat.flat_param, live + 1.0)
        with pytest.raises(RuntimeError, match="swapped in"):
            on.train_step({})
        with pytest.raises(RuntimeError, match="swapped in"):
            on.state_dict()
        with pytest.raises(RuntimeError, match="swapped in"):
            on.load_state_dict({"model": {}})
        with pytest.raises(RuntimeError, match="already"):
            with on.averaged_weights():
                pass
    assert not on.average.swapped and torch.equal(on.flat.flat_param, live)
    with pytest.raises(KeyError):
        with on.averaged_weights():
            raise KeyError("inside")
    assert not on.average.swapped and torch.equal(on.flat.flat_param, live)
    # no preset sets the keys
    with_optimizer = optimizer_presets()
    assert len(with_optimizer) >= 10
    assert all("ema_decay" not in c.optimizer and "ema_warmup" not in c.optimizer for c in with_optimizer)


# ---- 5. the launches of a step -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [None, 1.0])
def test_step_launches_switch_off_are_the_parents_and_on_is_one_more(monkeypatch, built, clip):
    """Recorded on a stub `_lib.launch` (host tensors, nothing runs)."""
    from multi_part_assembly_amd.pn_transformer import build_model
    from multi_part_assembly_amd.trainer import Trainer
    cfg = _tiny_cfg()
    cfg.optimizer.clip_grad = clip
    calls = _record(monkeypatch)
    parent = {(False, False): (["mpa_grad_clip_coef"] if clip else []) + ["mpa_adam_step_dev"],
              (True, False): ["mpa_step_guard", "mpa_adam_step_guarded"],
              (True, True): ["mpa_step_guard", "mpa_adam_step_guarded", "mpa_guard_commit"]}
    for (guard_step, guard_buffers), names_off in parent.items():
        for decay in (None, 0.99):
            t = Trainer(build_model(cfg), cfg, guard_step=guard_step, guard_buffers=guard_buffers, ema_decay=decay)
            opt = t.optimizer
            opt._hyper_dev = torch.zeros(8)  # (the device buffer of a real step)
            for _ in range(2):
                calls.clear()
                opt.step_dev()
                names = [c[0] for c in calls]
                if decay is None:
                    assert names == names_off, (guard_step, guard_buffers)
                    continue
                assert names == names_off + ["mpa_ema_update"], (guard_step, guard_buffers)
                a, avg, slab = calls[-1][1], t.average, t.buffer_slab
                assert a[0] is t.flat.flat_param and a[1] is avg.ema_param and a[2] == t.flat.numel
                assert a[3] is slab.live and a[4] is avg.ema_state and a[5] == slab.nbytes > 0
                assert list(a[6]) == a[7].tolist() == [w for s in avg.segments for w in s] and a[8] == len(slab.names)
                assert a[9] is opt._hyper_dev and a[10] == 0.99 and a[11] == 1 and len(a) == 13
                assert a[12] is (opt.guard_words() if guard_step else None)  # the guard words when guarded, NULL otherwise
                kinds = {name: s[2] for name, s in zip(slab.names, avg.segments)}
                assert all(k == (0 if n.endswith("num_batches_tracked") else 1) for n, k in kinds.items())


def test_a_bare_optimiser_takes_the_average_too(monkeypatch, built):
    calls = _record(monkeypatch)
    bare = nn.Linear(4, 2)
    flat = FlatBuffers(bare.parameters())
    opt = FusedAdam(flat, average=WeightAverage(flat, BufferSlab(bare), 0.5))
    opt._hyper_dev = torch.zeros(8)
    opt.step_dev()
    assert [c[0] for c in calls] == ["mpa_adam_step_dev", "mpa_ema_update"]
    assert calls[-1][1][5] == 0 and calls[-1][1][6] is None and calls[-1][1][8] == 0  # no slab, no table


# ---- 6. fit -------------------------------------------------------------------------------------------------------------------------
class OldStubTrainer(StubTrainer):
    """A trainer from before the average: its `evaluate` takes the batches only."""

    def evaluate(self, batches):
        self.asked.append("positional")
        return {"val/part_acc": 0.25}


def test_fit_val_weights_default_and_record():
    from multi_part_assembly_amd import fit as _fit
    run = lambda t, **kw: _fit.fit(t, StubProducer(), StubSampler(), val_batches=[1], epochs=2, val_every=2,  # noqa: E731
                                   log_every=0, **kw)
    t = StubTrainer(average=object())
    history = run(t)
    assert t.asked == ["ema"] and "val/weights" not in history[0] and history[1]["val/weights"] == "ema"
    t = StubTrainer(average=object())
    assert run(t, val_weights="live")[1]["val/weights"] == "live" and t.asked == ["live"]
    t = StubTrainer(average=None)
    assert run(t)[1]["val/weights"] == "live" and t.asked == ["live"]
    t = OldStubTrainer(average=None)
    history = run(t)
    assert t.asked == ["positional"] and history[1]["val/part_acc"] == 0.25 and history[1]["val/weights"] == "live"
    with pytest.raises(ValueError, match="needs a trainer that averages"):
        run(StubTrainer(average=None), val_weights="ema")
    with pytest.raises(ValueError, match="'live' or 'ema'"):
        run(StubTrainer(average=None), val_weights="both")


# ---- 7. checkpoints -----------------------------------------------------------------------------------------------------------------
def test_checkpoint_keys_and_load_rules(tmp_path):
    on, _ = _trainer(ema_decay=0.9, ema_warmup=False)
    with torch.no_grad():
        on.average.ema_param.mul_(0.5)
        off = next(o for n, o in zip(on.buffer_slab.names, on.buffer_slab.offsets) if n.endswith("running_var"))
        on.average.ema_state[off:off + 4].view(torch.float32).add_(3.0)
    state = on.state_dict()
    assert set(state["ema"]) == {"decay", "warmup", "model"} and state["ema"]["decay"] == 0.9 and state["ema"]["warmup"] is False
    assert list(state["ema"]["model"]) == list(state["model"])
    assert any(not torch.equal(state["ema"]["model"][k], state["model"][k]) for k in state["model"])
    torch.save(state, tmp_path / "ckpt.pt")
    state = torch.load(tmp_path / "ckpt.pt", weights_only=False)
    want = (on.average.ema_param.clone(), on.average.ema_state.clone())
    # with "ema": restored, whatever the average held before
    other, _ = _trainer(ema_decay=0.9)
    with torch.no_grad():
        other.average.ema_param.fill_(9.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        other.load_state_dict(state)
    assert torch.equal(other.average.ema_param, want[0]) and torch.equal(other.average.ema_state, want[1])
    assert torch.equal(other.flat.flat_param, on.flat.flat_param)
    # without "ema": reset to the loaded weights, with ONE warning per trainer
    no_ema = {k: v for k, v in state.items() if k != "ema"}
    with torch.no_grad():
        other.average.ema_param.fill_(9.0)
    with pytest.warns(UserWarning, match="no weight average"):
        other.load_state_dict(no_ema)
    assert torch.equal(other.average.ema_param, other.flat.flat_param)
    assert torch.equal(other.average.ema_state, other.buffer_slab.live)
    with torch.no_grad():
        other.average.ema_param.fill_(9.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        other.load_state_dict(no_ema)  # (no second warning)
        other.load_state_dict({"state_dict": state["model"]})  # Lightning-style: weights only, the average follows them
    assert torch.equal(other.average.ema_param, other.flat.flat_param)
    # a trainer without averaging ignores the key
    plain, _ = _trainer()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        plain.load_state_dict(state)
    assert plain.average is None and torch.equal(plain.flat.flat_param, on.flat.flat_param)


# ---- 8. the tools -------------------------------------------------------------------------------------------------------------------
def test_train_tool_flags():
    tool = _tool("train")
    base = ["--preset", "pn_transformer_everyday", "--synthetic"]
    args = tool.parse_args(base)
    assert args.ema is None and args.no_ema_warmup is False
    assert "ema_decay" not in tool.configure(args).optimizer and "ema_warmup" not in tool.configure(args).optimizer
    made = tool.configure(tool.parse_args(base + ["--ema", "0.99"]))
    assert made.optimizer.ema_decay == 0.99 and "ema_warmup" not in made.optimizer
    made = tool.configure(tool.parse_args(base + ["--ema", "0.5", "--no-ema-warmup"]))
    assert made.optimizer.ema_decay == 0.5 and made.optimizer.ema_warmup is False
    for bad in (["--no-ema-warmup"], ["--ema", "1.0"], ["--ema", "-0.1"], ["--ema", "nan"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)


@pytest.mark.parametrize("name", ["evaluate", "visualize"])
def test_evaluation_tools_take_the_averaged_weights(name, tmp_path):
    tool = _tool(name)
    base = ["--preset", "pn_transformer_everyday", "--data-dir", "d", "--data-fn", "f"] + (["--out", "o"] if name == "visualize" else [])
    assert tool.parse_args(base).weights == "live" and tool.parse_args(base + ["--weights", "ema"]).weights == "ema"
    with pytest.raises(SystemExit):
        tool.parse_args(base + ["--weights", "best"])
    from multi_part_assembly_amd.pn_transformer import build_model
    cfg = _tiny_cfg()
    torch.manual_seed(3)
    model = build_model(cfg)
    live = {k: v.clone() for k, v in model.state_dict().items()}
    ema = {k: (v + 1 if v.is_floating_point() else v.clone()) for k, v in live.items()}
    torch.save({"model": live, "ema": {"decay": 0.9, "warmup": True, "model": ema}, "epoch": 0, "optimizer": None},
               tmp_path / "with.pt")
    torch.save({"model": live, "epoch": 0, "optimizer": None}, tmp_path / "without.pt")
    load = tool.load_weights if name == "evaluate" else lambda m, *a: tool.load_checkpoint(m, cfg, *a)
    load(model, str(tmp_path / "with.pt"), "cpu", "ema")
    assert all(torch.equal(v, ema[k]) for k, v in model.state_dict().items())
    load(model, str(tmp_path / "with.pt"), "cpu", "live")
    assert all(torch.equal(v, live[k]) for k, v in model.state_dict().items())
    load(model, str(tmp_path / "with.pt"), "cpu")
    assert all(torch.equal(v, live[k]) for k, v in model.state_dict().items())
    with pytest.raises(SystemExit, match="holds no weight average"):
        load(model, str(tmp_path / "without.pt"), "cpu", "ema")
    torch.save(live, tmp_path / "bare.pt")
    with pytest.raises(SystemExit, match="holds no weight average"):
        load(model, str(tmp_path / "bare.pt"), "cpu", "ema")
