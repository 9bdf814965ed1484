"""B-LSTM's device-side draws without a GPU: the numpy restatement of `mpa_seq2seq_draw` (multi_part_assembly_amd/
seq2seq_draw_ref.py, the oracle of tests/test_lstm_draws_gpu.py) — its Philox against the plain-int one, the statistics of
coin, mask and noise — the `cfg.model.lstm_draws` key, and the argument contract of the two new entry points."""
import ctypes

import numpy as np
import pytest
import torch

from multi_part_assembly_amd import _build, _lib, config, lstm, matching, seq2seq_draw_ref as ref
from multi_part_assembly_amd.pn_transformer import build_model
from tool_loader import load_tool
from test_mesh_store import philox4x32_10

LSTM_PRESETS = ("lstm_everyday", "lstm_artifact", "lstm_partnet_chair")


@pytest.fixture(scope="module")
def built():
    return _build.build()


# ---- 1. the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,counter,salt,i", [(0, 0, 0, 0), (7, 1, 5, 3), ((3 << 32) | 9, (1 << 32) + 5, matching.SALT_STEP, 255),
                                                 (2 ** 64 - 1, 2 ** 64 - 1, 2, 63)])
def test_words_follow_the_documented_counter_layout(seed, counter, salt, i):
    """Block i of a kind = Philox4x32-10 with counter (i, TAG | kind, c low, c high), c = counter + salt mod 2^64, and key
    (seed low, seed high): against the plain-int Philox of tests/test_mesh_store.py (which reproduces the published
    vectors), as tests/test_epoch_sampler.py holds the epoch order to it."""
    c = (counter + salt) & 0xFFFFFFFFFFFFFFFF
    assert ref.step_value(counter, salt) == c
    for kind in (ref.KIND_TEACHER, ref.KIND_NOISE, ref.KIND_MASK):
        want = philox4x32_10([i, 0x73320000 | kind, c & 0xFFFFFFFF, c >> 32], [seed & 0xFFFFFFFF, seed >> 32])
        assert [int(w) for w in ref.words(kind, 256, seed, counter, salt)[i]] == want
    assert ref.TAG == 0x73320000  # the mesh sampler: < 4; matching: 0x6D61xxxx; PartNet: 0x706Exxxx; epoch order: 0x6570xxxx


def test_published_philox_vector():
    """Random123's known answer for Philox4x32-10 at counter = key = all ones."""
    got = ref.philox4x32_10(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    assert [int(w) for w in got] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert [int(w) for w in got] == philox4x32_10([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2)


def test_coin():
    """ratio 1 always forces, ratio 0 never; at 0.5 the count over 4096 consecutive counters is a Binomial(4096, 1/2):
    sigma = 32, within 5 sigma of 2048 (fixed seed: deterministic).  The integer comparison is the float32 one."""
    seed = 20240607
    for counter in range(64):
        assert int(ref.teacher(1.0, seed, counter)[0]) == 1 and int(ref.teacher(0.0, seed, counter)[0]) == 0
    coins = np.array([int(ref.teacher(0.5, seed, counter)[0]) for counter in range(4096)])
    assert set(coins.tolist()) == {0, 1}
    assert abs(int(coins.sum()) - 2048) <= 5 * 32, int(coins.sum())
    assert ref.teacher(0.5, seed, 3).dtype == np.int32 and ref.teacher(0.5, seed, 3).shape == (1,)
    for counter, ratio in ((0, 0.5), (1, 0.3), (2, 0.9999999), (3, 1e-8)):
        w = int(ref.words(ref.KIND_TEACHER, 1, seed, counter)[0, 0])
        u = np.float32(w >> 8) * np.float32(2.0 ** -24)
        assert int(ref.teacher(ratio, seed, counter)[0]) == int(u < np.float32(ratio))


def test_mask():
    """p = 0.2 over [20, 64, 128]: n = 163 840 Bernoulli(0.8) elements, sigma of the kept fraction = sqrt(0.16 / n)."""
    T, B, p = 20, 64, 0.2
    m = ref.mask(T, B, p, seed=5, counter=9, salt=matching.SALT_STEP)
    assert m.shape == (T, B, 128) and m.dtype == np.float32
    keep = np.float32(1) / (np.float32(1) - np.float32(0.2))
    assert set(np.unique(m).tolist()) == {0.0, float(keep)}
    n = m.size
    assert abs(float((m != 0).mean()) - 0.8) <= 5 * np.sqrt(0.8 * 0.2 / n)
    # the integer comparison is the float32 one, element e = word e % 4 of block e // 4
    w = ref.words(ref.KIND_MASK, n // 4, 5, 9, matching.SALT_STEP).reshape(-1)
    u = (w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    assert np.array_equal(m.reshape(-1) != 0, u >= np.float32(p))
    assert np.array_equal(ref.mask(3, 2, 0.0, seed=1), np.ones((3, 2, 128), np.float32))  # p = 0 keeps everything, unscaled


def test_noise():
    """64 x 16 normals for each of 64 counters: |mean| < 5 / sqrt(n), |var - 1| < 5 sqrt(2 / n); no two (counter, salt)
    streams are equal."""
    seed = 77
    rows = [ref.noise(64, seed, counter) for counter in range(64)]
    x = np.stack(rows)
    assert x.shape == (64, 64, 16) and x.dtype == np.float64 and np.isfinite(x).all()
    n = x.size
    assert abs(float(x.mean())) < 5 / np.sqrt(n)
    assert abs(float(x.var()) - 1.0) < 5 * np.sqrt(2.0 / n)
    streams = rows + [ref.noise(64, seed, 0, salt=k * matching.SALT_STEP) for k in range(1, 5)] + [ref.noise(64, seed + 1, 0)]
    flat = {s.tobytes() for s in streams}
    assert len(flat) == len(streams)
    u1, u2 = ref.noise_uniforms(64, seed, 3)
    assert u1.min() > 0.0 and u1.max() < 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
    # the float32 evaluation of the same formulas (the yardstick of the GPU test's bar) is close to the float64 one
    x32 = ref.noise(64, seed, 3, dtype=np.float32)
    assert x32.dtype == np.float32 and np.abs(x32 - rows[3]).max() / np.abs(rows[3]).max() < 1e-5


def test_draw_refuses_what_the_kernel_refuses():
    for B, T, p in ((0, 5, 0.2), (65, 5, 0.2), (3, 0, 0.2), (3, 4097, 0.2), (3, 5, 1.0), (3, 5, -0.1)):
        with pytest.raises(ValueError):
            ref.draw(B, T, p, 0.5, True)
    noise, coin, mask = ref.draw(3, 5, 0.2, 0.5, False, seed=1)
    assert noise.shape == (3, 16) and coin.shape == (1,) and mask is None
    assert ref.draw(3, 5, 0.2, 0.5, True, seed=1)[2].shape == (5, 3, 128)


# ---- 2. the configuration key ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", LSTM_PRESETS)
def test_lstm_draws_key(preset):
    cfg = getattr(config, preset)()
    assert "lstm_draws" not in cfg.model  # the presets stay on host draws
    torch.manual_seed(0)
    host = build_model(cfg)
    assert host.lstm_draws == "host" and host.host_draws_per_forward is True and host.draw_counter is None
    assert not [m for m in host.modules() if hasattr(m, "advance_seed")]
    cfg = getattr(config, preset)()
    cfg.model.lstm_draws = "device"
    torch.manual_seed(0)
    dev = build_model(cfg)
    assert dev.lstm_draws == "device" and dev.host_draws_per_forward is False
    assert list(dev.state_dict().keys()) == list(host.state_dict().keys())
    counter = dev.draw_counter
    assert isinstance(counter, matching.MatchSampler) and not list(counter.parameters()) and not list(counter.buffers())
    assert counter in list(dev.modules())  # where Trainer looks for advance_seed / prepare_streams
    cfg.model.lstm_draws = "gpu"
    with pytest.raises(ValueError, match="lstm_draws"):
        build_model(cfg)


def test_counter_follows_the_match_sampler_protocol():
    c = lstm.DrawCounter()
    cpu = torch.device("cpu")
    torch.manual_seed(123)
    c.begin_step(True)
    first = [c.draw_args(cpu) for _ in range(3)]
    assert [a["counter"] for a in first] == [1, 1, 1] and all(a["seed"] == 123 for a in first)
    assert [a["salt"] for a in first] == [(k * matching.SALT_STEP) & 0xFFFFFFFFFFFFFFFF for k in range(3)]
    c.begin_step(False)  # an evaluation pass: a stream of its own, the training stream does not move
    assert c.draw_args(cpu) == {"seed": 123, "salt": 0, "counter": (1 << 62) | 1} and c._calls == 1
    c.begin_step(True)
    assert c.draw_args(cpu)["counter"] == 2
    c.advance_seed()
    assert c._calls == 3


def test_device_mode_never_falls_back_to_host_draws():
    cfg = config.lstm_everyday()
    cfg.model.lstm_draws = "device"
    cfg.data.max_num_part = 4
    torch.manual_seed(0)
    model = build_model(cfg)
    x = torch.zeros(4, 2, 128)
    with pytest.raises(RuntimeError, match="lstm_draws"):
        model.seq2seq(x, x, valids=torch.ones(2, 4))
    with pytest.raises(RuntimeError, match="HIP device only"):
        lstm.draw(2, 4, 0.2, 0.5, True, device="cpu")


def test_train_tool_takes_the_key():
    mod = load_tool("train")
    args = mod.parse_args(["--preset", "lstm_everyday", "--synthetic", "--lstm-draws", "device"])
    assert args.lstm_draws == "device"
    assert mod.parse_args(["--preset", "lstm_everyday", "--synthetic"]).lstm_draws is None


# ---- 3. the entry points without a GPU --------------------------------------------------------------------------------------
def test_abi_declares_the_entry_points():
    declared = _lib.declared_functions()
    for name, nargs in (("mpa_seq2seq_draw", 12), ("mpa_seq2seq_decoder_forward_sel", 20)):
        assert name in declared and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert len(_lib.SIGNATURES["mpa_seq2seq_decoder_forward_sel"][1]) == len(_lib.SIGNATURES["mpa_seq2seq_decoder_forward"][1]) + 1
    assert _lib.ABI_VERSION == 10


def test_entry_points_validate_without_a_gpu(built):
    L = _lib.lib()
    one = ctypes.c_void_p(8)  # a non-null pointer that validation never dereferences

    def call(B, T, p, noise=one, teacher=one, mask=one):
        return L.mpa_seq2seq_draw(B, T, p, 0.5, 1, 0, None, 0, noise, teacher, mask, None)

    assert call(0, 5, 0.2) == -1 and b"B=0" in L.mpa_last_error()
    assert call(65, 5, 0.2) == -1 and b"B=65" in L.mpa_last_error()
    assert call(3, 0, 0.2) == -1 and b"T=0" in L.mpa_last_error()
    assert call(3, 4097, 0.2) == -1
    assert call(3, 4097, 0.2, mask=None) == -1  # T is checked with or without a mask
    assert call(3, 5, 1.0) == -1 and b"p=1" in L.mpa_last_error()
    assert call(3, 5, -0.5) == -1
    assert call(3, 5, float("nan")) == -1
    assert call(3, 5, 0.2, noise=None) == -1 and b"null" in L.mpa_last_error()
    assert call(3, 5, 0.2, teacher=None) == -1

    def sel(B, T, gi=one, teacher=one, rest=one):
        return L.mpa_seq2seq_decoder_forward_sel(gi, one, teacher, *([rest] * 9), B, T, rest, rest, rest, rest, None, None)

    assert sel(3, 5, gi=None) == -1 and b"null" in L.mpa_last_error()
    assert sel(3, 5, teacher=None) == -1
    assert sel(65, 5) == -1 and b"batch" in L.mpa_last_error()
    assert sel(3, 0) == -1
    assert sel(3, 5, rest=None) == -1 and b"null" in L.mpa_last_error()
