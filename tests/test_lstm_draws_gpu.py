"""B-LSTM with its draws on the device (`cfg.model.lstm_draws = "device"`), on the GPU: csrc/seq2seq_draw.hip against the
numpy restatement (multi_part_assembly_amd/seq2seq_draw_ref.py), the decoder launch that reads the coin from device
memory against the entry point that is told the mode, device mode against host mode on the same draws, the captured step
against eager launches (geometric and semantic presets), the position of the draw stream across evaluation passes and
checkpoints, and the absence of host-to-device copies in a forward."""
import os
import random
import sys

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import param_fill  # noqa: E402

from anchored import err  # noqa: E402
from multi_part_assembly_amd import _lib, config, gru, lstm, matching, regressor, synthetic  # noqa: E402
from multi_part_assembly_amd import seq2seq_draw_ref as ref  # noqa: E402
from multi_part_assembly_amd.pn_transformer import build_model  # noqa: E402
from multi_part_assembly_amd.trainer import Trainer  # noqa: E402

pytestmark = pytest.mark.gpu

_U64 = 0xFFFFFFFFFFFFFFFF
H, C, Z = 528, 128, 256


# ---- 1. the draw ------------------------------------------------------------------------------------------------------------
def _raw_draw(dev, B, T, p, ratio, training, seed, counter=0, counter_dev=None, salt=0):
    """One launch into outputs pre-filled with sentinels (NaN, -7): whatever survives was not written."""
    noise = torch.full((B, 16), float("nan"), device=dev)
    teacher = torch.full((1,), -7, dtype=torch.int32, device=dev)
    mask = torch.full((T, B, C), float("nan"), device=dev) if training else None
    _lib.launch("mpa_seq2seq_draw", dev, B, T, float(p), float(ratio), seed & _U64, counter & _U64, counter_dev, salt & _U64,
                noise, teacher, mask)
    return noise, teacher, mask


@pytest.mark.parametrize("B,T,p,training", [(1, 1, 0.2, True), (3, 8, 0.2, True), (64, 20, 0.2, True), (1, 1, 0.0, True),
                                            (3, 8, 0.0, True), (64, 20, 0.0, True), (3, 8, 0.2, False)])
def test_draw_equals_the_restatement(cuda_device, capsys, B, T, p, training):
    """Coin and mask bit for bit; the normals against the float64 restatement within 8 x the error the same formulas have
    in numpy float32 against float64 on the same words (never the kernel's own output), at most 1e-5."""
    word = torch.zeros(1, dtype=torch.int64, device=cuda_device)
    worst = (0.0, 0.0, 0.0, 0)
    for seed, counter, salt, ratio in ((0x1234567890ABCDEF, 0, 0, 0.5), (77, 1, 3 * matching.SALT_STEP, 0.5),
                                       (77, (1 << 32) + 5, 0, 0.3), (5, (1 << 62) | 2, matching.SALT_STEP, 1.0),
                                       (5, 9, 0, 0.0)):
        want_noise, want_teacher, want_mask = ref.draw(B, T, p, ratio, training, seed, counter, salt)
        noise, teacher, mask = _raw_draw(cuda_device, B, T, p, ratio, training, seed, counter, None, salt)
        word.fill_(counter)
        by_word = _raw_draw(cuda_device, B, T, p, ratio, training, seed, 12345, word, salt)  # the word wins over the value
        wrapped = lstm.draw(B, T, p, ratio, training, seed=seed, counter=counter, salt=salt, device=cuda_device)
        for other in (by_word, wrapped):
            assert torch.equal(other[0], noise) and torch.equal(other[1], teacher)
            assert (other[2] is None and mask is None) if not training else torch.equal(other[2], mask)
        assert teacher.dtype == torch.int32 and teacher.cpu().numpy().tolist() == want_teacher.tolist(), (seed, counter)
        if training:
            assert np.array_equal(mask.cpu().numpy(), want_mask), (seed, counter)  # (a surviving NaN sentinel fails this)
        else:
            assert want_mask is None
        got = noise.cpu().numpy()
        assert np.isfinite(got).all()
        e32 = err(ref.noise(B, seed, counter, salt, dtype=np.float32), want_noise)
        bar = min(8.0 * e32, 1e-5)
        mine = err(got, want_noise)
        worst = max(worst, (mine / bar, mine, e32, counter))
        assert mine <= bar, (seed, counter, mine, e32, bar)
    with capsys.disabled():
        print(f"\n  draw B={B} T={T} p={p} training={training}: noise vs float64, closest to its bar: {worst[1]:.2e} (numpy "
              f"float32 {worst[2]:.2e}, bar {min(8.0 * worst[2], 1e-5):.2e}; counter {worst[3]:#x})", end="")


# ---- 2. the decoder launch that reads the coin ---------------------------------------------------------------------------
def _decoder_case(dev, B, P, seed):
    torch.manual_seed(seed)
    s2s = lstm.Seq2Seq(128, 128, 256)
    param_fill.fill_parameters(s2s, seed + 11)
    s2s = s2s.to(dev)
    d = s2s.decoder
    weights = [d.gru.weight_ih_l0, d.gru.bias_ih_l0, d.gru.weight_hh_l0, d.gru.bias_hh_l0, d.linear1[0].weight,
               d.linear1[0].bias, d.linear1[2].weight, d.linear1[2].bias]
    weights = [w.detach().contiguous() for w in weights]
    g = torch.Generator().manual_seed(seed + 5)
    gi = (0.5 * torch.randn(P, B, 3 * H, generator=g)).to(dev)
    h0 = (0.5 * torch.randn(B, H, generator=g)).to(dev)
    mask = ((torch.rand(P, B, C, generator=g) > 0.2).float() / 0.8).to(dev)
    dh = torch.randn(P, B, H, generator=g).to(dev)
    return weights, gi, h0, mask, dh


def _run_decoder(dev, name, gi, mask, teacher, h0, weights, dh, B, P):
    """Forward by entry point `name`, then the backward on its workspace -> every output of both."""
    ws = torch.zeros(_lib.query("mpa_seq2seq_decoder_workspace", B, P), dtype=torch.float32, device=dev)
    hs, z1, y = (torch.full((P, B, n), float("nan"), device=dev) for n in (H, Z, C))
    word, host = gru._status(dev)
    if name == "mpa_seq2seq_decoder_forward_sel":
        _lib.launch(name, dev, gi, mask, teacher, h0, *weights, B, P, ws, hs, z1, y, word)
    else:
        _lib.launch(name, dev, gi, mask, h0, *weights, B, P, ws, hs, z1, y, word)
    host.copy_(word, non_blocking=True)
    gru.raise_if_failed(dev, synchronize=True)  # the status word is clean
    dgi = torch.full((P, B, 3 * H), float("nan"), device=dev)
    dwhh, dbhh, dh0 = torch.empty_like(weights[2]), torch.empty(3 * H, device=dev), torch.empty(B, H, device=dev)
    _lib.launch("mpa_seq2seq_decoder_backward", dev, dh, h0, weights[2], hs, B, P, ws, dgi, dwhh, dbhh, dh0, word)
    host.copy_(word, non_blocking=True)
    gru.raise_if_failed(dev, synchronize=True)
    return {"hs": hs, "z1": z1, "y": y, "dgi": dgi, "dwhh": dwhh, "dbhh": dbhh, "dh0": dh0}


@pytest.mark.parametrize("B,P", [(1, 20), (3, 8), (64, 20), (4, 1)])
def test_sel_launch_equals_the_entry_point_that_is_told_the_mode(cuda_device, B, P):
    dev = cuda_device
    assert lstm._decoder_resident(B)
    weights, gi, h0, mask, dh = _decoder_case(dev, B, P, seed=B + P)
    gru.prepare(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    runs = {}
    for coin in (1, 0):
        flag.fill_(coin)
        runs[coin] = _run_decoder(dev, "mpa_seq2seq_decoder_forward_sel", gi, mask, flag, h0, weights, dh, B, P)
        want = _run_decoder(dev, "mpa_seq2seq_decoder_forward", gi if coin else None, None if coin else mask, None, h0,
                            weights, dh, B, P)
        for k, v in want.items():
            assert torch.isfinite(v).all(), (coin, k)
            assert torch.equal(runs[coin][k], v), (coin, k)
    if P > 1:  # the two modes are two different computations
        assert not torch.equal(runs[0]["y"], runs[1]["y"])


# ---- 3. device mode = host mode on the same draws --------------------------------------------------------------------------
@pytest.mark.parametrize("coin", [1, 0], ids=["teacher", "free"])
def test_device_mode_equals_host_mode_on_the_same_draws(cuda_device, monkeypatch, coin):
    dev, B, P, seed = cuda_device, 3, 8, 31
    ratio = float(coin)  # ratio 1 always forces, ratio 0 never: both outcomes without hunting for a counter
    torch.manual_seed(seed)
    host = lstm.Seq2Seq(128, 128, 256)
    param_fill.fill_parameters(host, seed + 11)
    devm = lstm.Seq2Seq(128, 128, 256, draws="device")
    devm.load_state_dict(host.state_dict())
    host, devm = host.to(dev).train(), devm.to(dev).train()
    g = torch.Generator().manual_seed(seed + 5)
    x = torch.randn(P, B, 128, generator=g).to(dev)
    valids = (torch.arange(P)[None] < torch.tensor([8, 3, 1])[:, None]).float().to(dev)
    x = x * valids.t()[..., None]
    gout = torch.randn(P, B, 128, generator=g).to(dev)
    counter = devm.draw_counter
    counter.begin_step(True)
    args = {"seed": torch.initial_seed() & _U64, "counter": counter._current, "salt": 0}
    noise, teacher, mask = lstm.draw(B, P, devm.decoder.dropout_i, ratio, True, device=dev, **args)
    assert int(teacher) == coin
    noise_host = noise.cpu().numpy().reshape(1, B, 16)
    monkeypatch.setattr(np.random, "normal", lambda loc=0.0, scale=1.0, size=None: noise_host.astype(np.float64))
    monkeypatch.setattr(random, "random", lambda: 0.0 if coin else 1.0)
    out = {}
    for name, mod, kw in (("device", devm, {}), ("host", host, {"masks": mask})):
        xi = x.clone().requires_grad_(True)
        y, _ = mod(xi, xi.detach(), valids=valids, teacher_forcing_ratio=ratio, **kw)
        (y * gout).sum().backward()
        grads = {k: p.grad for k, p in mod.named_parameters() if p.grad is not None}
        grads["input"] = xi.grad
        out[name] = (y.detach(), grads)
    gru.raise_if_failed(dev, synchronize=True)
    assert torch.equal(out["device"][0], out["host"][0])
    assert sorted(out["device"][1]) == sorted(out["host"][1]) and len(out["host"][1]) > 8
    for k, v in out["host"][1].items():
        assert torch.equal(out["device"][1][k], v), k


# ---- 4. capture, evaluation passes, checkpoints ----------------------------------------------------------------------------
def _seed_with_both_coins(steps=4, ratio=0.5):
    """A seed (chosen with the restatement, on the CPU) whose first `steps` training steps contain both coin values."""
    for seed in range(3, 64):
        coins = [int(ref.teacher(ratio, seed, counter)[0]) for counter in range(1, steps + 1)]
        if 0 in coins[1:] and 1 in coins[1:]:  # both among the replays, not only in the eager warm-up step
            return seed, coins
    raise AssertionError("no seed below 64 gives both coin values")


def _trainer(preset, dev, seed, **kw):
    cfg = getattr(config, preset)()
    cfg.model.lstm_draws = "device"
    cfg.data.max_num_part = 8
    if cfg.data.dataset != "geometry":
        cfg.loss.match_sample = "device"
    torch.manual_seed(seed)
    model = build_model(cfg).to(dev)
    return Trainer(model, cfg, **kw)


def _batch(preset, step, dev):
    if preset == "lstm_partnet_chair":
        batch = synthetic.make_partnet_like_batch(3, 8, 128, seed=70 + step, device=dev)
        batch.pop("num_parts")
        return batch
    return synthetic.make_batch(3, max_parts=8, num_points=128, seed=70 + step, device=dev)


@pytest.fixture
def pinned_noise(monkeypatch):
    """The pose regressor's noise as one fixed tensor per shape (eager launches draw it on the CPU generator, a capture on
    the device generator: two streams by design; tests/test_semantic_device_gpu.py pins it the same way)."""
    fixed = {}

    def forward(self, x):
        if self.noise_dim == 0:
            return regressor.PoseRegressor.forward(self, x)
        key = (tuple(x.shape[:-1]), self.noise_dim)
        if key not in fixed:
            g = torch.Generator().manual_seed(11)
            fixed[key] = torch.randn(*key[0], self.noise_dim, generator=g).to(x.device)
        return regressor.PoseRegressor.forward(self, torch.cat([x, fixed[key]], dim=-1))

    monkeypatch.setattr(regressor.StocasticPoseRegressor, "forward", forward)


@pytest.fixture
def recorded_draws(monkeypatch):
    """Every (noise, teacher, mask) that eager launches of `lstm.draw` return, in call order."""
    calls, real = [], lstm.draw

    def draw(*a, **kw):
        out = real(*a, **kw)
        if not torch.cuda.is_current_stream_capturing():
            calls.append(out)
        return out

    monkeypatch.setattr(lstm, "draw", draw)
    return calls


@pytest.mark.parametrize("preset", ["lstm_everyday", "lstm_partnet_chair"])
def test_captured_step_equals_eager_steps(cuda_device, pinned_noise, recorded_draws, preset):
    """The whole B-LSTM step as ONE HIP graph — a capture that succeeds has no host draw left in it — walks the eager
    trajectory to the last bit over 4 steps on 4 batches that contain both outcomes of the coin."""
    seed, coins = _seed_with_both_coins()
    eager = _trainer(preset, cuda_device, seed)
    n_iter = eager.model.sample_iter
    assert n_iter == (5 if preset == "lstm_partnet_chair" else 1)
    eager_losses = []
    for step in range(4):
        eager_losses.append(float(eager.train_step(_batch(preset, step, cuda_device))))
    drawn = list(recorded_draws)
    assert len(drawn) == 4 * n_iter
    assert [int(d[1]) for d in drawn[::n_iter]] == coins and set(coins) == {0, 1}  # the first forward of every step
    for step in range(4):  # the forwards of one step use different draws, and so do the steps
        noises = [d[0] for d in drawn[step * n_iter:(step + 1) * n_iter]]
        assert all(not torch.equal(noises[i], noises[j]) for i in range(n_iter) for j in range(i))
    assert not torch.equal(drawn[0][0], drawn[n_iter][0]) and not torch.equal(drawn[0][2], drawn[n_iter][2])
    graph = _trainer(preset, cuda_device, seed, use_graph=True, graph_warmup=1)
    assert graph.use_graph is True
    for step in range(4):
        lg = float(graph.train_step(_batch(preset, step, cuda_device)))
        assert lg == eager_losses[step], (step, lg, eager_losses[step])
    assert graph._graph is not None and np.isfinite(eager_losses).all()
    assert torch.equal(graph.flat.flat_param, eager.flat.flat_param)
    assert eager.model.draw_counter._calls == graph.model.draw_counter._calls == 4
    graph.check_health(synchronize=True)


def test_draws_move_with_the_step_not_with_evaluation(cuda_device, recorded_draws):
    seed, preset = 5, "lstm_everyday"
    batch = _batch(preset, 0, cuda_device)
    plain = _trainer(preset, cuda_device, seed)
    for _ in range(2):
        plain.train_step(dict(batch))
    assert len(recorded_draws) == 2 and not torch.equal(recorded_draws[0][0], recorded_draws[1][0])  # same batch, new noise
    with_val = _trainer(preset, cuda_device, seed)
    with_val.train_step(dict(batch))
    with_val.model.eval()
    with torch.no_grad():
        for _ in range(2):
            with_val.model.validation_step(dict(batch))
    assert recorded_draws[-1][2] is None  # no mask outside training; noise and coin are drawn all the same
    assert not torch.equal(recorded_draws[-1][0], recorded_draws[-2][0])
    assert with_val.model.draw_counter._calls == 1 and with_val.model.draw_counter._eval_calls == 2
    with_val.train_step(dict(batch))
    assert torch.equal(recorded_draws[-1][0], recorded_draws[1][0])
    assert torch.equal(with_val.flat.flat_param, plain.flat.flat_param)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "captured"])
def test_checkpoint_round_trip_continues_the_draw_stream(cuda_device, use_graph):
    seed, preset = 7, "lstm_everyday"
    kw = {"use_graph": True, "graph_warmup": 1} if use_graph else {}
    full = _trainer(preset, cuda_device, seed, **kw)
    for step in range(2):
        full.train_step(_batch(preset, step, cuda_device))
    state = full.state_dict()
    assert state["dropout_calls"] == [2]
    state = {k: (v.copy() if isinstance(v, dict) else v) for k, v in state.items()}
    state["model"] = {k: v.clone() for k, v in state["model"].items()}
    want = float(full.train_step(_batch(preset, 2, cuda_device)))
    resumed = _trainer(preset, cuda_device, seed, **kw)
    resumed.load_state_dict(state)
    assert resumed.model.draw_counter._calls == 2
    got = float(resumed.train_step(_batch(preset, 2, cuda_device)))
    assert got == want
    assert torch.equal(resumed.flat.flat_param, full.flat.flat_param)


# ---- 5. no host traffic ------------------------------------------------------------------------------------------------------
class _HostCopies(TorchDispatchMode):
    """Counts the aten copies whose source is a CPU tensor and whose destination is not."""

    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = func.overloadpacket.__name__
        if name == "_to_copy" and not args[0].is_cuda and kwargs.get("device") is not None \
                and torch.device(kwargs["device"]).type == "cuda":
            self.n += 1
        if name == "copy_" and args[0].is_cuda and not args[1].is_cuda:
            self.n += 1
        return func(*args, **kwargs)


def _host_copies_per_forward(dev, draws):
    s2s = lstm.Seq2Seq(128, 128, 256, draws=draws).to(dev).train()
    x = torch.randn(8, 4, 128, device=dev, requires_grad=True)
    valids = torch.ones(4, 8, device=dev)
    for _ in range(2):
        with _HostCopies() as c:
            y, _ = s2s(x, x.detach(), valids=valids)
    return c.n


def test_no_host_to_device_copy_in_a_device_mode_forward(cuda_device):
    assert _host_copies_per_forward(cuda_device, "host") >= 1  # the noise: the counter sees what it is there to see
    assert _host_copies_per_forward(cuda_device, "device") == 0
