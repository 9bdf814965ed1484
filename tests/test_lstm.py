"""B-LSTM (multi_part_assembly_amd/lstm.py) on the CPU: the registry and presets, the library path of the seq2seq module
against the reference's own seq2seq calls recorded in the fixtures (tests/golden/make_golden_lstm.py: teacher forcing,
free running, and the semantic min-of-5 step with its seeded coins), the dead half, the host draws in eval mode and
the graph-mode guard.  The encoder and loss of the whole step are HIP-only: tests/test_lstm_gpu.py checks the full step
(loss terms included) on the GPU."""
import os
import random
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import param_fill  # noqa: E402

from multi_part_assembly_amd import config  # noqa: E402
from multi_part_assembly_amd.pn_transformer import build_model  # noqa: E402

# fixture -> (preset, forced teacher-forcing ratio: 1.0 teacher, 0.0 free running, None the seeded coin)
CASES = {
    "lstm_step_tf": (config.lstm_everyday, 1.0),
    "lstm_step_free": (config.lstm_everyday, 0.0),
    "lstm_semantic_step": (config.lstm_partnet_chair, None),
}
DEAD = ("seq2seq.encoder.rnn.gru.", "_l1"), ("seq2seq.decoder.gru.", "_l1"), ("seq2seq.decoder.linear3.", "")


def _dead(name):
    return any(name.startswith(p) and (s == "" or name.endswith(s) or (s + "_") in name) for p, s in DEAD)


def _model(name, z):
    cfg = CASES[name][0]()
    cfg.data.max_num_part = 5
    seed = int(z["seed"][0])
    torch.manual_seed(seed)
    model = build_model(cfg)
    param_fill.fill_parameters(model, seed)
    model.seq2seq.decoder.dropout_i = 0
    return model, seed


def _replay(name, z):
    """The reference's seq2seq calls of the fixture's step, on the library path: -> (model, outputs, input grad)."""
    model, seed = _model(name, z)
    s2s = model.seq2seq.train()
    ratio = CASES[name][1]
    np.random.seed(seed + 1)
    random.seed(seed + 1)
    x = torch.from_numpy(z["tap.in"].copy()).requires_grad_(True)
    valids = torch.from_numpy(z["data.part_valids"].copy())
    outs, total = [], 0.0
    for i in range(len(z["tap.coin"])):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out, stop = s2s(x, x.detach(), valids=valids, teacher_forcing_ratio=ratio)
        assert stop is None
        outs.append(out)
        total = total + (out * torch.from_numpy(z[f"tap.gout.{i}"].copy())).sum()
    total.backward()
    return model, outs, x.grad


def test_presets_build_with_the_reference_keys(golden):
    for name, (preset, _) in CASES.items():
        z = golden(name)
        cfg = preset()
        cfg.data.max_num_part = 5
        model = build_model(cfg)
        assert sorted(model.state_dict().keys()) == [str(n) for n in z["names"]], name
    assert config.lstm_partnet_chair().data.shuffle_parts is True
    assert config.lstm_artifact().model.name == "lstm"


@pytest.mark.parametrize("name", sorted(CASES))
def test_library_seq2seq_matches_the_reference_calls(golden, name):
    z = golden(name)
    model, outs, gin = _replay(name, z)
    assert len(outs) == len(z["tap.coin"])
    for i, out in enumerate(outs):
        ref = z[f"tap.out.{i}"]
        err = np.abs(out.detach().numpy() - ref).max() / np.abs(ref).max()
        assert err < 1e-5, (name, i, err)
    ref = z["tap.gin"]
    assert np.abs(gin.numpy() - ref).max() / np.abs(ref).max() < 1e-4
    record = dict(z)
    checked = 0
    for k, p in model.named_parameters():
        if not k.startswith("seq2seq.") or _dead(k):
            continue
        assert p.grad is not None, k
        param_fill.compare(record, "grad.", k, p.grad.numpy(), 1e-4)
        checked += 1
    assert checked == 16  # encoder layer 0 (both directions), decoder layer 0, linear1


@pytest.mark.parametrize("name", sorted(CASES))
def test_dead_half_gets_no_gradient(golden, name):
    z = golden(name)
    model, _, _ = _replay(name, z)
    dead = sorted([str(n) for n in z["grad_none"]] + [str(n) for n in z["grad_zero"]])
    assert dead == sorted(k for k, _ in model.named_parameters() if _dead(k))
    for k, p in model.named_parameters():
        if _dead(k):
            assert p.grad is None or not bool(p.grad.any()), k


def test_eval_mode_still_draws_the_coin_and_the_noise(golden):
    z = golden("lstm_step_tf")
    model, seed = _model("lstm_step_tf", z)
    s2s = model.seq2seq.eval()
    x = torch.from_numpy(z["tap.in"].copy())
    valids = torch.from_numpy(z["data.part_valids"].copy())
    np.random.seed(7)
    random.seed(7)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with torch.no_grad():
            s2s(x, x, valids=valids)
    after = (np.random.normal(size=3), random.random())
    np.random.seed(7)
    random.seed(7)
    np.random.normal(size=[2, x.shape[1], 16])
    random.random()
    assert np.array_equal(after[0], np.random.normal(size=3)) and after[1] == random.random()


def test_stop_signs_only_when_asked(golden):
    z = golden("lstm_step_tf")
    model, _ = _model("lstm_step_tf", z)
    x = torch.from_numpy(z["tap.in"].copy())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out, stop = model.seq2seq(x, x, return_stop_signs=True)
    assert stop.shape == (x.shape[0], x.shape[1], 1) and out.shape == x.shape


def test_library_path_takes_injected_masks(golden):
    """The masks a test injects replace the LockedDropout draws: zero masks make every step's input zero, so teacher
    forcing and free running give the same outputs."""
    z = golden("lstm_step_tf")
    model, _ = _model("lstm_step_tf", z)
    s2s = model.seq2seq.train()
    x = torch.from_numpy(z["tap.in"].copy())
    masks = torch.zeros_like(x)
    np.random.seed(3)
    a, _ = s2s(x, x, teacher_forcing_ratio=1.0, masks=masks)
    np.random.seed(3)
    b, _ = s2s(x, x, teacher_forcing_ratio=0.0, masks=masks)
    assert torch.equal(a, b)
    np.random.seed(3)
    c, _ = s2s(x, x, teacher_forcing_ratio=1.0, masks=torch.ones_like(x))
    assert not torch.equal(a, c)


def test_graph_mode_warns_and_runs_eager():
    from multi_part_assembly_amd.trainer import Trainer

    cfg = config.lstm_everyday()
    model = build_model(cfg)
    with pytest.warns(UserWarning, match="use_graph=True is not available for LSTMModel"):
        trainer = Trainer(model, cfg, use_graph=True)
    assert trainer.use_graph is False
