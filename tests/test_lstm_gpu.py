"""B-LSTM on the GPU: the HIP path (csrc/gru.hip for the encoder, csrc/seq2seq.hip for the decoder) against the
reference's steps recorded in the fixtures (tests/golden/make_golden_lstm.py) and against a float64 library evaluation
of the same equations at full size and at the edges of the envelope; determinism, the dead half under the Trainer,
launch-count independence of P and the status word."""
import copy
import os
import random
import sys
import warnings

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import param_fill  # noqa: E402

from multi_part_assembly_amd import config, gru  # noqa: E402
from multi_part_assembly_amd.lstm import Seq2Seq  # noqa: E402
from multi_part_assembly_amd.pn_transformer import build_model  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {
    "lstm_step_tf": (config.lstm_everyday, 1.0),
    "lstm_step_free": (config.lstm_everyday, 0.0),
    "lstm_semantic_step": (config.lstm_partnet_chair, None),
}
DEAD = ("seq2seq.encoder.rnn.gru.", "_l1"), ("seq2seq.decoder.gru.", "_l1"), ("seq2seq.decoder.linear3.", "")


def _dead(name):
    return any(name.startswith(p) and (s == "" or name.endswith(s) or (s + "_") in name) for p, s in DEAD)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hip_step_matches_reference(golden, cuda_device, capsys, name):
    z = golden(name)
    preset, ratio = CASES[name]
    cfg = preset()
    cfg.data.max_num_part = 5
    seed = int(z["seed"][0])
    torch.manual_seed(seed)
    model = build_model(cfg)
    param_fill.fill_parameters(model, seed)
    model.seq2seq.decoder.dropout_i = 0
    if ratio is not None:
        model.seq2seq.teacher_forcing_ratio = ratio
    model.to(cuda_device).train()
    assert model.seq2seq._hip_ok(torch.zeros(5, 3, 128, device=cuda_device))
    data = {k[5:]: torch.from_numpy(z[k].copy()).to(cuda_device) for k in z if k.startswith("data.")}
    torch.manual_seed(seed + 1)
    np.random.seed(seed + 1)
    random.seed(seed + 1)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = model.forward_pass(data, mode="train")
        res["loss"].backward()
    assert not [w for w in caught if "library operators" in str(w.message)]  # the whole step ran on the HIP path
    for k in z:
        if k.startswith("loss."):
            np.testing.assert_allclose(float(res[k[5:]]), float(z[k]), rtol=1e-4, atol=1e-6, err_msg=k)
    record = dict(z)
    rows = []
    for k, p in model.named_parameters():
        if _dead(k):
            assert p.grad is None or not bool(p.grad.any()), k
            continue
        assert p.grad is not None, k
        mine, ref32, _ = param_fill.anchored_errors(record, k, p.grad.cpu().numpy(), floor=1e-4)
        rows.append((mine, ref32, k))
        # anchored at float64 as tests/test_callers_gpu.py clause (a): within twice the float32 reference's own distance
        # from float64, plus 1e-4 of the tensor's largest float64 entry
        assert mine <= 2.0 * ref32 + 1e-4, (k, mine, ref32)
    with capsys.disabled():
        worst = max(rows)
        print(f"\n  {name}: {len(rows)} gradient tensors vs float64: worst {worst[0]:.2e} ({worst[2]}; float32 reference "
              f"there {worst[1]:.2e})", end="")


def _pair(dev, B, P, lengths, ratio, dropout, seed=0):
    """One Seq2Seq forward + backward on the HIP path (float32) and on the library path in float64 with the same
    weights, inputs, masks, noise and coin -> (hip outputs, hip grads, library outputs, library grads)."""
    torch.manual_seed(seed)
    s2s = Seq2Seq(128, 128, 256)
    param_fill.fill_parameters(s2s, seed + 11)
    s2s = s2s.to(dev).train()
    ref = copy.deepcopy(s2s).double()
    g = torch.Generator(device="cpu").manual_seed(seed + 5)
    x = torch.randn(P, B, 128, generator=g).to(dev)
    valids = (torch.arange(P)[None] < torch.tensor(lengths)[:, None]).float().to(dev)
    x = x * valids.t()[..., None]
    gout = torch.randn(P, B, 128, generator=g).to(dev)
    masks = ((torch.rand(P, B, 128, generator=g) > dropout).float() / (1 - dropout)).to(dev) if dropout else None
    out = []
    for mod, dt, hip in ((s2s, torch.float32, True), (ref, torch.float64, False)):
        xi = x.detach().to(dt).clone().requires_grad_(True)
        np.random.seed(seed + 3)
        random.seed(seed + 3)
        y, _ = mod(xi, xi.detach(), valids=valids, teacher_forcing_ratio=ratio,
                   masks=None if masks is None else masks.to(dt), hip=hip)
        (y * gout.to(dt)).sum().backward()
        grads = {k: p.grad.double() for k, p in mod.named_parameters() if p.grad is not None}
        grads["input"] = xi.grad.double()
        out += [y.detach().double(), grads]
    return out


def _close(a, b, bar, what):
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))
    assert err < bar, (what, err)
    return err


@pytest.mark.parametrize("ratio", [1.0, 0.0], ids=["teacher", "free"])
def test_decoder_full_size_against_float64(cuda_device, capsys, ratio):
    """B = 32, P = 20 with the same injected dropout masks: forward and backward (dh0 reaches the input through the
    encoder) against the float64 library evaluation."""
    B, P = 32, 20
    lengths = [P - (b % 18) for b in range(B)]
    y, gh, y64, g64 = _pair(cuda_device, B, P, lengths, ratio, 0.2)
    errs = {"y": _close(y, y64, 1e-4, "y")}
    assert sorted(gh) == sorted(g64)
    for k in g64:
        errs[k] = _close(gh[k], g64[k], 1e-4, k)
    with capsys.disabled():
        w = max(errs, key=errs.get)
        print(f"\n  decoder B={B} P={P} {'teacher' if ratio else 'free'}: worst {errs[w]:.2e} ({w})", end="")


@pytest.mark.parametrize("B,P,lengths", [
    (1, 20, [20]), (64, 20, None), (4, 1, [1, 1, 1, 1]), (8, 12, [12] * 8), (8, 12, [1, 2, 1, 12, 1, 5, 1, 1])],
    ids=["B1", "B64", "P1", "all_full", "lengths_1"])
@pytest.mark.parametrize("ratio", [1.0, 0.0], ids=["teacher", "free"])
def test_decoder_edges_against_float64(cuda_device, B, P, lengths, ratio):
    if lengths is None:
        lengths = [1 + (b * 7) % P for b in range(B)]
    y, gh, y64, g64 = _pair(cuda_device, B, P, lengths, ratio, 0.2, seed=B + P)
    _close(y, y64, 1e-4, "y")
    for k in g64:
        _close(gh[k], g64[k], 1e-4, k)


@pytest.mark.parametrize("ratio", [1.0, 0.0], ids=["teacher", "free"])
def test_two_runs_are_bit_identical(cuda_device, ratio):
    a = _pair(cuda_device, 32, 20, [20 - b % 7 for b in range(32)], ratio, 0.2)
    b = _pair(cuda_device, 32, 20, [20 - b % 7 for b in range(32)], ratio, 0.2)
    assert torch.equal(a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


def test_dead_parameters_unchanged_after_trainer_steps(cuda_device):
    from multi_part_assembly_amd.trainer import Trainer

    from multi_part_assembly_amd import synthetic

    cfg = config.lstm_everyday()
    cfg.data.max_num_part = 6
    torch.manual_seed(0)
    model = build_model(cfg).to(cuda_device)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    trainer = Trainer(model, cfg)
    batch = synthetic.make_batch(8, max_parts=6, num_points=256, seed=3, device=cuda_device)
    for _ in range(3):
        trainer.train_step(batch)
    trainer.check_health(synchronize=True)
    gru.raise_if_failed(synchronize=True)
    moved = 0
    for k, p in model.named_parameters():
        if _dead(k):
            assert torch.equal(p.detach(), before[k]), k
        else:
            moved += int(not torch.equal(p.detach(), before[k]))
    assert moved > 0


class _OpCount(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def _ops_per_step(dev, P, hip):
    s2s = Seq2Seq(128, 128, 256).to(dev).train()
    x = torch.randn(P, 16, 128, device=dev, requires_grad=True)
    valids = torch.ones(16, P, device=dev)
    for _ in range(2):
        with _OpCount() as c, warnings.catch_warnings():
            warnings.simplefilter("ignore")
            y, _ = s2s(x, x.detach(), valids=valids, teacher_forcing_ratio=0.0, hip=hip)
            y.sum().backward()
    return c.n


def test_aten_op_count_does_not_grow_with_parts(cuda_device, capsys):
    hip = (_ops_per_step(cuda_device, 8, True), _ops_per_step(cuda_device, 20, True))
    lib = (_ops_per_step(cuda_device, 8, False), _ops_per_step(cuda_device, 20, False))
    with capsys.disabled():
        print(f"\n  aten ops per seq2seq forward + backward, P = 8 / 20: HIP {hip}, library {lib}", end="")
    assert hip[0] == hip[1]
    assert lib[1] > lib[0]


def test_status_word_is_clean_after_a_step(cuda_device):
    _pair(cuda_device, 16, 10, [10] * 16, 0.0, 0.2)
    gru.raise_if_failed(synchronize=True)
