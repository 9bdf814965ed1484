"""The host layer's shared helpers on the GPU: the refinement model's loss summed over its rounds on whole [K, B] tensors
against the term-by-term sum, the batch's k-d order built once per `loss_function` call for semantic models too, and the
status word behind every cooperative launch (`gru.launch_watched`)."""
import warnings

import pytest
import torch

from multi_part_assembly_amd import _lib, config, gru, synthetic
from multi_part_assembly_amd.lstm import Seq2Seq
from multi_part_assembly_amd.pn_transformer import build_model

pytestmark = pytest.mark.gpu

B, P, N = 2, 3, 64


def _spy(monkeypatch):
    """Every `_lib.launch` of the test from here on: [(name, args)]."""
    calls, real = [], _lib.launch

    def launch(name, dev, *args, timer=None):
        calls.append((name, args))
        return real(name, dev, *args, timer=timer)

    monkeypatch.setattr(_lib, "launch", launch)
    return calls


def test_refine_rounds_on_whole_tensors_equal_the_term_by_term_sum(cuda_device, monkeypatch):
    """PNTransformerRefine, one training step: loss, every term and every parameter gradient with the rounds' [K, B]
    tensors kept whole are the bits of the same step with `.stacked` stripped from every round's terms."""
    cfg = config.pn_transformer_refine_everyday()
    cfg.model.refine_steps = 2
    cfg.data.max_num_part = P
    batch = synthetic.make_batch(B, P, N, seed=21, device=cuda_device, num_parts=[3, 2])
    batch.pop("num_parts")

    def step(strip):
        torch.manual_seed(3)
        model = build_model(cfg).to(cuda_device).train()
        real, seen = model._calc_loss, []

        def calc(out_dict, data_dict):
            loss_dict, out = real(out_dict, data_dict)
            seen.append(loss_dict.stacked is not None)
            if strip:
                loss_dict.stacked = None
            return loss_dict, out

        monkeypatch.setattr(model, "_calc_loss", calc)
        whole = []
        inner = model._loss_function
        monkeypatch.setattr(model, "_loss_function", lambda *a, **k: whole.append(inner(*a, **k)) or whole[-1])
        res = model.forward_pass(batch, mode="train")
        res["loss"].backward()
        assert seen == [True, True]  # both rounds came from the fused loss with every row in use
        assert (getattr(whole[0][0], "stacked", None) is None) == strip
        return res, {k: p.grad for k, p in model.named_parameters()}

    res_w, grad_w = step(False)
    res_s, grad_s = step(True)
    names = ["trans_loss", "rot_pt_cd_loss", "transform_pt_cd_loss", "rot_loss", "rot_pt_l2_loss"]
    assert list(res_w) == list(res_s) == names + [f"{k}_{i}" for i in range(2) for k in names] + ["loss"]
    for k in res_w:
        assert torch.equal(res_w[k], res_s[k]), k
    assert list(grad_w) == list(grad_s)
    for k in grad_w:
        assert grad_w[k] is not None and torch.equal(grad_w[k], grad_s[k]), k


def test_semantic_model_builds_the_part_order_once_per_loss_function_call(cuda_device, monkeypatch):
    """B-Global on semantic data with the leaf search and two min-of-N samples: `mpa_assembly_order` runs once per
    `loss_function` call and both samples' loss launches read that order; with nothing handing the loss an order every
    launch builds its own inside the library (what a semantic model did before) — the result is the same to the bit."""
    cfg = config.global_partnet_chair()
    cfg.data.max_num_part = P
    cfg.loss.shape_search = "leaf"
    cfg.loss.sample_iter = 2
    batch = synthetic.make_partnet_like_batch(B, P, N, seed=33, device=cuda_device)
    batch.pop("num_parts")
    torch.manual_seed(3)
    model = build_model(cfg).to(cuda_device).train()
    calls = _spy(monkeypatch)

    def run():
        del calls[:]
        torch.manual_seed(5)  # the pose head's noise and the matching's sub-samples: host draws
        res = model.forward_pass(batch, mode="train")
        built = [args[5] for name, args in calls if name == "mpa_assembly_order"]            # (its output)
        read = [args[11] for name, args in calls if name == "mpa_assembly_loss_forward_ordered"]
        return res, built, read

    res, built, read = run()
    assert len(built) == 1 and len(read) == 2 and all(r is built[0] for r in read)
    monkeypatch.setattr(model, "_start_part_order", lambda data_dict: data_dict)
    res_each, built, read = run()
    assert built == [] and read == [None, None]  # (every launch ordered the parts itself)
    assert list(res) == list(res_each) == ["trans_loss", "rot_pt_cd_loss", "transform_pt_cd_loss", "loss"]
    for k in res:
        assert torch.equal(res[k], res_each[k]), k


def _watched(calls):
    return [(name, args) for name, args in calls if name.startswith(("mpa_gru_", "mpa_seq2seq_decoder_"))]


def test_every_cooperative_launch_carries_the_status_word(cuda_device, monkeypatch):
    """`gru_recurrent` and the HIP seq2seq decoder, forward and backward: each launch got the device's status word as the
    argument in front of the stream, and the word is clean afterwards."""
    H, T = 128, 3
    if not gru.supported(H, B):
        pytest.skip("gru.hip not resident on this device")
    word = gru.prepare(cuda_device)[0]
    calls = _spy(monkeypatch)
    torch.manual_seed(2)
    gi = torch.randn(2, B, T, 3 * H, device=cuda_device, requires_grad=True)
    whh = (0.1 * torch.randn(2, 3 * H, H, device=cuda_device)).requires_grad_()
    bhh = torch.zeros(2, 3 * H, device=cuda_device, requires_grad=True)
    gru.gru_recurrent(gi, torch.zeros(2, B, H, device=cuda_device), whh, bhh).sum().backward()
    assert [name for name, _ in _watched(calls)] == ["mpa_gru_forward", "mpa_gru_backward"]

    s2s = Seq2Seq(128, 128, 256).to(cuda_device).train()
    x = torch.randn(T, B, 128, device=cuda_device, requires_grad=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y, _ = s2s(x, x.detach(), valids=torch.ones(B, T, device=cuda_device), teacher_forcing_ratio=0.0, hip=True)
    y.sum().backward()
    assert [name for name, _ in _watched(calls)][2:] == ["mpa_gru_forward", "mpa_seq2seq_decoder_forward",
                                                         "mpa_seq2seq_decoder_backward", "mpa_gru_backward"]
    # (the argument positions tests/test_workspace_guard_gpu.py's ROLES names: 10 and 12, 17 and 11)
    assert [len(args) - 1 for _, args in _watched(calls)] == [10, 12, 10, 17, 11, 12]
    for name, args in _watched(calls):
        assert args[-1] is word and word is gru._status(cuda_device)[0], name
    gru.raise_if_failed(cuda_device, synchronize=True)
