#!/usr/bin/env python3
"""Generate the B-LSTM fixtures under tests/golden/ by RUNNING THE REFERENCE's LSTMModel (models/b_lstm/), in this
container, with the helpers of make_golden.py:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lstm.py [--only lstm_step_tf,...]

  lstm_step_tf.npz        everyday flags, the teacher-forcing coin forced
  lstm_step_free.npz      everyday flags, the free-running coin forced
  lstm_semantic_step.npz  PartNet-chair flags (matching, min-of-5, 32 noise channels); coins from the seeded `random`

Shipped widths (pc_feat_dim 128, lstm_hidden_size 256), B = 3, P = 5, parts [2, 4, 5], N = 64 (128 for the semantic
step: the reference's matcher subsamples 100 points per part).  Each file holds the
batch, every loss term, the float32 and float64 gradients (param_fill.compact), the names whose gradient is None and
the names whose gradient is exactly zero, and a tap of the seq2seq module: its input, and per call its output, the
gradient arriving at that output and the coin — so the library path can be checked on the CPU without the HIP encoder
and loss.  Inside this generator only:
  * `Tensor.cuda` is a no-op (seq2seq.py:157,173 move the initial states to the GPU);
  * `DecoderRNN.dropout_i = 0` and the GRUs' inter-layer dropout = 0 (the latter only acts on the dead layer 1, but
    it draws from the CPU generator that the pose head's noise and the matcher also use);
  * `init_hidden` / `init_input` are cast for the float64 pass;
  * torch, numpy and `random` are seeded before both passes;
  * the coin is forced through Seq2Seq.forward's `teacher_forcing_ratio` (1.0: teacher, 0.0: free running).
"""
from __future__ import annotations

import argparse
import os
import random
import sys
from pathlib import Path

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden as mg  # noqa: E402
import param_fill  # noqa: E402


def _seed(seed):
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)


def _prepare(model, dtype):
    mg.zero_dropout(model)
    s2s = model.seq2seq
    s2s.decoder.dropout_i = 0
    s2s.encoder.rnn.gru.dropout = 0.0
    s2s.decoder.gru.dropout = 0.0
    s2s.encoder.rnn.init_hidden = s2s.encoder.rnn.init_hidden.to(dtype)
    s2s.decoder.init_input = s2s.decoder.init_input.to(dtype)


def _run(cfg, data, seed, ratio, dtype):
    """One training-mode forward_pass + backward; returns (model, loss dict, tap)."""
    from multi_part_assembly.models import build_model

    _seed(seed)
    model = build_model(cfg)
    param_fill.fill_parameters(model, seed)
    if dtype == torch.float64:
        model.double()
    _prepare(model, dtype)
    model.train()
    s2s = model.seq2seq
    if ratio is not None:
        type(s2s).forward.__defaults__ = (None, ratio)
    tap = {"in": None, "gin": None, "calls": []}
    coins = []
    real_random = random.random

    def coin():
        v = real_random()
        coins.append(v)
        return v

    def pre_hook(_m, args, kwargs):
        x = args[0]  # a new tensor per call (the same values): the gradient into it is summed over the calls
        if tap["in"] is None:
            tap["in"] = x.detach().clone()

        def acc(g):
            tap["gin"] = g.detach().clone() if tap["gin"] is None else tap["gin"] + g.detach()
        x.register_hook(acc)

    def post_hook(_m, _args, _kwargs, out):
        call = {"out": out[0].detach().clone(), "coin": coins[-1]}
        out[0].register_hook(lambda g: call.__setitem__("gout", g.detach().clone()))
        tap["calls"].append(call)

    h1 = s2s.register_forward_pre_hook(pre_hook, with_kwargs=True)
    h2 = s2s.register_forward_hook(post_hook, with_kwargs=True)
    random.random = coin
    try:
        _seed(seed + 1)
        cast = (lambda v: v.double()) if dtype == torch.float64 else (lambda v: v.clone())
        loss = model.forward_pass({k: (cast(v) if v.is_floating_point() else v.clone()) for k, v in data.items()},
                                  mode="val", optimizer_idx=-1)
        loss["loss"].backward()
    finally:
        random.random = real_random
        h1.remove()
        h2.remove()
        if ratio is not None:
            type(s2s).forward.__defaults__ = (None, 0.5)
    return model, loss, tap


def _lstm_step(name, cfg, data, seed, ratio):
    out = {f"data.{k}": mg.npy(v) for k, v in data.items()}
    out["seed"] = np.array([seed])
    out["cfg"] = np.array([cfg.model.pc_feat_dim, cfg.model.lstm_hidden_size])
    model, loss, tap = _run(cfg, data, seed, ratio, torch.float32)
    out["names"] = np.array(sorted(model.state_dict().keys()))
    for k, v in loss.items():
        if torch.is_tensor(v):
            out[f"loss.{k}"] = mg.npy(v)
    none, zero = [], []
    for k, p in model.named_parameters():
        if p.grad is None:
            none.append(k)
            continue
        if not bool(p.grad.any()):
            zero.append(k)
        out.update(param_fill.compact("grad.", k, mg.npy(p.grad)))
    out["grad_none"] = np.array(sorted(none))
    out["grad_zero"] = np.array(sorted(zero))
    out["tap.in"] = mg.npy(tap["in"])
    out["tap.gin"] = mg.npy(tap["gin"])
    out["tap.coin"] = np.array([c["coin"] for c in tap["calls"]])
    for i, c in enumerate(tap["calls"]):
        out[f"tap.out.{i}"] = mg.npy(c["out"])
        out[f"tap.gout.{i}"] = mg.npy(c["gout"])
    model64, loss64, tap64 = _run(cfg, data, seed, ratio, torch.float64)
    for k, v in loss64.items():
        if torch.is_tensor(v):
            out[f"loss64.{k}"] = mg.npy(v).astype(np.float64)
    for k, p in model64.named_parameters():
        if p.grad is not None:
            out.update(param_fill.compact("grad64.", k, mg.npy(p.grad)))
    assert [c["coin"] for c in tap64["calls"]] == [c["coin"] for c in tap["calls"]]
    mg.save(name, **out)


def _geometric(ratio, name):
    cfg = mg._load_cfg("configs/lstm", "lstm-32x1-cosine_200e-everyday")
    cfg.data.max_num_part = 5
    g = torch.Generator().manual_seed(1020)
    data = mg.synthetic_batch(g, 3, 5, 64, [2, 4, 5])
    _lstm_step(name, cfg, data, 1020, ratio)


def gen_lstm_semantic_step():
    cfg = mg._load_cfg("configs/lstm", "lstm-32x1-cosine_200e-partnet_chair")
    cfg.data.max_num_part = 5
    g = torch.Generator().manual_seed(1022)
    B, P, N = 3, 5, 128  # the reference's matcher subsamples 100 points per part
    data = mg.synthetic_batch(g, B, P, N, [2, 4, 5])
    match_ids = torch.tensor([[0, 0, 0, 0, 0], [1, 1, 0, 0, 0], [1, 1, 2, 2, 0]])
    for b in range(B):
        for gid in range(1, int(match_ids[b].max()) + 1):
            members = torch.nonzero(match_ids[b] == gid).flatten().tolist()
            for m in members[1:]:
                data["part_pcs"][b, m] = data["part_pcs"][b, members[0]]
    data["match_ids"] = match_ids
    data["instance_label"] = torch.eye(P)[None].repeat(B, 1, 1) * data["part_valids"][..., None]
    _lstm_step("lstm_semantic_step", cfg, data, 1022, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    mg.shim.import_reference()
    torch.Tensor.cuda = lambda self, *a, **k: self
    todo = {
        "lstm_step_tf": lambda: _geometric(1.0, "lstm_step_tf"),
        "lstm_step_free": lambda: _geometric(0.0, "lstm_step_free"),
        "lstm_semantic_step": gen_lstm_semantic_step,
    }
    for name, fn in todo.items():
        if not only or name in only:
            fn()


if __name__ == "__main__":
    main()
