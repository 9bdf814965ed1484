"""B-LSTM baseline — mirror of the reference's LSTMModel and its seq2seq module (multi_part_assembly/models/b_lstm/
network.py:9-152, seq2seq.py:12-241), same sub-module names and state_dict keys (the dead layers and `linear3`
included).

What reaches the loss is one layer of each GRU:
  encoder  layer 0 of nn.GRU(128, 256, 2 layers, bidirectional) over the valid parts -> its final states;
  decoder  layer 0 of nn.GRU(128, 528, 2 layers), initial state cat(forward final, reverse final, noise), all P steps,
           then linear1 (Linear(528, 256), LeakyReLU(True) — slope 1.0, the identity — Linear(256, 128)).
Encoder layer 1 only feeds decoder layer 1's initial state, decoder layer 1 only feeds itself, and `linear3` (the stop
signs) is unused by LSTMModel: none of them is computed (their gradients stay None; the GRU inter-layer dropout only acts
on them).  Stop signs are computed, on library operators, only when `Seq2Seq.forward(..., return_stop_signs=True)`.

Hot path: the encoder's recurrence on csrc/gru.hip (both directions in one launch, the device-side length plan of
RGL-NET's GRU: no `lengths.cpu()`), the decoder's P steps + head in one launch of csrc/seq2seq.hip each way.  Outside
the kernels' envelope (CPU tensors, lstm_hidden_size != 256, pc_feat_dim != 128, B > 64, a device that cannot hold the
grid, MPA_GRU=library) the same equations run on library operators, step by step as the reference does, with one warning.

Host randomness is drawn like the reference, in its order and on its generators: the decoder noise with
`np.random.normal`, the teacher-forcing coin with `random.random()`, once per forward — in eval mode too.  The
LockedDropout masks (training mode) are one `bernoulli_` of [P, B, C] per forward on the input's device.

`cfg.model.lstm_draws = "device"` draws all three with one launch of csrc/seq2seq_draw.hip instead (`draw`; the numpy
restatement seq2seq_draw_ref.py is its definition) and lets the decoder launch read the coin from device memory
(`mpa_seq2seq_decoder_forward_sel`): no host generator, no host-to-device copy, nothing read back — the step can be
captured into a HIP graph, and `DrawCounter` keeps the position of the stream as `matching.MatchSampler` does for the
matching's draws.  That mode has no library path: outside the kernels' envelope it raises."""
from __future__ import annotations

import ctypes
import random

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from . import gru as _gru
from .base_model import BaseModel
from .encoder import build_encoder
from .matching import MatchSampler
from .regressor import StocasticPoseRegressor

_H, _C, _Z = 528, 128, 256  # the decoder shapes csrc/seq2seq.hip is built for
_DEC_RESIDENT: dict = {}
_U64 = 0xFFFFFFFFFFFFFFFF


def _decoder_resident(batch):
    key = (batch, torch.cuda.current_device())
    if key not in _DEC_RESIDENT:
        _DEC_RESIDENT[key] = bool(_lib.query("mpa_seq2seq_decoder_resident", batch, slot=ctypes.c_int))
    return _DEC_RESIDENT[key]


class _DecoderFn(torch.autograd.Function):
    """Layer 0 of the decoder GRU + linear1 over all P steps (csrc/seq2seq.hip).  `target` [P, B, C] (detached part
    features) selects teacher forcing — step t > 0 reads target[t - 1] — and None free running — step t > 0 reads the
    launch's own y[t - 1].  `mask` [P, B, C]: the scaled LockedDropout mask of every step (None: no dropout)."""

    @staticmethod
    def forward(ctx, h0, target, mask, P, w_ih, b_ih, w_hh, b_hh, w1, b1, w2, b2):
        B = h0.shape[0]
        dev = h0.device
        h0 = h0.detach().float().contiguous()
        gi = None
        if target is not None:  # teacher forcing: the step inputs are known, their projections are one GEMM
            x = torch.cat([torch.zeros_like(target[:1]), target[:-1]], dim=0)
            if mask is not None:
                x = x * mask
            gi = F.linear(x, w_ih, b_ih).contiguous()
        ws = torch.empty(_lib.query("mpa_seq2seq_decoder_workspace", B, P), dtype=torch.float32, device=dev)
        hs = torch.empty((P, B, _H), dtype=torch.float32, device=dev)
        z1 = torch.empty((P, B, _Z), dtype=torch.float32, device=dev)
        y = torch.empty((P, B, _C), dtype=torch.float32, device=dev)
        mask_c = mask.contiguous() if (mask is not None and target is None) else None
        _gru.launch_watched("mpa_seq2seq_decoder_forward", dev, gi, mask_c, h0, w_ih, b_ih, w_hh, b_hh, w1, b1, w2, b2,
                            B, P, ws, hs, z1, y, timer=f"seq2seq_decoder_forward[{B}x{P}]")
        if target is None:  # free running: the inputs were the launch's own outputs (the same values)
            x = torch.cat([torch.zeros_like(y[:1]), y[:-1]], dim=0)
            if mask is not None:
                x = x * mask
        ctx.save_for_backward(h0, x, w_hh, w1, w2, hs, z1, ws)
        return y

    @staticmethod
    def backward(ctx, dy):
        dh0, *rest = _decoder_backward(ctx, dy)
        return (dh0, None, None, None, *rest)


def _decoder_backward(ctx, dy):
    """(dh0, dwih, dbih, dwhh, dbhh, dw1, db1, dw2, db2) from what either decoder function saved."""
    h0, x, w_hh, w1, w2, hs, z1, ws = ctx.saved_tensors
    P, B, _ = hs.shape
    dev = hs.device
    dy2 = dy.reshape(P * B, _C).float()
    # the head over all P * B rows: batched GEMMs (its gradient w.r.t. h_t of every step is known up front)
    dw2 = dy2.t() @ z1.reshape(P * B, _Z)
    db2 = dy2.sum(0)
    dz1 = dy2 @ w2
    dw1 = dz1.t() @ hs.reshape(P * B, _H)
    db1 = dz1.sum(0)
    dh = (dz1 @ w1).reshape(P, B, _H).contiguous()
    dgi = torch.empty((P, B, 3 * _H), dtype=torch.float32, device=dev)
    dwhh = torch.empty_like(w_hh)
    dbhh = torch.empty((3 * _H,), dtype=torch.float32, device=dev)
    dh0 = torch.empty((B, _H), dtype=torch.float32, device=dev)
    _gru.launch_watched("mpa_seq2seq_decoder_backward", dev, dh, h0, w_hh, hs, B, P, ws, dgi, dwhh, dbhh, dh0,
                        timer=f"seq2seq_decoder_backward[{B}x{P}]")
    dgi2 = dgi.reshape(P * B, 3 * _H)
    dwih = dgi2.t() @ x.reshape(P * B, _C)
    dbih = dgi2.sum(0)
    return dh0, dwih, dbih, dwhh, dbhh, dw1, db1, dw2, db2


class _DecoderSelFn(torch.autograd.Function):
    """`_DecoderFn` with the mode read on the device: `teacher` (int32 [1] on the device, from `draw`) picks teacher forcing
    (nonzero) or free running (zero) inside the launch.  `target` is always given and its projections always computed (one
    GEMM: cheap beside a launch shape the host would have to choose); the flag is never read back."""

    @staticmethod
    def forward(ctx, h0, target, mask, teacher, P, w_ih, b_ih, w_hh, b_hh, w1, b1, w2, b2):
        B = h0.shape[0]
        dev = h0.device
        h0 = h0.detach().float().contiguous()
        xt = torch.cat([torch.zeros_like(target[:1]), target[:-1]], dim=0)
        if mask is not None:
            xt = xt * mask
        gi = F.linear(xt, w_ih, b_ih).contiguous()
        ws = torch.empty(_lib.query("mpa_seq2seq_decoder_workspace", B, P), dtype=torch.float32, device=dev)
        hs = torch.empty((P, B, _H), dtype=torch.float32, device=dev)
        z1 = torch.empty((P, B, _Z), dtype=torch.float32, device=dev)
        y = torch.empty((P, B, _C), dtype=torch.float32, device=dev)
        _gru.launch_watched("mpa_seq2seq_decoder_forward_sel", dev, gi, mask, teacher, h0, w_ih, b_ih, w_hh, b_hh, w1, b1,
                            w2, b2, B, P, ws, hs, z1, y, timer=f"seq2seq_decoder_forward[{B}x{P}]")
        # the step inputs behind dW_ih: the targets, or the launch's own outputs (the same values it fed back)
        xy = torch.cat([torch.zeros_like(y[:1]), y[:-1]], dim=0)
        if mask is not None:
            xy = xy * mask
        x = torch.where(teacher != 0, xt, xy)
        ctx.save_for_backward(h0, x, w_hh, w1, w2, hs, z1, ws)
        return y

    @staticmethod
    def backward(ctx, dy):
        dh0, *rest = _decoder_backward(ctx, dy)
        return (dh0, None, None, None, None, *rest)


def draw(B, T, p, ratio, training, seed=0, counter=0, counter_dev=None, salt=0, device="cuda"):
    """One launch of csrc/seq2seq_draw.hip: (noise float32 [B, 16], teacher int32 [1], mask float32 [T, B, 128] — the
    scaled LockedDropout mask, None unless `training`) on the HIP device, Philox4x32-10 keyed by `seed`, stream
    counter + salt (seq2seq_draw_ref.py restates the layout).  `counter_dev` (int64 [1] on the device) is read by the
    kernel instead of `counter`: a captured step passes it and rewrites the word between replays."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("lstm.draw: HIP device only — no CPU fallback")
    if counter_dev is not None:
        assert counter_dev.dtype == torch.int64 and counter_dev.device == dev and counter_dev.numel() == 1
    noise = torch.empty((B, 16), dtype=torch.float32, device=dev)
    teacher = torch.empty((1,), dtype=torch.int32, device=dev)
    mask = torch.empty((T, B, _C), dtype=torch.float32, device=dev) if training else None
    _lib.launch("mpa_seq2seq_draw", dev, B, T, float(p), float(ratio), int(seed) & _U64, int(counter) & _U64, counter_dev,
                int(salt) & _U64, noise, teacher, mask, timer=f"seq2seq_draw[{B}x{T}]")
    return noise, teacher, mask


class DrawCounter(MatchSampler):
    """Seed and step counter of a model's device-side seq2seq draws (`cfg.model.lstm_draws = "device"`): the protocol of
    `matching.MatchSampler` — `begin_step` once per `loss_function`, the k-th forward of the step draws from the stream
    (counter, k), by value in eager launches and through the device word while a step is captured, evaluation passes on
    the `1 << 62` stream — with `draw_args` feeding `draw`.  No parameters, no buffers."""


class LockedDropout(nn.Module):
    """seq2seq.py:226-241: one mask per sequence and channel, shared by the steps of a call."""

    def forward(self, x, dropout=0.5):
        if not self.training or not dropout:
            return x
        m = x.data.new(1, x.size(1), x.size(2)).bernoulli_(1 - dropout)
        mask = m.detach().clone().requires_grad_(False) / (1 - dropout)
        return mask.expand_as(x) * x


class EncoderRNN(nn.Module):
    """seq2seq.py:12-57 (parameters and `init_hidden` only: Seq2Seq runs the live layer itself)."""

    def __init__(self, input_size, hidden_size, n_layer=1, bidirectional=False):
        super().__init__()
        self.input_size, self.hidden_size, self.n_layer = input_size, hidden_size, n_layer
        self.bidirectional = bidirectional
        self.num_directions = 2 if bidirectional else 1
        self.gru = nn.GRU(input_size, hidden_size, n_layer, bidirectional=bidirectional,
                          dropout=0.2 if n_layer == 2 else 0)
        self.init_hidden = torch.zeros(n_layer * self.num_directions, 1, hidden_size)


class _RNNWrapper(nn.Module):
    """The reference's RNNWrapper (modules/rnn.py:6-46) as a container: keeps the `encoder.rnn.gru.*` keys."""

    def __init__(self, rnn, batch_first=False):
        super().__init__()
        self.rnn = rnn
        self.batch_first = batch_first


class DecoderRNN(nn.Module):
    """seq2seq.py:60-137: nn.GRU(input, hidden, 2 layers), linear1 (the output code), linear3 (the stop signs)."""

    def __init__(self, input_size, hidden_size, n_layer=1, bidirectional=False):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        self.bidirectional = bidirectional
        self.num_directions = 2 if bidirectional else 1
        self.n_units_hidden1, self.n_units_hidden2 = 256, 128
        self.gru = nn.GRU(input_size, hidden_size, n_layer, bidirectional=bidirectional,
                          dropout=0.2 if n_layer == 2 else 0)
        self.linear1 = nn.Sequential(nn.Linear(hidden_size, self.n_units_hidden1), nn.LeakyReLU(True),
                                     nn.Linear(self.n_units_hidden1, input_size))
        self.linear3 = nn.Sequential(nn.Linear(hidden_size, self.n_units_hidden2), nn.ReLU(True), nn.Dropout(0.2),
                                     nn.Linear(self.n_units_hidden2, 1))
        self.lockdrop = LockedDropout()
        self.dropout_i = 0.2
        self.dropout_o = 0.2
        self.init_input = torch.zeros((1, 1, input_size))


class Seq2Seq(nn.Module):
    """seq2seq.py:140-223."""

    def __init__(self, enc_input_size, dec_input_size, hidden_size, draws="host"):
        super().__init__()
        self.n_layer = 2
        self.draws = draws  # "host": the reference's generators; "device": csrc/seq2seq_draw.hip
        if draws == "device":
            self.draw_counter = DrawCounter()
        self.encoder = _RNNWrapper(EncoderRNN(enc_input_size, hidden_size, n_layer=self.n_layer, bidirectional=True))
        self.decoder = DecoderRNN(dec_input_size, hidden_size * 2 + 16, n_layer=self.n_layer, bidirectional=False)
        self.teacher_forcing_ratio = 0.5
        self.hip = None  # None: the HIP kernels inside their envelope; False: library operators (tools/lstm_step.py)

    # ---- envelope ---------------------------------------------------------------------------------------------------
    def _hip_ok(self, x):
        B = x.shape[1]
        enc = self.encoder.rnn
        if not (x.is_cuda and enc.hidden_size == 256 and enc.input_size == _C and self.decoder.input_size == _C
                and B <= 64 and x.dtype == torch.float32):
            return False
        return _gru.supported(enc.hidden_size, B, 2) and _decoder_resident(B)

    def _warn_library(self, x):
        if not getattr(self, "_warned_library", False):
            import warnings
            warnings.warn(f"Seq2Seq: {tuple(x.shape)} {x.device.type} input with lstm_hidden_size = "
                          f"{self.encoder.rnn.hidden_size} is outside the HIP kernels' envelope; running the seq2seq "
                          "module on library operators (slow path)")
            self._warned_library = True

    # ---- encoder: layer 0, both directions, final states ------------------------------------------------------------
    def infer_encoder(self, input_seq, valids, hip):
        """input_seq [P, B, C] -> (forward final state [B, H], reverse final state [B, H]) of encoder layer 0 over the
        valid prefix of every sample (valid parts come first)."""
        from .gnn import _MaskedBiGRU
        P, B, _ = input_seq.shape
        g = self.encoder.rnn.gru
        H = g.hidden_size
        if valids is None:
            valids = torch.ones(B, P, device=input_seq.device, dtype=input_seq.dtype)
        rev_idx, _ = _MaskedBiGRU.plan(valids, P)
        last = (valids.sum(dim=1).long() - 1).clamp(min=0)                              # [B], on the device
        x = input_seq.transpose(0, 1)                                                    # [B, P, C]
        x_rev = torch.gather(x, 1, rev_idx[..., None].expand_as(x))
        h0 = input_seq.new_zeros(2, B, H)
        if hip:
            gi = torch.stack([F.linear(x, g.weight_ih_l0, g.bias_ih_l0),
                              F.linear(x_rev, g.weight_ih_l0_reverse, g.bias_ih_l0_reverse)])
            hs = _gru.gru_recurrent(gi, h0, torch.stack([g.weight_hh_l0, g.weight_hh_l0_reverse]),
                                    torch.stack([g.bias_hh_l0, g.bias_hh_l0_reverse]))
            fwd, bwd = hs[0], hs[1]
        else:
            fwd = torch._VF.gru(x, h0[0:1], [g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0],
                                True, 1, 0.0, self.training, False, True)[0]
            bwd = torch._VF.gru(x_rev, h0[1:2], [g.weight_ih_l0_reverse, g.weight_hh_l0_reverse, g.bias_ih_l0_reverse,
                                                 g.bias_hh_l0_reverse], True, 1, 0.0, self.training, False, True)[0]
        rows = torch.arange(B, device=input_seq.device)
        return fwd[rows, last], bwd[rows, last]

    # ---- decoder: layer 0 + linear1 over all P steps ----------------------------------------------------------------
    def _decode_library(self, h0, target_seq, teacher, masks, stop):
        d = self.decoder
        g = d.gru
        h = h0
        inp = h0.new_zeros(h0.shape[0], target_seq.shape[2])
        outs, stops = [], []
        for t in range(target_seq.shape[0]):
            x = inp * masks[t] if masks is not None else inp
            h = torch._VF.gru_cell(x, h, g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0)
            y = d.linear1(h)
            outs.append(y)
            if stop:
                stops.append(d.linear3(h))
            inp = target_seq[t] if teacher else y.detach()
        return torch.stack(outs, 0), (torch.stack(stops, 0) if stop else None)

    def _decode_hip(self, h0, target_seq, teacher, masks):
        d = self.decoder
        g = d.gru
        l1, l2 = d.linear1[0], d.linear1[2]
        return _DecoderFn.apply(h0, target_seq.detach().float().contiguous() if teacher else None,
                                None if masks is None else masks.float().contiguous(), target_seq.shape[0],
                                g.weight_ih_l0, g.bias_ih_l0, g.weight_hh_l0, g.bias_hh_l0, l1.weight, l1.bias,
                                l2.weight, l2.bias)

    def _forward_device(self, input_seq, target_seq, valids, ratio, return_stop_signs, masks, hip):
        """The forward with coin, noise and masks drawn by one launch and the coin read by the decoder launch."""
        if hip is False or self.hip is False or return_stop_signs or not self._hip_ok(input_seq):
            raise RuntimeError(f"Seq2Seq: lstm_draws = 'device' needs the HIP kernels, and {tuple(input_seq.shape)} "
                               f"{input_seq.device.type} input with lstm_hidden_size = {self.encoder.rnn.hidden_size} "
                               "(or a forced library path / stop signs) is outside their envelope; use lstm_draws = 'host'")
        P, B, _ = target_seq.shape
        dev = input_seq.device
        noise, teacher, drawn = draw(B, P, self.decoder.dropout_i, ratio, self.training,
                                     **self.draw_counter.draw_args(dev), device=dev)
        if masks is None:
            masks = drawn
        h_f, h_b = self.infer_encoder(input_seq, valids, True)
        h0 = torch.cat([h_f, h_b, noise], dim=1)                                        # decoder layer 0's state
        d = self.decoder
        g = d.gru
        l1, l2 = d.linear1[0], d.linear1[2]
        return _DecoderSelFn.apply(h0, target_seq.detach().float().contiguous(),
                                   None if masks is None else masks.float().contiguous(), teacher, P, g.weight_ih_l0,
                                   g.bias_ih_l0, g.weight_hh_l0, g.bias_hh_l0, l1.weight, l1.bias, l2.weight, l2.bias)

    def draw_masks(self, target_seq):
        """The LockedDropout masks of one forward, scaled: [P, B, C] (None outside training mode or at p = 0)."""
        p = self.decoder.dropout_i
        if not self.training or not p:
            return None
        m = target_seq.new_empty(target_seq.shape).bernoulli_(1 - p)
        return m / (1 - p)

    def forward(self, input_seq, target_seq, valids=None, teacher_forcing_ratio=None, return_stop_signs=False,
                masks=None, hip=None):
        """input_seq / target_seq [P, B, C], valids [B, P] -> (decoder outputs [P, B, C], stop signs [P, B, 1] or None).
        `masks` [P, B, C]: the scaled dropout masks to use instead of drawing them (tests compare the two paths with
        them); `hip` forces a path (None: the HIP kernels inside their envelope)."""
        ratio = self.teacher_forcing_ratio if teacher_forcing_ratio is None else teacher_forcing_ratio
        if self.draws == "device":
            return self._forward_device(input_seq, target_seq, valids, ratio, return_stop_signs, masks, hip), None
        B = target_seq.size(1)
        noise = np.random.normal(loc=0.0, scale=1.0, size=[self.n_layer * 1, B, 16]).astype(np.float32)
        noise = torch.tensor(noise).to(input_seq.device, non_blocking=True).type_as(input_seq)
        if hip is None and self.hip is False:
            hip = False
        if hip is None:
            hip = self._hip_ok(input_seq) and not return_stop_signs
            if not hip and not return_stop_signs:
                self._warn_library(input_seq)
        h_f, h_b = self.infer_encoder(input_seq, valids, hip)
        h0 = torch.cat([h_f, h_b, noise[0]], dim=1)                                     # decoder layer 0's state
        teacher = random.random() < ratio
        if masks is None:
            masks = self.draw_masks(target_seq)
        if hip:
            return self._decode_hip(h0, target_seq, teacher, masks), None
        return self._decode_library(h0, target_seq.detach(), teacher, masks, return_stop_signs)


class LSTMModel(BaseModel):
    """network.py:9-152."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.encoder = build_encoder(cfg.model.encoder, feat_dim=self.pc_feat_dim, global_feat=True,
                                     pointnet2_eval=self.pointnet2_eval)
        self.seq2seq = Seq2Seq(self.pc_feat_dim, self.pc_feat_dim, cfg.model.lstm_hidden_size, draws=self.lstm_draws)
        if self.lstm_draws == "device":  # nothing is drawn on the host: Trainer may capture the step
            self.host_draws_per_forward = False
        dim = self.pc_feat_dim
        if self.semantic:
            dim += self.max_num_part
        if self.use_part_label:
            dim += cfg.data.num_part_category
        self.pose_predictor = StocasticPoseRegressor(feat_dim=dim, noise_dim=cfg.loss.noise_dim, rot_type=self.rot_type)

    # the coin and the noise are host draws of every forward: a captured step would replay one draw for ever
    host_draws_per_forward = True

    @property
    def draw_counter(self):
        """The counter of the device-side draws (None on host draws): `BaseModel.loss_function` begins its steps."""
        return getattr(self.seq2seq, "draw_counter", None)

    def forward(self, data_dict):
        part_feats = data_dict.get("part_feats", None)
        if part_feats is None:
            part_feats = self._extract_part_feats(data_dict["part_pcs"], data_dict["part_valids"])
        seq = part_feats.transpose(0, 1).contiguous()                                    # [P, B, C]
        out, _ = self.seq2seq(seq, seq.detach(), valids=data_dict["part_valids"])
        out = out.transpose(0, 1)                                                         # [B, P, C]
        feats = torch.cat([out, data_dict["part_label"].type_as(part_feats),
                           data_dict["instance_label"].type_as(part_feats)], dim=-1)
        rot, trans = self.pose_predictor(feats)
        return {"rot": self._wrap_rotation(rot), "trans": trans, "part_feats": part_feats}

    def _loss_function(self, data_dict, out_dict={}, optimizer_idx=-1):
        """One MoN sample: the part features are reused, the seq2seq (new coin, noise and masks) re-runs."""
        return self._sample_loss(data_dict, out_dict, ("part_pcs", "part_valids", "part_label", "instance_label"),
                                 ("part_feats",))
