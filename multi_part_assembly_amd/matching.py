"""Device-side GT <-> prediction matching of equivalent parts (csrc/match.hip).

`linear_sum_assignment` mirrors scipy's (square problems, batched); `match_parts` does the work of
`BaseModel._match_parts` (multi_part_assembly/models/modules/base_model.py:181-238) for every group of every sample of
the batch in three launches, with no device-to-host copy; `sample_indices` draws the matching's point sub-samples on
the device (csrc/match_sample.hip), and `MatchSampler` keeps the seed and step counter of those draws for a model."""
from __future__ import annotations

import torch

from . import _lib

SUBSAMPLE = 100  # points per part in the cost matrix (base_model.py:163)
MAX_POINTS = 16384  # N of the device-side draw (include/mpa_hip.h: the permutation lives in LDS)
SALT_STEP = 0x632BE59BD9B4E019  # odd: the k-th draw of one step adds k * SALT_STEP to the step counter
_U64 = 0xFFFFFFFFFFFFFFFF


def static_groups(P: int) -> int:
    """Group slots of the device-side draw: groups have at least two members and the datasets number them consecutively
    from 1 (partnet_data.py:195-208, `datasets.match_ids`), so no id of a sample with P slots exceeds P // 2."""
    return max(1, P // 2)


def sample_indices(B, G, N, n, seed, counter=0, counter_dev=None, salt=0, device="cuda"):
    """sample_idx [B, G, n] int32 on the HIP device: per group slot the first n entries of a random permutation of
    0..N-1 (`torch.randperm(N)[:n]`), Philox4x32-10 keyed by `seed`, stream (slot, counter + salt); the layout is fixed in
    include/mpa_hip.h.  `counter_dev` (int64 [1] on the device) is read by the kernel instead of `counter`: a captured
    step passes it and rewrites the word between replays."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("sample_indices: HIP device only — no CPU fallback")
    if counter_dev is not None:
        assert counter_dev.dtype == torch.int64 and counter_dev.device == dev and counter_dev.numel() == 1
    out = torch.empty((B, G, n), dtype=torch.int32, device=dev)
    _lib.launch("mpa_match_sample_indices", dev, B, G, N, n, int(seed) & _U64, int(counter) & _U64, counter_dev,
                int(salt) & _U64, out)
    return out


class MatchSampler(torch.nn.Module):
    """Seed and step counter of a model's device-side matching draws (`cfg.loss.match_sample = "device"`): no parameters,
    no buffers, so the model's `state_dict` is unchanged.  `_calls` is the number of training steps drawn so far and
    `advance_seed()` moves it on for the next replay of a captured step — the names `Trainer` looks for, so its replay
    loop and the "dropout_calls" entry of its checkpoints cover this module as they cover the transformer's dropout seed.

    One step = one `begin_step()` followed by any number of `draw_args()`: the k-th draw of the step uses the stream
    (counter, k).  Eager launches carry the counter by value; while a step is being captured the kernels read it from a
    device word instead, so that every replay draws afresh — the same numbers an eager run draws at that step."""

    def __init__(self):
        super().__init__()
        self._calls = 0       # training steps begun (or replays announced by advance_seed)
        self._eval_calls = 0  # evaluation passes draw from a stream of their own: they never move the training stream
        self._current = 0
        self._salt = 0
        self._word = None

    def prepare_streams(self, dev):
        """Allocate the device word outside any capture (Trainer.__init__ calls this)."""
        dev = torch.device(dev)
        if dev.type == "cuda" and (self._word is None or self._word.device != dev):
            self._word = torch.zeros(1, dtype=torch.int64, device=dev)

    def begin_step(self, training=True):
        self._salt = 0
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            return  # the replay's counter is whatever advance_seed() wrote last
        if training:
            self._calls += 1
            self._current = self._calls
        else:
            self._eval_calls += 1
            self._current = (1 << 62) | self._eval_calls

    def advance_seed(self):
        self._calls += 1
        if self._word is not None:
            self._word.fill_(self._calls)

    def draw_args(self, dev):
        """Keyword arguments of `match_parts` / `sample_indices` for the next draw of the current step."""
        salt = (self._salt * SALT_STEP) & _U64
        self._salt += 1
        args = {"seed": torch.initial_seed() & _U64, "salt": salt}
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            if self._word is None or self._word.device != dev:
                raise RuntimeError("MatchSampler: the counter's device word must exist before a step is captured "
                                   "(Trainer.__init__ allocates it through prepare_streams)")
            args["counter_dev"] = self._word
        else:
            args["counter"] = self._current
        return args


def linear_sum_assignment(cost: torch.Tensor, sizes: torch.Tensor | None = None) -> torch.Tensor:
    """cost [problems, ld, ld] float32 on the HIP device (sizes[i] x sizes[i] used; default the full ld) ->
    col4row [problems, ld] int32, the column assigned to each row (scipy's `col_ind`; -1 past the size)."""
    _lib.require_hip("linear_sum_assignment", cost)
    cost = cost.detach().to(torch.float32).contiguous()
    problems, ld, ld2 = cost.shape
    assert ld == ld2, "square problems only"
    dev = cost.device
    if sizes is None:
        sizes = torch.full((problems,), ld, dtype=torch.int32, device=dev)
    sizes = sizes.to(device=dev, dtype=torch.int32).contiguous()
    out = torch.empty((problems, ld), dtype=torch.int32, device=dev)
    _lib.launch("mpa_linear_sum_assignment", dev, cost, sizes, problems, ld, out)
    return out


def match_parts(part_pcs, pred_trans, pred_quat, gt_trans, gt_quat, match_ids, sample_idx=None, ret_aux=False, seed=0,
                counter=0, counter_dev=None, salt=0):
    """GT poses rearranged inside every group of equivalent parts so that they line up with the predictions at
    minimum Chamfer cost.  match_ids [B,P] (0 = unique / padded, g >= 1 = group g), sample_idx [B,G,n] point
    indices per group slot; the rotations are quaternions [B,P,4] or rotation matrices [B,P,3,3].  Returns
    (new_trans [B,P,3], new_rot in the rotations' shape) and, with ret_aux, also
    (perm [B,P], cost [B,G,P,P], col4row [B,G,P]).

    sample_idx=None draws the indices on the device (`sample_indices` with seed / counter | counter_dev / salt) for the
    static number of group slots G = `static_groups(P)`: nothing is read back, so the call can be captured.  The
    contract on `match_ids` in that mode: no id above P // 2 — groups numbered consecutively from 1 with at least two
    members each, as `datasets.match_ids` builds them (it checks); a larger id would be left unmatched."""
    _lib.require_hip("match_parts", part_pcs)
    B, P, N, _ = part_pcs.shape
    dev = part_pcs.device
    f = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
    i32 = lambda t: t.detach().to(device=dev, dtype=torch.int32).contiguous()
    if sample_idx is None:
        sample_idx = sample_indices(B, static_groups(P), N, min(SUBSAMPLE, N), seed, counter, counter_dev, salt, dev)
    sample_idx = i32(sample_idx)
    _, G, n = sample_idx.shape
    cost = torch.empty((B, G, P, P), dtype=torch.float32, device=dev)
    col4row = torch.empty((B, G, P), dtype=torch.int32, device=dev)
    new_t = torch.empty((B, P, 3), dtype=torch.float32, device=dev)
    rmat = pred_quat.shape[-2:] == (3, 3)  # rotation matrices (rot_type='rmat') instead of quaternions
    new_q = torch.empty((B, P) + tuple(pred_quat.shape[2:]), dtype=torch.float32, device=dev)
    perm = torch.empty((B, P), dtype=torch.int32, device=dev)
    args = [f(part_pcs), f(pred_trans), f(pred_quat), f(gt_trans), f(gt_quat), i32(match_ids), sample_idx]
    _lib.launch("mpa_match_parts_rmat" if rmat else "mpa_match_parts", dev, *args, B, P, N, G, n, cost, col4row, new_t,
                new_q, perm)
    return (new_t, new_q, perm, cost, col4row) if ret_aux else (new_t, new_q)
