"""The shared tail of the training step without a device: `FlatBuffers.owner` (one lookup for `guard_report` and the
checkpoint refusal), `trainer.graph_refusal` (one function for the three `use_graph` refusals) and the order of mark and
collectives in `Trainer._reduce_grad`, recorded on stubs and compared with literals taken from the code this replaced."""
import types
import warnings

import pytest
import torch
import torch.distributed as dist
import torch.nn as nn

from multi_part_assembly_amd import _lib, config
from multi_part_assembly_amd import trainer as trainer_mod
from multi_part_assembly_amd.optim import FlatBuffers, FusedAdam
from multi_part_assembly_amd.trainer import Trainer


# ---- 1. which parameter owns a flat index ---------------------------------------------------------------------------------------
def _layout():
    """Sizes 1, 5 and 4 at offsets 0, 4 and 12: two paddings, [1, 4) and [9, 12)."""
    flat = FlatBuffers([nn.Parameter(torch.zeros(1)), nn.Parameter(torch.zeros(5)), nn.Parameter(torch.zeros(2, 2))])
    assert flat.offsets == [0, 4, 12] and flat.numel == 16
    return flat


OWNERS = {0: (0, (1,), 0),                                   # the one element of the first tensor
          2: (0, (1,), 2),                                   # its padding: the tensor in front, element >= numel
          4: (1, (5,), 0), 8: (1, (5,), 4), 10: (1, (5,), 6),  # first, last, padding
          12: (2, (2, 2), 0), 15: (2, (2, 2), 3)}            # first and last = numel - 1


def test_owner_is_the_last_parameter_whose_offset_is_not_behind_the_index():
    flat = _layout()
    assert {i: flat.owner(i) for i in OWNERS} == OWNERS
    assert flat.owner(flat.numel - 1) == (2, (2, 2), 3)


@pytest.mark.parametrize("index", sorted(OWNERS))
def test_guard_report_and_the_checkpoint_refusal_name_the_same_owner(monkeypatch, index):
    flat = _layout()
    opt = FusedAdam(flat, guard=True)
    opt.guard_words().copy_(torch.tensor([1, 0, 1, 1, index, 1, 1, 0], dtype=torch.int32))
    rep = opt.guard_report()
    assert (rep["parameter"], rep["shape"], rep["element"]) == OWNERS[index]
    # the refusal: a trainer's `_refuse_nonfinite_state` on this layout, the finite-ness pass stood in for
    t = Trainer.__new__(Trainer)
    on_device = types.SimpleNamespace(is_cuda=True)  # (the refusal looks at device tensors only)
    t.flat, t.optimizer = types.SimpleNamespace(flat_param=on_device, owner=flat.owner), opt
    monkeypatch.setattr(opt, "first_nonfinite", lambda tensor: index)
    k, shape, element = OWNERS[index]
    with pytest.raises(RuntimeError) as err:
        t._refuse_nonfinite_state()
    assert f"parameter {k} (shape {shape}) holds a non-finite value at element {element};" in str(err.value)


# ---- 2. the use_graph refusals -----------------------------------------------------------------------------------------------------
class Marked(nn.Module):
    """A model showing the marks it is given."""

    def __init__(self, sub_mark=False, **marks):
        super().__init__()
        self.head = nn.Linear(3, 2)
        self.encoder = nn.Linear(2, 3)
        self.encoder.host_sync_per_forward = sub_mark
        for name, value in marks.items():
            setattr(self, name, value)


REASONS = {
    "semantic": (dict(semantic=True), "models with semantic part matching (the matching's point sample is drawn on the host "
                                      "every step)"),
    "draws": (dict(host_draws_per_forward=True), "Marked (its teacher-forcing coin and decoder noise are drawn on the host every "
                                                  "forward)"),
    "sync": (dict(sub_mark=True), "Marked (its encoder synchronises with the host in every forward to compact the valid parts)"),
}


@pytest.mark.parametrize("which", list(REASONS))
def test_each_mark_refuses_the_capture_with_its_reason(which):
    marks, reason = REASONS[which]
    model = Marked(**marks)
    assert trainer_mod.graph_refusal(model) == reason
    with pytest.warns(UserWarning) as seen:
        t = Trainer(model, config.pn_transformer_everyday(), use_graph=True)
    assert [str(w.message) for w in seen] == [f"Trainer: use_graph=True is not available for {reason}; running eager launches"]
    assert t.use_graph is False and t.reducer.enabled


def test_no_mark_leaves_use_graph_as_asked():
    assert trainer_mod.graph_refusal(Marked()) is None
    assert trainer_mod.graph_refusal(Marked(semantic=True, match_sample="device")) is None  # (the draw is a kernel)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert Trainer(Marked(), config.pn_transformer_everyday(), use_graph=True).use_graph is True
        assert Trainer(Marked(), config.pn_transformer_everyday(), use_graph=False).use_graph is False
        assert Trainer(Marked(semantic=True), config.pn_transformer_everyday(), use_graph=False).use_graph is False


# ---- 3. mark and collectives on the paths without the reducer's hooks ---------------------------------------------------------------
# Recorded with this recorder on the three places that spelled the sequence before `_reduce_grad` (the warm-up step of
# `_graph_step`, its replay around the second graph, its replay without one), on this model: head 0..12, encoder 12..24.
MARK, SECOND = ("launch", "mpa_guard_mark"), ("second_half",)
EXPECTED = {
    ("warmup", True): [MARK, ("all_reduce", 0, 24)],
    ("warmup", False): [("all_reduce", 0, 24)],
    ("second", True): [MARK, ("all_reduce", 0, 12), SECOND, ("all_reduce", 12, 12), ("wait", 0), ("wait", 12)],
    ("second", False): [("all_reduce", 0, 12), SECOND, ("all_reduce", 12, 12), ("wait", 0), ("wait", 12)],
    ("none", True): [MARK, ("all_reduce", 0, 24)],
    ("none", False): [("all_reduce", 0, 24)],
    ("second_one_bucket", True): [SECOND, MARK, ("all_reduce", 0, 24), ("wait", 0)],
    ("second_one_bucket", False): [SECOND, ("all_reduce", 0, 24), ("wait", 0)],
}


@pytest.mark.parametrize("guard", [True, False], ids=["guarded", "unguarded"])
@pytest.mark.parametrize("site", ["warmup", "second", "none", "second_one_bucket"])
def test_the_mark_comes_directly_in_front_of_the_collective_holding_element_zero(monkeypatch, site, guard):
    events = []
    t = Trainer(Marked(), config.pn_transformer_everyday(), guard_step=guard, use_graph=True)
    t.world = 2
    t.optimizer.launch_status = torch.zeros(1, dtype=torch.int32)
    base = t.flat.flat_grad.data_ptr()

    class Work:
        def __init__(self, start):
            self.start = start

        def wait(self):
            events.append(("wait", self.start))

    def all_reduce(tensor, op=None, group=None, async_op=False):
        start = (tensor.data_ptr() - base) // 4
        events.append(("all_reduce", start, tensor.numel()))
        return Work(start) if async_op else None

    monkeypatch.setattr(_lib, "launch", lambda name, dev, *args, **kw: events.append(("launch", name)))
    monkeypatch.setattr(dist, "all_reduce", all_reduce)
    if site == "second_one_bucket":
        t.reducer.buckets = [{"slice": t.flat.flat_grad, "count": len(t.flat.params), "ready": 0}]
    if site in ("warmup", "none"):
        t._reduce_grad()
    else:
        t._reduce_grad(lambda: events.append(SECOND))
    assert events == EXPECTED[(site, guard)]
    # the mark: once and directly in front of the collective whose range contains element 0 when guarded, else nowhere
    assert events.count(MARK) == int(guard)
    if guard:
        nxt = events[events.index(MARK) + 1]
        assert nxt[0] == "all_reduce" and nxt[1] == 0
    # one rank: no collective and no mark on any path
    events.clear()
    t.world = 1
    t._reduce_grad()
    assert events == []
