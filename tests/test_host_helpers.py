"""The host layer's shared helpers on the CPU: the parameter-gradient hand-back of gradsink.py under a toy Function whose
"kernel" is `copy_`, and `loss.sum_loss_rounds` on whole [K, B] tensors against the same values term by term."""
import pytest
import torch

from multi_part_assembly_amd.gradsink import GradSink
from multi_part_assembly_amd.loss import LossTerms, sum_loss_rounds


class _Toy(torch.autograd.Function):
    """y = x; d loss / d param k := (k + 1) * sum(grad_y), written by `copy_` into the buffers the hand-back names."""
    seen = []

    @staticmethod
    def forward(ctx, x, label, *params):
        GradSink.register(ctx, params)
        return x * 1.0

    @staticmethod
    def backward(ctx, grad_y):
        grads = GradSink.outputs(ctx.params)
        for k, (buf, p) in enumerate(zip(grads.buffers, ctx.params)):
            assert (buf is None) == (p is None)
            if p is not None:
                buf.copy_(torch.full(p.shape, float(k + 1)) * grad_y.sum())
        back = grads.handed_back()
        _Toy.seen.append((grads.buffers, back))
        return (grad_y, None, *back)


def _params():
    g = torch.Generator().manual_seed(1)
    return [torch.nn.Parameter(torch.randn(3, 4, generator=g)), torch.nn.Parameter(torch.randn(5, generator=g))]


def _step(params, sink, calls=1, x=None):
    """`calls` uses of the parameters in one step -> their .grad's."""
    _Toy.seen.clear()
    x = torch.tensor([0.3, 1.7]) if x is None else x
    with (sink if sink is not None else torch.enable_grad()):
        loss = sum((_Toy.apply(x * (c + 1), "label", *params) * (0.1 + c)).sum() for c in range(calls))
        loss.backward()
    return [None if p is None else p.grad for p in params]


def test_hand_back_writes_into_zeroed_grads_and_returns_none():
    params = _params()
    for p in params:
        p.grad = torch.zeros_like(p)
    own = [p.grad for p in params]
    fired = []
    got = _step(params, GradSink(on_ready=fired.append))
    (buffers, back), = _Toy.seen
    assert all(b is g for b, g in zip(buffers, own)) and all(g is o for g, o in zip(got, own))  # the buffers ARE .grad
    assert back == (None, None) and len(back) == len(params)
    assert len(fired) == 2 and all(f is p for f, p in zip(fired, params))  # once per parameter
    want = _step(_params(), None)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert GradSink.active is None


def test_a_parameter_used_twice_falls_back_and_accumulates_to_the_same_bits():
    params = _params()
    for p in params:
        p.grad = torch.zeros_like(p)
    own = [p.grad for p in params]
    fired = []
    got = _step(params, GradSink(on_ready=fired.append), calls=2)
    assert len(_Toy.seen) == 2 and not fired
    for buffers, back in _Toy.seen:
        assert len(back) == len(params) and all(b is t for b, t in zip(back, buffers))  # returned, for autograd to add
        assert not any(b is o for b in buffers for o in own)
    ref = _params()
    for p in ref:
        p.grad = torch.zeros_like(p)
    want = _step(ref, None, calls=2)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and float(got[0].abs().max()) > 0


@pytest.mark.parametrize("how", ["none", "non_contiguous", "no_sink"])
def test_a_grad_that_cannot_be_overwritten_falls_back(how):
    params = _params()
    params[1].grad = torch.zeros_like(params[1])
    if how == "non_contiguous":
        params[0].grad = torch.zeros(4, 3).t()
        assert not params[0].grad.is_contiguous()
    fired = []
    got = _step(params, None if how == "no_sink" else GradSink(on_ready=fired.append))
    (buffers, back), = _Toy.seen
    assert not fired and len(back) == len(params) and all(b is t for b, t in zip(back, buffers))
    assert all(b is not params[1].grad for b in buffers)  # all or nothing: one launch writes every gradient
    want = _step(_params(), None)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_an_absent_parameter_keeps_its_place_in_the_hand_back():
    w, b = _params()
    w.grad = torch.zeros_like(w)
    fired = []
    _step([w, None], GradSink(on_ready=fired.append))
    (buffers, back), = _Toy.seen
    assert buffers[0] is w.grad and buffers[1] is None and back == (None, None) and fired == [w]
    w.grad = None
    _step([w, None], None)
    (buffers, back), = _Toy.seen
    assert len(back) == 2 and back[0] is buffers[0] and back[1] is None and torch.equal(w.grad, buffers[0])


# ---- loss summed over rounds --------------------------------------------------------------------------------------------
NAMES = ("trans_loss", "rot_pt_cd_loss", "transform_pt_cd_loss", "rot_loss")


def _rounds(stacked):
    g = torch.Generator().manual_seed(4)
    out = []
    for r, keep in enumerate(stacked):
        t = torch.rand(len(NAMES), 5, generator=g) * 10.0 ** (r - 1)
        terms = LossTerms((k, t[j]) for j, k in enumerate(NAMES))
        if keep:
            terms.stacked = (NAMES, t)
        out.append(terms if keep is not None else dict(terms))
    return out


def test_rounds_sum_whole_tensors_to_the_bits_of_the_term_by_term_sum():
    whole = sum_loss_rounds(_rounds([True, True, True]))
    plain = sum_loss_rounds(_rounds([None, None, None]))
    mixed = sum_loss_rounds(_rounds([True, False, True]))
    keys = list(NAMES) + [f"{k}_{i}" for i in range(3) for k in NAMES]
    assert list(whole) == list(plain) == list(mixed) == keys
    for k in keys:
        assert torch.equal(whole[k], plain[k]) and torch.equal(mixed[k], plain[k]), k
    names, full = whole.stacked
    assert names == tuple(keys) and full.shape == (len(keys), 5)
    assert all(torch.equal(full[j], plain[k]) for j, k in enumerate(keys))
    assert getattr(plain, "stacked", None) is None and getattr(mixed, "stacked", None) is None
    rounds = _rounds([True, True, True])
    assert torch.equal(whole["rot_loss"], rounds[0]["rot_loss"] + rounds[1]["rot_loss"] + rounds[2]["rot_loss"])
