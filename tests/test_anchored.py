"""CPU tests of the float64-anchored bars of tests/anchored.py themselves: on the oracle alone (no GPU) they show that
the bar separates rounding from error.  A float32 evaluation in another summation order passes; a float32 evaluation
with one defect of the kind a HIP kernel could have — a weight that lost the third term of its bf16 split, a wrong
epsilon, one gradient tensor off by 2e-5 — is rejected; and the bar stays between its median term and 1e-4 on every
shape of the GPU tests."""
import pytest
import torch

import anchored as A
from oracle import nets as on

PN = [A.POINTNET_CASES[i] for i in (1, 4, 5)]          # (5, 31, 128), (7, 65, 64) with padded parts, (3, 97, 128)
TF = [A.TRANSFORMER_CASES[i] for i in (8, 10, 12)]     # (2,33,256,8,1024,2), (3,20,64,8,256,2), (2,5,256,8,64,1)
_cache = {}


def _pointnet(case):
    """(fn, sd, inputs, wrt, r32, r64) of a PointNet case; the oracle pair is computed once and shared."""
    key = ("pn", case)
    if key not in _cache:
        shape, valids = case
        enc, pts, v, w = A.pointnet_case(shape, valids)
        keep = v > 0
        sd = {k: t.detach().clone() for k, t in enc.state_dict().items()}
        inputs = {"pts": pts[keep], "w": w[keep]}
        _cache[key] = (A.pointnet_fn(True), sd, inputs, ()) + A.oracle_pair(A.pointnet_fn(True), sd, inputs)
    return _cache[key]


def _transformer(dims):
    key = ("tf", dims)
    if key not in _cache:
        enc, tok, valid, w = A.transformer_case(dims)
        sd = {k: t.detach().clone() for k, t in enc.state_dict().items()}
        inputs = {"tok": tok, "valid": valid, "w": w}
        fn = A.transformer_fn(dims)
        _cache[key] = (fn, sd, inputs, ("tok",)) + A.oracle_pair(fn, sd, inputs, ("tok",))
    return _cache[key]


def _pose_head(case):
    key = ("head", case)
    if key not in _cache:
        head, x, w_r, w_t = A.pose_head_case(*case)
        sd = {k: t.detach().clone() for k, t in head.state_dict().items()}
        inputs = {"x": x, "w_rot": w_r, "w_trans": w_t}
        _cache[key] = (A.pose_head_fn, sd, inputs, ("x",)) + A.oracle_pair(A.pose_head_fn, sd, inputs, ("x",))
    return _cache[key]


def _case(kind, case):
    return _pointnet(case) if kind == "pn" else _transformer(case)


CASES = [("pn", c) for c in PN] + [("tf", c) for c in TF]
IDS = ["pn-%dx%dx%d" % c[0] for c in PN] + ["tf-" + "x".join(map(str, c)) for c in TF]


def _differs(a, b):
    return any(not torch.equal(a[k], b[k]) for k in a)


def _reassociated(kind, fn, sd, inputs, wrt):
    """The same float32 function in another summation order.  PointNet: the parts permuted (BatchNorm's sums and every
    weight gradient add up in another order; the points keep their order, since a zero bn5.weight makes every point of a
    part an exact tie of the max and the lowest index takes the gradient, here as in the kernels).  Transformer: the two
    halves of the batch evaluated one after the other (samples do not interact without dropout), parameter gradients
    summed."""
    if kind == "pn":
        g = torch.Generator().manual_seed(1)
        pm = torch.randperm(inputs["pts"].shape[0], generator=g)
        r = A.oracle_run(fn, sd, {"pts": inputs["pts"][pm], "w": inputs["w"][pm]}, wrt, torch.float32)
        r["out.feat"] = r["out.feat"][torch.argsort(pm)]
        return r
    h = inputs["tok"].shape[0] // 2
    parts = [A.oracle_run(fn, sd, {k: v[s] for k, v in inputs.items()}, wrt, torch.float32)
             for s in (slice(0, h), slice(h, None))]
    return {k: torch.cat([p[k] for p in parts]) if k.startswith(("out.", "gin.")) else parts[0][k] + parts[1][k]
            for k in parts[0]}


@pytest.mark.parametrize("kind,case", CASES, ids=IDS)
def test_a_float32_evaluation_in_another_order_passes(kind, case):
    fn, sd, inputs, wrt, r32, r64 = _case(kind, case)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        single = A.oracle_run(fn, sd, inputs, wrt, torch.float32)
    finally:
        torch.set_num_threads(threads)
    A.assert_anchored(single, r32, r64, "one thread")
    # small shapes do not split over threads and give the same bits: the re-association always differs
    other = _reassociated(kind, fn, sd, inputs, wrt)
    assert _differs(other, r32)
    A.assert_anchored(other, r32, r64, "re-associated")


def _round_to_bf16_pair(t):
    """Round to 16 significant bits: what the hi + mid terms of the three-term bf16 split of a float32 hold."""
    bits = t.contiguous().view(torch.int32)
    return ((bits + 0x80) & ~0xFF).view(torch.float32)


@pytest.mark.parametrize("kind,case", CASES, ids=IDS)
def test_a_weight_without_the_third_term_of_its_bf16_split_is_rejected(kind, case):
    fn, sd, inputs, wrt, r32, r64 = _case(kind, case)
    name = "conv1.weight" if kind == "pn" else "transformer_encoder.layers.0.self_attn.in_proj_weight"
    bad_sd = dict(sd)
    bad_sd[name] = _round_to_bf16_pair(sd[name])
    assert float((bad_sd[name] / sd[name] - 1).abs().max()) <= 2.0 ** -16
    got = A.oracle_run(fn, bad_sd, inputs, wrt, torch.float32)
    with pytest.raises(AssertionError, match="> bar"):
        A.assert_anchored(got, r32, r64)


@pytest.mark.parametrize("kind,case", CASES, ids=IDS)
def test_a_wrong_epsilon_is_rejected(kind, case, monkeypatch):
    fn, sd, inputs, wrt, r32, r64 = _case(kind, case)
    monkeypatch.setattr(on, "BN_EPS" if kind == "pn" else "LN_EPS", 1.1e-5)
    got = A.oracle_run(fn, sd, inputs, wrt, torch.float32)
    with pytest.raises(AssertionError, match="> bar"):
        A.assert_anchored(got, r32, r64)


@pytest.mark.parametrize("kind,case", CASES, ids=IDS)
def test_one_gradient_tensor_off_by_2e_5_is_rejected(kind, case):
    fn, sd, inputs, wrt, r32, r64 = _case(kind, case)
    names = ([f"grad.bn{i}.weight" for i in range(1, 6)] if kind == "pn" else
             [k for k in r32 if k.startswith("grad.") and "norm" in k and k.endswith(".weight")])
    assert names
    for name in names:  # every LayerNorm dgamma / BatchNorm weight gradient in turn
        got = dict(r32)
        got[name] = r32[name] * (1.0 + 2e-5)
        rows, bad = A.check(got, r32, r64)
        assert len(bad) == 1 and bad[0].startswith(name), (name, bad)


def test_bar_bounds_on_every_shape_of_the_gpu_tests():
    """min(CEIL, MULT x median e32) <= bar <= CEIL for every tensor, on every shape of the PointNet, transformer and
    pose-head tests."""
    for get, cases in ((_pointnet, A.POINTNET_CASES), (_transformer, A.TRANSFORMER_CASES), (_pose_head, A.POSE_HEAD_CASES)):
        for case in cases:
            *_, r32, r64 = get(case)
            e32, bar, med = A.bars(r32, r64)
            assert bar and med > 0.0, case
            for k, b in bar.items():
                assert min(A.CEIL, A.MULT * med) <= b <= A.CEIL, (case, k, b, med)
                assert b == A.CEIL or b >= A.MULT * e32[k], (case, k)


def test_structurally_zero_gradients_take_the_absolute_rule():
    r64 = {"grad.l.weight": torch.tensor([2.0, -1.0]), "grad.l.bias": torch.tensor([1e-12, 0.0]),
           "grad.m.weight": torch.tensor([1.0])}
    r32 = {k: v * (1 + 1e-7) for k, v in r64.items()}
    assert "grad.l.bias" not in A.bars(r32, r64)[0]
    assert not A.check({"grad.l.bias": torch.tensor([1.9e-5, 0.0])}, r32, r64)[1]
    assert A.check({"grad.l.bias": torch.tensor([2.1e-5, 0.0])}, r32, r64)[1]
    assert A.err(torch.zeros(3), torch.zeros(3)) == 0.0 and A.err(torch.ones(3), torch.zeros(3)) == float("inf")
    assert A.err(torch.tensor([float("nan")]), torch.ones(1)) == float("inf")
