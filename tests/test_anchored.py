"""CPU tests of the float64-anchored bars of tests/anchored.py themselves: on the oracle alone (no GPU) they show that
the bar separates rounding from error.  A float32 evaluation in another summation order passes; a float32 evaluation
with one defect of the kind a HIP kernel could have — a weight that lost the third term of its bf16 split, a wrong
epsilon, one gradient tensor off by 2e-5 — is rejected; and the bar stays between its median term and 1e-4 on every
shape of the GPU tests.  For the GRU recurrence, the MLP layer and the pair layer (csrc/gru.hip, csrc/mlp.hip) they pin the
oracle functions to torch's modules in float64, check every case (ReLU pinning share, no all-zero anchor, e32 below the
ceiling) and show one planted error per family rejected and a re-associated float32 evaluation accepted."""
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


# ---- the GRU recurrence, the MLP layer and the pair layer (csrc/gru.hip, csrc/mlp.hip) ------------------------------------

def _gru(dims):
    key = ("gru", dims)
    if key not in _cache:
        sd, inputs = A.gru_case(dims)
        _cache[key] = (A.gru_fn, sd, inputs, A.GRU_WRT, 0.0) + A.oracle_pair(A.gru_fn, sd, inputs, A.GRU_WRT)
    return _cache[key]


def _gru_wrapper(dims):
    key = ("gruw", dims)
    if key not in _cache:
        mod, inputs = A.gru_wrapper_case(dims)
        sd = {k: t.detach().clone() for k, t in mod.state_dict().items()}
        _cache[key] = (A.gru_wrapper_fn, sd, inputs, ("x",), 0.0) + A.oracle_pair(A.gru_wrapper_fn, sd, inputs, ("x",))
    return _cache[key]


def _mlp_layer(case):
    key = ("mlp", case)
    if key not in _cache:
        sd, inputs, wrt, share = A.mlp_layer_case(case)
        fn = A.mlp_layer_fn(case)
        _cache[key] = (fn, sd, inputs, wrt, share) + A.oracle_pair(fn, sd, inputs, wrt)
    return _cache[key]


def _pair_layer(case):
    key = ("pair", case)
    if key not in _cache:
        sd, inputs, wrt, share = A.pair_layer_case(case)
        fn = A.pair_layer_fn(case)
        _cache[key] = (fn, sd, inputs, wrt, share) + A.oracle_pair(fn, sd, inputs, wrt)
    return _cache[key]


LAYER_CASES = ([(_gru, c) for c in A.GRU_CASES] + [(_gru_wrapper, c) for c in A.GRU_WRAPPER_CASES] +
               [(_mlp_layer, c) for c in A.MLP_LAYER_CASES] + [(_pair_layer, c) for c in A.PAIR_LAYER_CASES])
LAYER_IDS = [get.__name__[1:] + "-" + A.case_id(c) for get, c in LAYER_CASES]


def test_the_flip_constant_is_the_one_of_the_caller_tests():
    import test_callers_gpu
    assert A.FLIP_PREACT == test_callers_gpu.FLIP_PREACT


def test_the_gru_oracle_is_torch_gru_in_float64():
    """oracle.callers.gru_recurrent behind the input projection against torch.nn.GRU on the CPU, both directions; the
    reverse direction is fed the reversed input (and its output is reversed back)."""
    from oracle import callers as oc
    B, T, H = 3, 4, 8
    torch.manual_seed(3)
    gru = torch.nn.GRU(H, H, 1, batch_first=True, bidirectional=True).double()
    x, h0 = torch.randn(B, T, H, dtype=torch.float64), torch.randn(2, B, H, dtype=torch.float64)
    gru.requires_grad_(False)
    want, _ = gru(x, h0)
    lin = torch.nn.functional.linear
    gi = torch.stack([lin(x, gru.weight_ih_l0, gru.bias_ih_l0), lin(x.flip(1), gru.weight_ih_l0_reverse, gru.bias_ih_l0_reverse)])
    got = oc.gru_recurrent(gi, h0, torch.stack([gru.weight_hh_l0, gru.weight_hh_l0_reverse]),
                           torch.stack([gru.bias_hh_l0, gru.bias_hh_l0_reverse]))
    assert got.dtype == torch.float64 and got.shape == (2, B, T, H)
    assert float((got[0] - want[..., :H]).abs().max()) <= 1e-12
    assert float((got[1].flip(1) - want[..., H:]).abs().max()) <= 1e-12


@pytest.mark.parametrize("bn,bias,relu,training", [(True, True, True, True), (True, True, False, True), (True, True, True, False),
                                                   (False, True, True, True), (False, False, False, True)])
def test_the_mlp_layer_oracle_is_linear_batchnorm_relu_in_float64(bn, bias, relu, training):
    from oracle import callers as oc
    R, K, N = 7, 12, 10
    torch.manual_seed(4)
    lin, norm = torch.nn.Linear(K, N, bias=bias).double(), torch.nn.BatchNorm1d(N).double()
    with torch.no_grad():
        norm.weight.uniform_(-1.0, 1.5)
        norm.bias.normal_()
        norm.running_mean.normal_()
        norm.running_var.uniform_(0.5, 1.5)
    lin.train(training), norm.train(training)
    sd = {"lin." + k: v.detach().clone() for k, v in lin.state_dict().items()}
    sd.update({"bn." + k: v.detach().clone() for k, v in norm.state_dict().items()})
    x = torch.randn(R, K, dtype=torch.float64)
    pre = norm(lin(x)) if bn else lin(x)
    want = torch.relu(pre) if relu else pre
    stats = {}
    got, got_pre = oc.mlp_layer(x, sd, "", bn, relu, training, stats, return_preact=True)
    assert float((got - want).abs().max()) <= 1e-12 and float((got_pre - pre).abs().max()) <= 1e-12
    assert torch.equal(got, oc.mlp_layer(x, sd, "", bn, relu, training, None))
    if bn and training:
        for k in ("running_mean", "running_var"):
            assert float((stats["bn." + k] - getattr(norm, k)).abs().max()) <= 1e-12
            assert not torch.equal(stats["bn." + k], sd["bn." + k])
    else:
        assert not stats


@pytest.mark.parametrize("get,case", LAYER_CASES, ids=LAYER_IDS)
def test_layer_cases_are_pinned_nonzero_and_within_their_own_bars(get, case):
    """For every case of the GRU and MLP GPU tests: the ReLU pinning takes at most PIN_SHARE of the output entries out of
    the loss, no compared float64 tensor is all zero (apart from the structurally zero bias gradients), and the float32
    oracle passes its own bars (every e32 is below CEIL)."""
    fn, sd, inputs, wrt, share, r32, r64 = get(case)
    assert share <= A.PIN_SHARE, share
    assert set(r32) == set(r64) and any(k.startswith("grad.") for k in r64)
    for k, v in r64.items():
        if A._zero_scale(k, r64) is None:
            assert float(v.abs().max()) > 0.0, k
        else:
            assert k == "grad.lin.bias", k
    zero_bias = "grad.lin.bias" in r64 and A._zero_scale("grad.lin.bias", r64) is not None
    assert zero_bias == ("bn.weight" in sd)  # a bias in front of a BatchNorm, and only that
    A.assert_anchored(r32, r32, r64, "float32 oracle")


def test_the_pinning_zeroes_the_weights_next_to_a_flip():
    """A pre-activation planted at 1e-6 of its channel's scale is found and its loss weight zeroed; the others stay."""
    sd = {"lin.weight": torch.eye(64)}
    x = torch.randn(9, 64, generator=torch.Generator().manual_seed(0))
    x[:, 0] = torch.tensor([2.0, 2e-6, -2e-6, 1.1e-5, -1.0, 0.5, 0.0, 1.0, -2.0])
    inputs = {"x": x, "w": torch.ones(9, 64)}
    share = A._pin_relu(A.mlp_layer_fn((9, 64, 64, "nobias"), preact=True), sd, inputs)
    assert inputs["w"][:, 0].tolist() == [1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 1.0, 1.0]
    assert share == 3 / (9 * 64) and float(inputs["w"][:, 1:].min()) == 1.0


GRU_PLANT = (2, 33, 3, 256)
MLP_PLANT = (5, 64, 64, "bn")
PAIR_PLANT = (3, 5, 192, 192, "distinct")


def test_a_gru_with_b_hn_outside_the_reset_product_is_rejected(monkeypatch):
    from oracle import callers as oc
    fn, sd, inputs, wrt, _, r32, r64 = _gru(GRU_PLANT)

    def wrong(gi, h0, whh, bhh):  # n = tanh(gi_n + r * (W_hn h) + b_hn): the "other" GRU convention
        H = h0.shape[-1]
        h, out = h0, []
        for t in range(gi.shape[2]):
            gh = torch.matmul(h, whh.transpose(1, 2))
            g = gi[:, :, t] + bhh[:, None]
            r = torch.sigmoid(g[..., :H] + gh[..., :H])
            z = torch.sigmoid(g[..., H:2 * H] + gh[..., H:2 * H])
            h = (1.0 - z) * torch.tanh(g[..., 2 * H:] + r * gh[..., 2 * H:]) + z * h
            out.append(h)
        return torch.stack(out, dim=2)

    monkeypatch.setattr(oc, "gru_recurrent", wrong)
    got = A.oracle_run(fn, sd, inputs, wrt, torch.float32)
    with pytest.raises(AssertionError, match="> bar"):
        A.assert_anchored(got, r32, r64)


def test_a_running_variance_from_the_biased_variance_is_rejected():
    fn, sd, inputs, wrt, _, r32, r64 = _mlp_layer(MLP_PLANT)
    y = torch.nn.functional.linear(inputs["x"], sd["lin.weight"], sd["lin.bias"])
    got = dict(r32)
    got["out.stat.bn.running_var"] = 0.9 * sd["bn.running_var"] + 0.1 * y.var(dim=0, unbiased=False)
    rows, bad = A.check(got, r32, r64)
    assert len(bad) == 1 and bad[0].startswith("out.stat.bn.running_var"), bad
    got["out.stat.bn.running_var"] = 0.9 * sd["bn.running_var"] + 0.1 * y.var(dim=0, unbiased=True)
    A.assert_anchored(got, r32, r64)


def test_a_pair_layer_with_swapped_weight_halves_is_rejected():
    fn, sd, inputs, wrt, _, r32, r64 = _pair_layer(PAIR_PLANT)
    F = PAIR_PLANT[2]
    bad_sd = dict(sd)
    bad_sd["lin.weight"] = torch.cat([sd["lin.weight"][:, F:], sd["lin.weight"][:, :F]], dim=1)
    got = A.oracle_run(fn, bad_sd, inputs, wrt, torch.float32)
    with pytest.raises(AssertionError, match="> bar"):
        A.assert_anchored(got, r32, r64)


def test_re_associated_float32_layers_pass():
    """The same three cases in float32 in another summation order: the GRU's batch in two parts (samples do not interact;
    the weight and bias gradients are summed), the MLP layer's rows permuted (BatchNorm's sums and every parameter
    gradient add up in another order), the pair layer's samples permuted."""
    fn, sd, inputs, wrt, _, r32, r64 = _gru(GRU_PLANT)
    parts = [A.oracle_run(fn, sd, {k: v[:, s] for k, v in inputs.items()}, wrt, torch.float32)
             for s in (slice(0, 16), slice(16, None))]
    other = {k: torch.cat([p[k] for p in parts], dim=1) if k.startswith(("out.", "gin.")) else parts[0][k] + parts[1][k]
             for k in parts[0]}
    assert _differs(other, r32)
    A.assert_anchored(other, r32, r64, "GRU in two parts")

    fn, sd, inputs, wrt, _, r32, r64 = _mlp_layer(MLP_PLANT)
    pm = torch.randperm(MLP_PLANT[0], generator=torch.Generator().manual_seed(1))
    other = A.oracle_run(fn, sd, {k: v[pm] for k, v in inputs.items()}, wrt, torch.float32)
    back = torch.argsort(pm)
    other["out.y"], other["gin.x"] = other["out.y"][back], other["gin.x"][back]
    assert _differs(other, r32)
    A.assert_anchored(other, r32, r64, "MLP layer, rows permuted")

    fn, sd, inputs, wrt, _, r32, r64 = _pair_layer(PAIR_PLANT)
    B, P, F, N, _ = PAIR_PLANT
    pm = torch.tensor([2, 0, 1])
    back = torch.argsort(pm)
    perm = {"a": inputs["a"][pm], "b": inputs["b"][pm], "w": inputs["w"].view(B, P * P, N)[pm].reshape(B * P * P, N)}
    other = A.oracle_run(fn, sd, perm, wrt, torch.float32)
    other["out.y"] = other["out.y"].view(B, P * P, N)[back].reshape(B * P * P, N)
    other["gin.a"], other["gin.b"] = other["gin.a"][back], other["gin.b"][back]
    assert _differs(other, r32)
    A.assert_anchored(other, r32, r64, "pair layer, samples permuted")
