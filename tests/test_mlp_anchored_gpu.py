"""One layer of csrc/mlp.hip at a time — mlp.mlp_layer (Linear [+ BatchNorm1d] [+ ReLU] over rows) and mlp.pair_layer (the
edge MLP's first layer on (a_i, b_j) pairs without the pair tensor) — against oracle.callers.mlp_layer evaluated in
FLOAT64 on the CPU, under the bars of tests/anchored.py: the output, the running statistics after one training call, the
input gradient and every parameter gradient.  A single layer has its only ReLU last, so the entries whose float64
pre-activation lies within FLIP_PREACT of zero are pinned (their loss weight is zero: anchored._pin_relu) and no escape
for ReLU flips is needed.  gamma has negative entries and one exact zero in every BatchNorm case.

The shapes are the smallest that reach each branch of the dispatch:

  rows R <= 2048 (tf_gemm.h: one 32 x 32 tile per block, K in phases; BatchNorm in one launch per pass over 256-row slabs)
    R = 5, 31, 33, 257, 2048: below / on either side of the 32-row tile edge, one row past a 256-row slab, the last small R
    K -> N = 64->64 (one 64-wide phase), 192->320 and 384->192 (the generic phase loop, 64- and 128-wide), 768->64 and
    1024->128 (6 and 8 phases), 128->768; the input gradient multiplies over N, so each of these kernels also runs as dX
  rows R > 2048 (dg_gemm_split.h: 128-row tiles, split-bf16 products; row-tiled BatchNorm; chunked weight gradient)
    R = 2049 = 16 * 128 + 1 and 2177 = 17 * 128 + 1; 64->64, 192->320, 320->192, 128->128: N % 128 and K % 128 both ways
    (the 64- and 128-column kernels forward and as dX, gemm_tn_split_kernel<64> and <128>), 32 row chunks of 96 rows of
    which the last ones receive no rows
  no BatchNorm, R = 1, 33, 2049, 256->512 and 192->64: bias + ReLU, bias alone, no bias (above 2048 rows the weight
    gradient's plain chunk sum), x as data (no input gradient)
  pair layer (B, P, F, N): (1, 2, 64, 64) has 4 pair rows, (3, 5, 192, 192) 75 (no multiple of the 16-row tiles),
    (2, 46, 64, 128) 4232 from 92 part rows, one weight-gradient chunk; each with distinct a and b, one tensor in both
    roles (its gradient is the in-place sum) and b as data
"""
import pytest
import torch

import anchored as A

pytestmark = pytest.mark.gpu


def _modules(sd, dev):
    """(nn.Linear, nn.BatchNorm1d or None) on the device holding the case's parameters."""
    N, K = sd["lin.weight"].shape
    lin = torch.nn.Linear(K, N, bias="lin.bias" in sd)
    lin.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("lin.")})
    bn = None
    if "bn.weight" in sd:
        bn = torch.nn.BatchNorm1d(N)
        bn.load_state_dict({k[3:]: v for k, v in sd.items() if k.startswith("bn.")}, strict=False)
    return lin.to(dev), (bn.to(dev) if bn is not None else None)


def _collect(y, lin, bn, gin):
    res = {"out.y": y}
    res.update({"gin." + k: v.grad for k, v in gin.items()})
    res.update({"grad.lin." + k: p.grad for k, p in lin.named_parameters()})
    if bn is not None:
        res.update({"grad.bn." + k: p.grad for k, p in bn.named_parameters()})
        res.update({"out.stat.bn.running_mean": bn.running_mean, "out.stat.bn.running_var": bn.running_var})
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in res.items()}


def _layer(dev, case, sd, inputs, wrt, x=None):
    """One training-mode forward + backward of mlp.mlp_layer on fresh modules; `x`: the device input to use instead."""
    from multi_part_assembly_amd import mlp
    relu = case[3] in ("bn", "bias-relu", "nobias", "data")
    lin, bn = _modules(sd, dev)
    x = inputs["x"].to(dev) if x is None else x
    x.requires_grad_("x" in wrt)
    y = mlp.mlp_layer(x, lin.weight, lin.bias, bn, relu=relu, training=True)
    (y * inputs["w"].to(dev)).sum().backward()
    if bn is not None:
        assert int(bn.num_batches_tracked) == 1
    return _collect(y, lin, bn, {"x": x} if "x" in wrt else {})


def _family(case):
    return "no-BatchNorm" if not case[3].startswith("bn") else ("small path" if case[0] <= 2048 else "big path")


@pytest.mark.parametrize("case", A.MLP_LAYER_CASES, ids=A.case_id)
def test_mlp_layer_against_the_float64_oracle(cuda_device, capsys, case):
    from multi_part_assembly_amd import mlp
    R, K, N, mode = case
    assert mlp.supported(K, N)
    sd, inputs, wrt, share = A.mlp_layer_case(case)
    assert share <= A.PIN_SHARE
    r32, r64 = A.oracle_pair(A.mlp_layer_fn(case), sd, inputs, wrt)
    got = _layer(cuda_device, case, sd, inputs, wrt)
    assert set(got) == set(r64) and ("gin.x" in got) == (mode != "data"), sorted(set(got) ^ set(r64))
    A.assert_anchored(got, r32, r64, f"MLP layer {_family(case)} {case}, pinned {share:.1e}", capsys)
    A.assert_bit_equal(got, _layer(cuda_device, case, sd, inputs, wrt))


@pytest.mark.parametrize("case", [(257, 192, 320, "bn"), (2177, 192, 320, "bn")], ids=A.case_id)
def test_mlp_layer_eval_mode_and_a_strided_input(cuda_device, capsys, case):
    """Evaluation-mode BatchNorm (output only; the running statistics and the batch counter stay as they are, bit for
    bit) and a strided input — the first K columns of a [R, K + 64] tensor — against its contiguous copy, bit for bit."""
    from multi_part_assembly_amd import mlp
    R, K, N, mode = case
    sd, inputs, wrt, share = A.mlp_layer_case(case)
    fn = A.mlp_layer_fn(case, training=False)
    e32, e64 = (A.oracle_run(fn, sd, inputs, (), dt) for dt in (torch.float32, torch.float64))
    lin, bn = _modules(sd, cuda_device)
    bn.eval()
    with torch.no_grad():
        y = mlp.mlp_layer(inputs["x"].to(cuda_device), lin.weight, lin.bias, bn, relu=True, training=False)
    assert torch.equal(bn.running_mean.cpu(), sd["bn.running_mean"]) and torch.equal(bn.running_var.cpu(), sd["bn.running_var"])
    assert int(bn.num_batches_tracked) == 0
    A.assert_anchored({"out.y": y.cpu()}, {"out.y": e32["out.y"]}, {"out.y": e64["out.y"]},
                      f"MLP layer {_family(case)} {case}, eval mode", capsys)

    wide = torch.zeros(R, K + 64, device=cuda_device)
    wide[:, :K] = inputs["x"].to(cuda_device)
    wide[:, K:] = float("nan")  # nothing may read past the K columns
    strided = wide[:, :K].detach()
    assert strided.stride() == (K + 64, 1)
    A.assert_bit_equal(_layer(cuda_device, case, sd, inputs, wrt), _layer(cuda_device, case, sd, inputs, wrt, x=strided))


@pytest.mark.parametrize("case", A.PAIR_LAYER_CASES, ids=A.case_id)
def test_pair_layer_against_the_float64_oracle_over_the_pair_rows(cuda_device, capsys, case):
    from multi_part_assembly_amd import mlp
    B, P, F, N, mode = case
    assert mlp.pair_layer_supported(F, N)
    sd, inputs, wrt, share = A.pair_layer_case(case)
    assert share <= A.PIN_SHARE
    r32, r64 = A.oracle_pair(A.pair_layer_fn(case), sd, inputs, wrt)

    def run():
        lin, bn = _modules(sd, cuda_device)
        a = inputs["a"].to(cuda_device).requires_grad_()
        b = a if mode == "same" else inputs["b"].to(cuda_device).requires_grad_(mode == "distinct")
        y = mlp.pair_layer(a, b, lin.weight, lin.bias, bn, relu=True, training=True)
        (y * inputs["w"].to(cuda_device)).sum().backward()
        assert int(bn.num_batches_tracked) == 1
        return _collect(y, lin, bn, {"a": a, "b": b} if mode == "distinct" else {"a": a})

    got = run()
    assert set(got) == set(r64), sorted(set(got) ^ set(r64))
    A.assert_anchored(got, r32, r64, f"pair layer {case}, {B * P * P} rows, pinned {share:.1e}", capsys)
    A.assert_bit_equal(got, run())
