"""The last layer's backward pass of PointNet (csrc/pn_bwd_q.h: pn_bwd_top_q_kernel) with the input gradient's epilogue in
the stager waves: the thread that fetched (row, 4 columns) of Y4 keeps them in one of three named register sets from the
request (unit u - 2) to the unit's epilogue (u + 1), reads A Q + c0 from `outp[u & 1]` and S W5 from `rowsum[u % 3]` one
barrier after the matrix waves consumed the unit, and writes dZ4 (through a buffer descriptor that ends with the part) and
the BatchNorm-backward sums.  Driven through the public path (`PointNet.forward_parts`, backward of a weighted sum of the
features) against oracle.nets.pointnet in float64 on the valid parts, every conv / bn gradient of the five layers under
the bars of tests/anchored.py.

The kernel runs 256 persistent blocks over 32-row units (valid part u / TB, row tile u % TB, TB = ceil(N / 32)); the
stagers' pipeline is three units deep and its loop is peeled into a ramp-up iteration, branch-free steady iterations
(0 < it, it + 3 < n_it) and three ramp-down iterations, so the shapes are the ones at which that hand-over changes its path:

  (3, 33, 256), valids 1,0,1   4 units: blocks 0-3 run one iteration (prologue, ramp-up and the final epilogue only), the
                               other 252 none; the second unit of each part holds ONE real row (31 of 32 fail the row
                               check: their dZ4 stores fall to the descriptor's range check)
  (32, 1000, 256), 28 valid    896 units: blocks 0-127 run 4 iterations, the others 3 (no steady iteration: ramp-up and
                               ramp-down meet); the last tile of a part has 8 real rows; run twice, bit-equal: nothing in
                               the hand-over may depend on timing
  (12, 64, 64), (12, 64, 128)  24 exact units, no ragged tile; the other two feature widths the operator admits
  (6, 97, 256), w[2] = 0       a valid part whose incoming feature gradient is zero: its tile records carry empty masks, so
                               the sparse slots of its units are all zeros and dZ4 is the dense term alone

  (40, 1000, 64)               1280 units, 5 per block: ramp-up, ONE steady iteration, ramp-down.  The steady iterations
                               need more than 4 units per block (> 1024 units), which neither the cases above nor those
                               of tests/anchored.py and tests/test_pn_top_rows_gpu.py reach
"""
import pytest
import torch

import anchored as A

pytestmark = pytest.mark.gpu

_VALID28 = tuple(0 if i % 8 == 5 else 1 for i in range(32))  # 28 valid parts, the padded ones interleaved


def _run(enc, pts, v, w):
    enc.zero_grad()
    out = enc.forward_parts(pts, v)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    res = {"out.feat": out.detach().clone()}
    res.update({"grad." + k: p.grad.detach().clone() for k, p in enc.named_parameters()})
    return res


def _case(cuda_device, shape, valids=None, zero_part=None, runs=1):
    """(runs on the GPU, float32 oracle, float64 oracle, mask of the valid parts) of one case."""
    enc, pts, v, w = A.pointnet_case(shape, valids)
    if zero_part is not None:
        w[zero_part] = 0.0
    sd0 = {k: t.detach().clone() for k, t in enc.state_dict().items()}
    keep = v > 0
    r32, r64 = A.oracle_pair(A.pointnet_fn(True), sd0, {"pts": pts[keep], "w": w[keep]})
    enc.to(cuda_device).train()
    dpts, dv, dw = pts.to(cuda_device), v.to(cuda_device), w.to(cuda_device)
    got = []
    for _ in range(runs):
        enc.load_state_dict(sd0)  # the same running statistics in front of every run
        got.append(_run(enc, dpts, dv, dw))
    return got, r32, r64, keep


def _assert_anchored(run, r32, r64, keep, label, capsys):
    feat = run["out.feat"].cpu()
    assert float(feat[~keep].abs().max() if (~keep).any() else 0.0) == 0.0  # rows of padded parts are zero
    got = {"out.feat": feat[keep], **{k: t.cpu() for k, t in run.items() if k.startswith("grad.")}}
    grads = {k for k in got if k.startswith("grad.")}
    for i in range(1, 6):  # every conv and BatchNorm weight of the five layers is among them
        assert {f"grad.conv{i}.weight", f"grad.bn{i}.weight", f"grad.bn{i}.bias"} <= grads, sorted(grads)
    assert set(got) <= set(r64), sorted(set(got) - set(r64))
    A.assert_anchored(got, {k: r32[k] for k in got}, {k: r64[k] for k in got}, label, capsys)


@pytest.fixture(scope="module")
def valid28(cuda_device):
    return _case(cuda_device, (32, 1000, 256), _VALID28, runs=2)


def test_fewer_units_than_blocks_and_single_row_tiles(cuda_device, capsys):
    (run,), r32, r64, keep = _case(cuda_device, (3, 33, 256), (1, 0, 1))
    _assert_anchored(run, r32, r64, keep, "conv5 backward roles (3, 33, 256), 2 valid", capsys)


def test_three_and_four_iterations_per_block(valid28, capsys):
    (first, _), r32, r64, keep = valid28
    assert int(keep.sum()) == 28
    _assert_anchored(first, r32, r64, keep, "conv5 backward roles (32, 1000, 256), 28 valid", capsys)


def test_two_runs_in_one_process_are_bit_equal(valid28):
    (first, second), _, _, _ = valid28
    A.assert_bit_equal(first, second)


@pytest.mark.parametrize("feat", [64, 128])
def test_exact_units_at_the_other_feature_widths(cuda_device, capsys, feat):
    (run,), r32, r64, keep = _case(cuda_device, (12, 64, feat))
    _assert_anchored(run, r32, r64, keep, f"conv5 backward roles (12, 64, {feat})", capsys)


def test_steady_iterations_of_the_peeled_loop(cuda_device, capsys):
    (run,), r32, r64, keep = _case(cuda_device, (40, 1000, 64))
    _assert_anchored(run, r32, r64, keep, "conv5 backward roles (40, 1000, 64), 5 units per block", capsys)


def test_valid_part_with_a_zero_feature_gradient(cuda_device, capsys):
    (run,), r32, r64, keep = _case(cuda_device, (6, 97, 256), zero_part=2)
    _assert_anchored(run, r32, r64, keep, "conv5 backward roles (6, 97, 256), part 2 without a gradient", capsys)
