"""PointNet on csrc/pointnet.hip (6-product split-bf16 GEMMs in wave-specialised persistent kernels, csrc/pn_fwd_ws.h; the
backward in its Q form with prebuilt arg-max row sums, csrc/pn_bwd_q.h) against oracle.nets.pointnet evaluated in FLOAT64
on the valid parts, under the bars of tests/anchored.py: features, every conv / bn gradient, the running statistics after
the training forward, an eval-mode forward; two back-to-back runs bit-equal.  bn5.weight has negative and zero entries and
bn4.weight negative ones in every case.

The shapes are the smallest that reach each structural edge of the launch plan (mpa_pointnet_forward / _backward).  The
persistent kernels of layers 2-4 (pn_fwd_ws_kernel, pn_bwd_q_kernel) and the top layer's backward (pn_bwd_top_q_kernel)
walk RB-row units u = block, block + grid, ...; a unit is (valid part u / TB, row tile u % TB) with TB = ceil(N / RB), so
units never span parts and the last unit of every part is ragged unless RB divides N.  The top layer's FORWARD
(pn_fwd_ws_top_kernel, whose output is never stored) walks groups (valid part, row split) instead, all 32-row tiles of a
group back to back with the group's running top-2 records in registers; the number of splits is 1 below 481 points, 2 up
to 992, 8 above, so its 256 blocks take a second group only with more than 256 / splits valid parts.

  (33, 1, 64)    one point per part, 33 BatchNorm positions
  (5, 31, 128)   less than one 32-row tile per part
  (1, 33, 64)    one part, a one-row ragged second tile
  (6, 64, 256)   exactly one 64-row unit per part
  (7, 65, 64)    valids 1,0,1,1,0,0,1: one row past a unit, padding between valid parts (the `vlist` of valid parts)
  (3, 97, 128)   ragged 32-row and 64-row tails together
  (40, 224, 256) 280 32-row units, 160 64-row units: the 256 blocks of the top layer's backward and of layer 4's backward take
                 a second unit; those of layers 2 and 3 (64-row units), the 512 of layer 4's forward and the top layer's
                 forward (40 groups) do not
  (40, 460, 64)  36 valid parts, 4 padded ones interleaved: 288 64-row units (the 256 blocks of layers 2 and 3 take a second
                 unit) and 540 32-row units (so do the 512 blocks of layer 4's forward); 36 groups in the top layer's forward
  (260, 33, 64)  260 groups of two tiles in the top layer's forward: blocks 0-3 finish one group's records, write them and
                 start a second group; 520 32-row units (every 256-block kernel wraps twice, layer 4's forward once)
  (3, 513, 128)  17 tiles per part in two row splits of 9: the second split's records start at tile 9, its eighth tile has
                 one row and its ninth lies past the part's end (an empty tile)
"""
import pytest
import torch

import anchored as A

pytestmark = pytest.mark.gpu

IDS = ["%dx%dx%d" % c[0] for c in A.POINTNET_CASES]


def _run(enc, pts, v, w):
    enc.zero_grad()
    out = enc.forward_parts(pts, v)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    res = {"out.feat": out.detach().clone()}
    res.update({"grad." + k: p.grad.detach().clone() for k, p in enc.named_parameters()})
    return res


@pytest.mark.parametrize("case", A.POINTNET_CASES, ids=IDS)
def test_pointnet_against_the_float64_oracle(cuda_device, capsys, case):
    shape, valids = case
    enc, pts, v, w = A.pointnet_case(shape, valids)
    sd0 = {k: t.detach().clone() for k, t in enc.state_dict().items()}
    keep = v > 0
    r32, r64 = A.oracle_pair(A.pointnet_fn(True), sd0, {"pts": pts[keep], "w": w[keep]})

    enc.to(cuda_device).train()
    dpts, dv, dw = pts.to(cuda_device), v.to(cuda_device), w.to(cuda_device)
    first = _run(enc, dpts, dv, dw)
    stats = {"out.stat." + k: t.detach().clone() for k, t in enc.state_dict().items() if "running_" in k}
    enc.load_state_dict(sd0)  # the same running statistics in front of the second run
    second = _run(enc, dpts, dv, dw)
    A.assert_bit_equal(first, second)
    for k, t in enc.state_dict().items():
        if "running_" in k:
            assert torch.equal(t, stats["out.stat." + k]), k
        elif "num_batches_tracked" in k:
            assert int(t) == int(sd0[k]) + 1, k

    feat = first.pop("out.feat").cpu()
    assert float(feat[~keep].abs().max() if (~keep).any() else 0.0) == 0.0  # rows of padded parts are zero
    got = {"out.feat": feat[keep], **first, **stats}
    assert set(got) == set(r64), sorted(set(got) ^ set(r64))
    A.assert_anchored(got, r32, r64, f"PointNet {shape}, {int(keep.sum())} valid parts, training", capsys)

    e32, e64 = ({"out.feat": r["out.feat"]} for r in A.oracle_pair(A.pointnet_fn(False), sd0, {"pts": pts[keep], "w": w[keep]}))
    enc.load_state_dict(sd0)
    enc.eval()
    with torch.no_grad():
        ev = enc.forward_parts(dpts, dv).cpu()
    assert all(torch.equal(t.cpu(), sd0[k]) for k, t in enc.state_dict().items())  # eval mode touches no statistic
    A.assert_anchored({"out.feat": ev[keep]}, e32, e64, f"PointNet {shape}, eval mode", capsys)
