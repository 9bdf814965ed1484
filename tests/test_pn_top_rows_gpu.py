"""PointNet's last-layer backward pass reads the sparse arg-max term S W5 from a table of finished rows
(csrc/pointnet.hip: pn_top_csr_kernel builds `rtile` / `rsum`, csrc/pn_bwd_q.h: the stagers of pn_bwd_top_q_kernel read
them).  Inputs that stress that table, through the public entry point (`PointNet.forward_parts`), against the float64
oracle (oracle/nets.py: pointnet) on the valid parts, and bit for bit between two runs.

How the arg-maxima are steered: rows that are exact copies of one point give exactly equal features, and among equal
values the lowest row index is the arg-max.  A part whose rows are all copies of ONE point has all F arg-maxima on row 0;
a part whose rows 1 .. N-2 copy row 0 has them on row 0 or on row N-1; a part whose rows >= 32 copy rows 0 .. 31 has them
on the 32 rows of its first tile.  Copies have equal activations, so the parameter gradients do not depend on which of
them a tie goes to: the oracle needs no tie rule.  Ordinary random parts share every batch (healthy BatchNorm statistics).

Features and every parameter gradient are held to the float64-anchored bar of tests/anchored.py: per tensor, 8 x the float32
CPU oracle's own deviation from float64 on the same inputs (or 8 x the median of those deviations), never above 1e-4."""
import ctypes

import pytest
import torch

import anchored as A
from multi_part_assembly_amd import _lib
from multi_part_assembly_amd.encoder import build_encoder

gpu = pytest.mark.gpu


def _one_row(n, g):
    """Every row the same point: all arg-maxima on row 0, one distinct row with F entries."""
    return (torch.randn(1, 3, generator=g) * 0.3).expand(n, 3).clone()


def _first_and_last(n, g):
    """Rows 0 .. n-2 one point, row n-1 another: arg-maxima on the first and on the last valid row only."""
    p = _one_row(n, g)
    p[n - 1] = torch.randn(3, generator=g) * 0.3
    return p


def _full_tile(n, g):
    """32 different points in rows 0 .. 31, every later row a copy of one of them: arg-maxima on the 32 rows of tile 0."""
    base = torch.randn(32, 3, generator=g) * 0.3
    return base[torch.arange(n) % 32].clone()


def _random(n, g):
    return torch.randn(n, 3, generator=g) * 0.2


def _batch(kinds, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([k(n, g) for k in kinds])


def _run(enc, pts, valids, w):
    enc.zero_grad()
    out = enc.forward_parts(pts, valids)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    return out.detach().clone(), {k: p.grad.detach().clone() for k, p in enc.named_parameters()}


def _check(cuda_device, capsys, feat, pts, valids, seed=0):
    torch.manual_seed(seed)
    enc = build_encoder("pointnet", feat).to(cuda_device).train()
    with torch.no_grad():  # both signs of the last BatchNorm's weight: maxima and minima of the never-stored Y5
        enc.bn5.weight[::3] *= -1.0
    sd = {k: v.detach().cpu().clone() for k, v in enc.state_dict().items()}
    M = pts.shape[0]
    w = torch.randn(M, feat, generator=torch.Generator().manual_seed(seed + 1))
    out, grads = _run(enc, pts.to(cuda_device), valids.to(cuda_device), w.to(cuda_device))
    out2, grads2 = _run(enc, pts.to(cuda_device), valids.to(cuda_device), w.to(cuda_device))
    assert torch.equal(out, out2)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), f"{k}: two runs differ"
    keep = valids > 0
    assert float(out[~keep.to(cuda_device)].abs().max() if (~keep).any() else 0.0) == 0.0
    if not keep.any():
        for k, gk in grads.items():
            assert bool(torch.isfinite(gk).all()) and float(gk.abs().max()) == 0.0, k
        return
    r32, r64 = A.oracle_pair(A.pointnet_fn(True), sd, {"pts": pts[keep], "w": w[keep]})
    got = {"out.feat": out.cpu()[keep], **{"grad." + k: gk.cpu() for k, gk in grads.items()}}
    A.assert_anchored(got, {k: r32[k] for k in got}, {k: r64[k] for k in got},
                      f"PointNet arg-max rows, F={feat}, {tuple(pts.shape)}, {int(keep.sum())} valid", capsys)


@gpu
@pytest.mark.parametrize("feat", [256, 128, 64])
@pytest.mark.parametrize("N", [1000, 37])
def test_all_arg_maxima_on_one_row(cuda_device, capsys, feat, N):
    kinds = [_one_row, _random, _one_row, _random, _random, _one_row]
    _check(cuda_device, capsys, feat, _batch(kinds, N, 11), torch.ones(len(kinds)))


@gpu
@pytest.mark.parametrize("feat", [256, 128, 64])
@pytest.mark.parametrize("N", [1000, 37])
def test_arg_maxima_on_first_and_last_valid_row(cuda_device, capsys, feat, N):
    kinds = [_first_and_last, _random, _first_and_last, _random, _first_and_last]
    _check(cuda_device, capsys, feat, _batch(kinds, N, 12), torch.ones(len(kinds)))


@gpu
@pytest.mark.parametrize("feat", [256, 128, 64])
@pytest.mark.parametrize("N", [1000, 37])
def test_arg_maxima_on_the_32_rows_of_one_tile(cuda_device, capsys, feat, N):
    kinds = [_full_tile, _random, _full_tile, _full_tile, _random]
    _check(cuda_device, capsys, feat, _batch(kinds, N, 13), torch.ones(len(kinds)))


@gpu
@pytest.mark.parametrize("feat", [256, 64])
def test_padded_parts_between_valid_ones(cuda_device, capsys, feat):
    kinds = [_random, _one_row, _random, _full_tile, _first_and_last, _random, _random, _one_row]
    valids = torch.tensor([0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 0.0])
    _check(cuda_device, capsys, feat, _batch(kinds, 1000, 14), valids)


@gpu
@pytest.mark.parametrize("N", [1000, 37])
def test_batch_without_a_valid_part(cuda_device, capsys, N):
    kinds = [_random, _one_row, _full_tile]
    _check(cuda_device, capsys, 256, _batch(kinds, N, 15), torch.zeros(len(kinds)))


# sizes of the workspace before the row table existed (float elements, int elements), recorded from that build
_BEFORE = {(640, 1000, 256): (348294676, 3134724), (12, 1000, 128): (21267988, 29596), (7, 37, 64): (15230228, 2276),
           (3, 32768, 256): (65578004, 17676)}


@pytest.mark.parametrize("shape", sorted(_BEFORE))
def test_workspace_grows_by_the_row_table(shape):
    """Appended behind the earlier fields, each rounded up to 16 bytes: rsum [M][F][128] floats, rtile [M][T + 1] int2.
    The fields they made dead have since been retired from the layout: eval [M][F] floats, and erow [M][F], ech [M][F],
    tptr [M][T + 1] ints."""
    M, N, F = shape
    nf, ni = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.lib().mpa_pointnet_workspace(M, N, F, ctypes.byref(nf), ctypes.byref(ni)), "mpa_pointnet_workspace")
    pad = lambda n: (n + 3) // 4 * 4
    T = (N + 31) // 32
    assert nf.value - _BEFORE[shape][0] == pad(M * F * 128) - pad(M * F)
    assert ni.value - _BEFORE[shape][1] == pad(2 * M * (T + 1)) - 2 * pad(M * F) - pad(M * (T + 1))
    assert nf.value % 4 == 0 and ni.value % 4 == 0 and _BEFORE[shape][0] % 4 == 0 and _BEFORE[shape][1] % 4 == 0
