"""The DGCNN encoder on csrc/dgcnn_enc.hip against its float64 restatement (tests/dgcnn_ref.py) with the kNN graphs AND
the max selections held to the HIP path's own, under the bars of tests/anchored.py.

Per case: run the HIP encoder (forward_parts, training mode, input gradient on), read back the graphs of the four stages
(mpa_dgcnn_export_graph) and the selections the forward stored for its backward (mpa_dgcnn_export_selection), evaluate
the restatement on the CPU in float32 and in float64 on those graphs with every max replaced by a gather at the HIP
path's site, and compare

  arithmetic  features, grad_x, the 17 parameter gradients and the 10 running statistics through anchored.assert_anchored:
              ceiling 1e-4, 8 x the float32 restatement's own deviation from float64 (or 8 x the median).  Nothing in a bar
              comes from the HIP path.  Rows of padded slots are exactly zero in the features and in grad_x.
  slopes      LeakyReLU is a third discrete choice: an activation within rounding of zero takes the slope 1 in one
              float32-grade evaluation and 0.2 in another; the value does not move, that row's gradient does by a factor of
              five, which is 1 / R of a whole gradient tensor — in case (d) the float32 CPU restatement itself is 1e-4
              (median) to 2e-3 away from float64 for two such sites among a million.  So the slopes the backward takes
              (mpa_dgcnn_export_branch) are pinned as well, and checked like the selections: wherever the float64
              activation is further than tol from zero the slope must be the float64 one.
  selection   a pinned comparison would accept a kernel that picks the wrong neighbour, so every selection is checked on
              the float64 values: regret = max_t z64 - z64[selected] <= tol x max|z64| of its channel, at every site of
              the four stages and of the pooling over the points, with tol = min(1e-4, 8 x 2 x d32), d32 = the float32
              restatement's largest forward deviation from float64 at that stage (8 = anchored.MULT; 2: a flip involves
              two values).  Exact ties (coinciding points) have regret 0 whichever tied slot is taken.

The cases are the smallest shapes that reach each branch of the launch plan (R = valid rows, tiles = 128-row tiles, G =
groups of the cooperative column sums, 64 table rows each):

  a    6 slots, 1 valid, N = 20, F = 64     R = 20: all but one gemm_tn chunk empty, one partial first-stage tile, k = N,
                                            every in-degree 20 (the shape where test_fused_dgcnn_edge_sizes checks no value)
  b    4 slots, all valid, N = 20, F = 128  R = 80 < 128: less than one row tile
  c    9 slots, 7 valid interleaved, N = 33, F = 256   grid.y rounded up to 16, N % 16 != 0, the 128-wide tail GEMM twice
  d    131 slots, 130 valid, N = 64, F = 128           R = 8320: 65 tiles (tail statistics and every backward coefficient
                                            G = 2), 131 slots (stage statistics G = 3): tickets, agent-scope stores and the
                                            last block's sum over the groups
  e    2 slots, N = 1024, F = 64            the largest part: four elements per thread in phase A, no padding sort keys
  f    3 slots, 2 valid, N = 1000, F = 128  the benchmark's N: a partial last pass
  g*   2 slots, N = 1024, F = 64, graphs of all four stages imported: one hub per part listed by exactly 511 / 512 / 513 /
       1024 points (the staged run of dg_agg_bwd_kernel holds 512 in-edges, the degree sort key clamps at 511), the other
       entries a ring
  h    2 slots, N = 600, F = 64, imported: every list = 0..19 — twenty points of in-degree 600, 580 of in-degree 0
  i    3 slots, N = 257, F = 128, own search: part 0 = one point 257 times, part 1 = 30 distinct points repeated, part 2
       generic: exact ties everywhere in parts 0 and 1
  eval (c) and (d) in evaluation mode: features against the float64 restatement, running statistics untouched

(a), (d) and (g1024) run twice and their outputs and gradients must be bit-equal.
"""
import copy
import math

import numpy as np
import pytest
import torch

import anchored as A
import dgcnn_ref as D

pytestmark = pytest.mark.gpu

K = D.K
TILE, GROUP = 128, 64  # kTile of csrc/dgcnn_enc.hip, kEB of csrc/coop_reduce.h


@pytest.fixture(scope="module", autouse=True)
def _at_most_16_threads():
    old = torch.get_num_threads()
    torch.set_num_threads(min(16, old))
    yield
    torch.set_num_threads(old)


class Case:
    def __init__(self, name, valid, N, F, points="random", graphs=None, expect=None, twice=False):
        self.name, self.valid, self.N, self.F = name, list(valid), N, F
        self.points, self.graphs, self.expect, self.twice = points, graphs, expect or {}, twice
        self.M, self.nv = len(valid), int(sum(valid))

    def build(self):
        """The encoder (on the CPU; about a fifth of the BatchNorm scales negative: the aggregation then selects a
        minimum of the pre-BatchNorm values), points for every slot (the padded ones hold points too: they must be
        ignored), the validity vector and the weights of the scalar loss."""
        from multi_part_assembly_amd.encoder import DGCNN
        seed = 1000 * self.M + self.N + self.F
        torch.manual_seed(seed)
        enc = DGCNN(self.F)
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for m in enc.modules():
                if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                    m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                    m.weight[::5] *= -1.0
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                    m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=g))
                    m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
        pts = torch.randn(self.M, self.N, 3, generator=g) * 0.2
        if self.points == "ties":
            pts[0] = pts[0, 0]
            pts[1] = pts[1, :30][torch.arange(self.N) % 30]
        v = torch.tensor(self.valid, dtype=torch.float32)
        w = torch.randn(self.M, self.F, generator=g)
        graphs = None
        if self.graphs is not None:
            graphs = [torch.stack([self.graphs(self.N, l, p) for p in range(self.nv)]) for l in range(4)]
            for gr in graphs:  # nothing unchecked goes to the device
                D.in_degrees(gr, self.N)
        return enc.train(), pts, v, w, graphs


def _hub(l, p, N):
    return (37 + 211 * l + 500 * p) % N


def _hub_case(listers):
    def check(deg, N):
        for l in range(4):
            for p in range(deg[l].shape[0]):
                h = _hub(l, p, N)
                assert deg[l][p, h] == listers and np.delete(deg[l][p], h).max() <= 21, (l, p)
    return Case(f"g{listers}", [1, 1], 1024, 64, graphs=lambda N, l, p: D.hub_ring_graph(N, _hub(l, p, N), listers),
                expect={"rows": 2048, "tiles": 16, "degrees": check}, twice=listers == 1024)


def _all_twenty(deg, N):
    for d in deg:
        assert (d == K).all()


def _twenty_hubs(parts):
    def check(deg, N):
        for d in deg:
            for p in parts:
                assert (d[p, :K] == N).all() and (d[p, K:] == 0).all()
    return check


CASES = [
    Case("a", [0, 0, 1, 0, 0, 0], 20, 64, expect={"rows": 20, "tiles": 1, "degrees": _all_twenty}, twice=True),
    Case("b", [1, 1, 1, 1], 20, 128, expect={"rows": 80, "tiles": 1, "degrees": _all_twenty}),
    Case("c", [1, 0, 1, 1, 0, 1, 1, 1, 1], 33, 256, expect={"rows": 231, "tiles": 2}),
    Case("d", [1] * 77 + [0] + [1] * 53, 64, 128, expect={"rows": 8320, "tiles": 65, "tile_groups": 2, "slot_groups": 3},
         twice=True),
    Case("e", [1, 1], 1024, 64, expect={"rows": 2048, "tiles": 16}),
    Case("f", [1, 0, 1], 1000, 128, expect={"rows": 2000, "tiles": 16}),
    _hub_case(511), _hub_case(512), _hub_case(513), _hub_case(1024),
    Case("h", [1, 1], 600, 64, graphs=lambda N, l, p: D.constant_graph(N),
         expect={"rows": 1200, "tiles": 10, "degrees": _twenty_hubs((0, 1))}),
    Case("i", [1, 1, 1], 257, 128, points="ties", expect={"rows": 771, "tiles": 7, "degrees": _twenty_hubs((0,))}),
]
BY_NAME = {c.name: c for c in CASES}


def _hip(case, built, dev, training=True):
    """One forward (and backward) of the HIP encoder on a fresh copy of the case's module.  Returns the compared tensors
    under the keys of anchored.oracle_run, the exported graphs [nv, N, 20] and selections, and the module."""
    enc0, pts, v, w, graphs = built
    enc = copy.deepcopy(enc0).to(dev).train(training)
    nv, N, M = case.nv, case.N, case.M
    hooks = {"export": True, "export_selection": True}
    if graphs is not None:
        hooks["graphs"] = [g.reshape(nv * N, K).int() for g in graphs]
    enc.graph_hooks = hooks
    x = pts.to(dev).requires_grad_(training)
    with torch.enable_grad() if training else torch.no_grad():
        out = enc.forward_parts(x, v.to(dev))
        exported = [t.cpu() for t in hooks["exported"]]
        selection = [t.cpu() for t in hooks["selection"]]
        slopes = [t.cpu() for t in hooks["branch"]]
        if training:
            (out * w.to(dev)).sum().backward()
    torch.cuda.synchronize()
    for l in range(4):  # rows past the valid parts are marked, the valid ones come first
        assert exported[l].shape == (M * N, K) and selection[l].shape == (M * N, D.WIDTHS[l])
        assert (exported[l][nv * N:] == -1).all() and (selection[l][nv * N:] == -1).all()
        assert slopes[l].shape == selection[l].shape and (slopes[l][nv * N:] == -1).all()
    assert selection[4].shape == (M, case.F) and (selection[4][nv:] == -1).all()
    assert slopes[4].shape == (M * N, case.F) and (slopes[4][nv * N:] == -1).all()
    gr = [t[:nv * N].view(nv, N, K).long() for t in exported]
    sel = [t[:nv * N].view(nv, N, -1).long() for t in selection[:4]] + [selection[4][:nv].long()]
    sel.append([t[:nv * N].view(nv, N, -1) for t in slopes])  # sel[5]: the LeakyReLU slopes of the backward
    for l in range(4):
        assert int(sel[l].min()) >= 0 and int(sel[l].max()) < K
    assert all(int(t.min()) >= 0 and int(t.max()) <= 1 for t in sel[5])
    assert int(sel[4].min()) >= 0 and int(sel[4].max()) < N
    keep = v > 0
    feat = out.detach().cpu()
    assert float(feat[~keep].abs().max() if (~keep).any() else 0.0) == 0.0  # rows of padded slots are exactly zero
    res = {"out.feat": feat[keep]}
    if training:
        gx = x.grad.detach().cpu()
        assert float(gx[~keep].abs().max() if (~keep).any() else 0.0) == 0.0
        res["gin.pts"] = gx[keep]
        res.update({"grad." + k: p.grad.detach().cpu() for k, p in enc.named_parameters()})
        res.update({"out.stat." + k: t.detach().cpu() for k, t in enc.state_dict().items()
                    if "running_" in k and k.startswith("bn")})
    return res, gr, sel, enc


def _restatement(built, graphs, sel, dtype, training=True):
    """tests/dgcnn_ref.py on the valid parts in `dtype` (cast from the float32 values), pinned at `sel`: the tensors under
    the keys of anchored.oracle_run (float64 copies) and the post-activation values of the five maxima."""
    enc0, pts, v, w, _ = built
    keep = v > 0
    cast = lambda t: (t.detach().to(dtype) if t.is_floating_point() else t.detach()).clone()
    sd = {k: cast(t) for k, t in enc0.state_dict().items()}
    params = {k: t.requires_grad_(training) for k, t in sd.items() if t.is_floating_point() and "running_" not in k}
    x, stats = cast(pts[keep]).requires_grad_(training), {}
    with torch.enable_grad() if training else torch.no_grad():
        feat, z = D.dgcnn_ref(x, sd, graphs, sel[:5], training, stats, branch=sel[5])
        if training:
            (feat * cast(w[keep])).sum().backward()
    r = {"out.feat": feat.detach().double()}
    if training:
        r["gin.pts"] = x.grad.double()
        r.update({"grad." + k: p.grad.double() for k, p in params.items() if p.grad is not None})
        r.update({"out.stat." + k: t.double() for k, t in stats.items()})
    return r, [t.detach() for t in z]


def _check_inputs(case, graphs):
    """What the case is built for is present, counted on the graphs that were read back."""
    e = case.expect
    assert case.nv * case.N == e["rows"] and math.ceil(e["rows"] / TILE) == e["tiles"]
    if "tile_groups" in e:
        assert math.ceil(e["tiles"] / GROUP) == e["tile_groups"] and math.ceil(case.M / GROUP) == e["slot_groups"]
    deg = [D.in_degrees(g, case.N) for g in graphs]  # (asserts 20 distinct indices below N in every list)
    if "degrees" in e:
        e["degrees"](deg, case.N)
    return max(int(d.max()) for d in deg)


def _check_selection(z32, z64, sel, label, capsys):
    reg = D.selection_regret(z64, sel[:5])
    lines, bad = [], []
    # the slope: wherever the float64 activation is clear of zero by tol x its channel's max|z64|, the backward's slope is
    # the float64 one (nearer to zero either slope is a legitimate float32-grade choice; it is pinned, and counted here)
    own = D.own_branch(z64, sel[:5])
    for l, (regret, scale, differ) in enumerate(reg):
        top = float(z64[l].abs().max())
        d32 = float((z32[l].double() - z64[l]).abs().max()) / top
        tol = min(A.CEIL, A.MULT * 2.0 * d32)
        worst = float((regret / scale.clamp_min(1e-300)).max())
        lines.append(f"{'stage %d' % (l + 1) if l < 4 else 'pool'}: tol {tol:.1e}, {differ} of {sel[l].numel()} sites off "
                     f"the float64 arg-max, worst regret {worst:.1e}")
        a64 = z64[l].gather(2, sel[l].unsqueeze(2)).squeeze(2) if l < 4 else z64[l]
        off = own[l] != sel[5][l].bool()
        # (a negative activation is 0.2 x its pre-activation: the distance from the kink is |a| on either side of it,
        # up to that factor, which the test gives away)
        lines[-1] += f", {int(off.sum())} slopes off the float64 sign"
        if not bool((regret <= tol * scale).all()) or bool((off & (a64.abs() > tol * scale)).any()):
            bad.append(lines[-1])
    with capsys.disabled():
        print(f"\n  {label} selections: " + "; ".join(lines), end="")
    assert not bad, f"{label}: a selection is not a maximum (or a slope not the sign) of the float64 values: " + "; ".join(bad)


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_dgcnn_against_the_pinned_float64_restatement(cuda_device, capsys, name):
    case = BY_NAME[name]
    built = case.build()
    got, graphs, sel, _ = _hip(case, built, cuda_device)
    top_degree = _check_inputs(case, graphs)
    if built[4] is not None:
        for a, b in zip(graphs, built[4]):
            assert torch.equal(a, b)  # an imported graph is what the forward used
    if case.points == "ties":  # part 0 is one point N times: every candidate ties, and ties go to the FIRST (the kernels' rule)
        assert all(int(sel[l][0].max()) == 0 for l in range(5)), [int(sel[l][0].max()) for l in range(5)]
    if case.twice:
        again, graphs2, sel2, _ = _hip(case, built, cuda_device)
        A.assert_bit_equal(got, again)
        assert all(torch.equal(a, b) for a, b in zip(graphs + sel[:5] + sel[5], graphs2 + sel2[:5] + sel2[5]))
    r32, z32 = _restatement(built, graphs, sel, torch.float32)
    r64, z64 = _restatement(built, graphs, sel, torch.float64)
    assert set(got) == set(r64) and len(got) == 1 + 1 + 17 + 10, sorted(set(got) ^ set(r64))
    label = f"DGCNN {name}: {case.M} slots, {case.nv} valid, N {case.N}, F {case.F}, largest in-degree {top_degree}"
    _check_selection(z32, z64, sel, label, capsys)
    A.assert_anchored(got, r32, r64, label, capsys)


@pytest.mark.parametrize("name", ["c", "d"])
def test_dgcnn_evaluation_mode_against_the_float64_restatement(cuda_device, capsys, name):
    case = BY_NAME[name]
    built = case.build()
    sd0 = {k: t.detach().clone() for k, t in built[0].state_dict().items()}
    got, graphs, sel, enc = _hip(case, built, cuda_device, training=False)
    _check_inputs(case, graphs)
    for k, t in enc.state_dict().items():  # evaluation mode touches no statistic and no counter
        assert torch.equal(t.cpu(), sd0[k]), k
    r32, z32 = _restatement(built, graphs, sel, torch.float32, training=False)
    r64, z64 = _restatement(built, graphs, sel, torch.float64, training=False)
    label = f"DGCNN {name}, evaluation mode"
    _check_selection(z32, z64, sel, label, capsys)
    A.assert_anchored(got, r32, r64, label, capsys)
