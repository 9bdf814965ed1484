"""Randomised differential checks of the index-exact kernels, for a time budget on the GPU box (dev tool; the fixed cases
live in tests/).  Every case draws its own sizes, masks and pose regime from the seed:

  loss   grid-pruned whole-shape search vs the brute-force scan of the same library (MPA_SHAPE_SEARCH): arg-mins of both
         directions bit-equal on the valid parts, the five loss terms within 2e-6;
  lossgrad  forward + backward of the fused loss through the C ABI under a random search route (both rotation forms, training
         and eval normalisation, non-prefix masks, a sample without a valid part, predictions 0.1 / 0.25 from the ground truth) vs tests/assembly_loss_ref.py
         in float64 with the nearest-neighbour selections pinned to the kernel's own: the five terms and the pose gradients
         of every sample under the bars of tests/anchored.py (8 x the float32 reference's own deviation, at most 1e-4);
  chamfer  the Chamfer operator (three scan variants) vs oracle/chamfer_ref.c: distances and indices bit-equal;
  cgrid  the operator's grid-pruned search (variant 3: outlier-trimmed grid, unbounded border cells, run dedupe, hand-back
         of non-finite samples) vs its exhaustive scan on clouds built to break it — blobs at different scales and offsets,
         planes and lines, far outliers, runs of repeated points, 1e3-filled padded parts, NaN / inf / huge coordinates,
         1 to 6000 points per cloud: all four outputs bit-equal (small cases also against oracle/chamfer_ref.c);
  cgate  the operator's matrix-core gated search (variant 4, csrc/gate_nn.hip) vs the exhaustive scan on the same clouds,
         1 to 3000 points (several LDS panels), coincident clouds, one-distinct-target clouds: all four outputs bit-equal;
  knn    mpa_knn_exact (C = 3, 64, 128) vs oracle/knn_ref.c: every neighbour index, in order;
  knn3g  C = 3: the gated search (csrc/dg_knn3_gate.h) vs the exhaustive knn3_kernel on those clouds, index for index;
  glue   the graph-network glue kernels vs float64 library ops;
  nets   PointNet (random part counts, masks, point counts, negative / zero BatchNorm weights) and transformer + pose head
         (random widths, depths, masks, odd head widths) vs oracle/nets.py evaluated in float64: features and every
         gradient within 2e-4, or no further from float64 than twice the float32 oracle is;
  dgcnn  the one-call DGCNN encoder (random part counts, 20-400 points, widths 64 / 128 / 256, negative BatchNorm weights) vs
         the reference's edge-tensor formulation in float64 on the graphs the encoder itself built (read back): features,
         input and parameter gradients, same bounds and conditioning check as `nets`;
  step   a whole training step (forward, five-term loss, backward) of PNTransformer + PointNet — random batch sizes, part
         counts, point counts, widths, depths — vs oracle/nets.py (pn_transformer_loss) in float64: loss and every
         parameter gradient, same bounds and conditioning check;
  gnn    the same for DGL (three GNN iterations) on either encoder vs oracle/callers.py (dgl_loss);
  global the same for B-Global on semantic batches (identical-part matching, min-of-N sampling, noise channels) vs
         oracle/callers.py (global_loss), every evaluation re-seeded so that all three see the same noise;
  adam   the fused optimiser vs torch.optim.Adam / AdamW (+ clip_grad_norm_) over 1-7 steps on random tensor sets;
  graph  four training steps replayed as a HIP graph vs eager launches (PNTransformer or DGL, dropout on): losses and the
         final parameters bit-equal;
  repro  bit-reproducibility: forward + backward of every module of the path (both encoders, transformer, pose head, MLP layer,
         GRU recurrence, fused loss) run twice on the same inputs — outputs and every gradient bit-equal.

usage: python tools/fuzz_parity.py [seconds=240] [first_seed=0] [families, e.g. glue,knn]
       -> one summary line per family, exit 1 on a mismatch
"""
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multi_part_assembly_amd import _lib, chamfer as C, synthetic  # noqa: E402
from multi_part_assembly_amd.encoder import knn_exact  # noqa: E402
from multi_part_assembly_amd.gnn_ops import narrow_linear_relu, pair_rows, relation_head, relation_mean  # noqa: E402
from multi_part_assembly_amd.rotation import Rotation3D  # noqa: E402
from oracle import chamfer as oc  # noqa: E402
from oracle.knn import knn_exact as oracle_knn  # noqa: E402

dev = torch.device("cuda:0")
bad = []
edge = []  # cases at which the float64 oracle itself is discontinuous (a 2e-6 .. 2e-5 relative input change moves its gradients by > 1e-3)


def raw_loss(batch, qp, tp, mode, all_four=False, part="gate"):
    os.environ["MPA_SHAPE_SEARCH"] = mode
    os.environ["MPA_PART_SEARCH"] = part  # the per-part term: matrix-core gated search (default) | the scan / leaves of `mode`
    pcs, v = batch["part_pcs"], batch["part_valids"]
    qg, tg = Rotation3D(batch["part_quat"]).rot.contiguous(), batch["part_trans"].contiguous()
    B, P, N, _ = pcs.shape
    L = _lib.lib()
    nf, ni = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(L.mpa_assembly_loss_workspace(B, P, N, ctypes.byref(nf), ctypes.byref(ni)), "ws")
    fws = torch.full((nf.value,), float("nan"), device=dev)
    iws = torch.full((ni.value,), 0x7F7F7F7F, dtype=torch.int32, device=dev)
    losses = torch.empty(5, B, device=dev)
    _lib.check(L.mpa_assembly_loss_forward(_lib.ptr(pcs), _lib.ptr(v), _lib.ptr(qp), _lib.ptr(tp), _lib.ptr(qg), _lib.ptr(tg),
                                           B, P, N, 1, 0, _lib.ptr(fws), _lib.ptr(iws), _lib.ptr(losses),
                                           _lib.current_stream(dev)), "fwd")
    torch.cuda.synchronize()
    pn = B * P * N
    if all_four:  # per-part arg-mins (both directions) too
        return losses, [iws[k * pn:(k + 1) * pn].view(B, P, N).clone() for k in range(4)]
    return losses, iws[2 * pn:3 * pn].view(B, P, N).clone(), iws[3 * pn:4 * pn].view(B, P, N).clone()


def case_loss(rng):
    B = int(rng.choice([1, 2, 3, 4, 5, 7, 8, 9, 13, 16, 33]))
    P = int(rng.integers(1, 21))
    N = int(rng.choice([1, 16, 33, 64, 100, 255, 256, 500, 777, 1000, 1200, 2048, 2100]))  # (> 2048: leaf -> grid fallback)
    counts = [int(rng.integers(1, P + 1)) for _ in range(B)]
    batch = synthetic.make_batch(B, P, N, seed=int(rng.integers(1 << 30)), device=dev, num_parts=counts,
                                 preset=str(rng.choice(["everyday", "artifact"])))
    if rng.random() < 0.3:  # valid flags that are not a prefix
        v = batch["part_valids"]
        for b in range(B):
            perm = torch.randperm(P, generator=torch.Generator().manual_seed(int(rng.integers(1 << 30))))
            v[b] = v[b][perm.to(v.device)]
        if rng.random() < 0.3:
            v[int(rng.integers(B))] = 0  # a sample with no valid part
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    spread = float(rng.choice([0.0, 0.02, 0.3, 1.0, 30.0]))
    qp = torch.nn.functional.normalize(torch.randn(B, P, 4, generator=g), dim=-1).to(dev)
    tp = (torch.randn(B, P, 3, generator=g) * spread).to(dev)
    if rng.random() < 0.15:  # duplicated points: exact ties
        batch["part_pcs"][:, :, 1::2] = batch["part_pcs"][:, :, 0::2][:, :, : batch["part_pcs"][:, :, 1::2].shape[2]]
    regime = "random"
    if rng.random() < 0.35:  # predictions close to (or exactly at) the ground truth: the twin-point seed / the matrix-core
        eps = float(rng.choice([0.0, 1e-6, 1e-3, 0.02]))  # gate of the leaf search at near-coincident clouds
        qg = Rotation3D(batch["part_quat"]).rot
        qp = torch.nn.functional.normalize(qg + eps * torch.randn(B, P, 4, generator=g).to(dev), dim=-1).contiguous()
        tp = (batch["part_trans"] + eps * torch.randn(B, P, 3, generator=g).to(dev)).contiguous()
        regime = f"near-gt eps={eps}"
    lb, ib = raw_loss(batch, qp, tp, "brute", all_four=True, part="scan")
    valid = batch["part_valids"].bool()
    fin = torch.isfinite(lb)
    ok = True
    # the grid of rounds 1-4, the k-d leaves (round 5), the per-sample route; the per-part term on the gated search
    # (gate_nn.hip) and, for the leaves, on the leaf search as well
    for mode, part in (("brute", "gate"), ("grid", "gate"), ("leaf", "gate"), ("leaf", "scan"), ("auto", "gate")):
        lm, im = raw_loss(batch, qp, tp, mode, all_four=True, part=part)
        ok = ok and all(torch.equal(ib[k][valid], im[k][valid]) for k in range(4))
        ok = ok and bool(torch.equal(fin, torch.isfinite(lm)))
        ok = ok and bool(((lm[fin] - lb[fin]).abs() <= 2e-6 * lb[fin].abs() + 1e-9).all())
    return ok, f"B={B} P={P} N={N} spread={spread} {regime}"


def case_lossgrad(rng):
    """Drawn as `case_loss` draws (without duplicated points and non-finite poses; near-GT distances: below), B P N capped at 200 000 so that the float64
    autograd on the host stays short.  The arg-mins are not re-checked here: the `loss` family proves them."""
    tests = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests")
    if tests not in sys.path:
        sys.path.insert(0, tests)
    import anchored as A
    import assembly_loss_hip as H
    import assembly_loss_ref as R

    B = int(rng.choice([1, 2, 3, 4, 5, 7, 8, 9, 13, 16, 33]))
    P = int(rng.integers(1, 21))
    N = int(rng.choice([1, 16, 33, 64, 100, 255, 256, 500, 777, 1000, 1200, 2048, 2100]))
    B = max(1, min(B, 200000 // (P * N)))
    counts = [int(rng.integers(1, P + 1)) for _ in range(B)]
    sb = synthetic.make_batch(B, P, N, seed=int(rng.integers(1 << 30)), device=dev, num_parts=counts,
                              preset=str(rng.choice(["everyday", "artifact"])))
    v = sb["part_valids"]
    if rng.random() < 0.3:  # valid flags that are not a prefix
        for b in range(B):
            perm = torch.randperm(P, generator=torch.Generator().manual_seed(int(rng.integers(1 << 30))))
            v[b] = v[b][perm.to(v.device)]
            for k in ("part_pcs", "part_quat", "part_trans"):  # (the parts move with their flags)
                sb[k][b] = sb[k][b][perm.to(v.device)]
        if B > 1 and rng.random() < 0.3:
            v[int(rng.integers(B))] = 0  # a sample with no valid part
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    spread = float(rng.choice([0.0, 0.02, 0.3, 1.0, 30.0]))
    qg = Rotation3D(sb["part_quat"]).rot.cpu()
    qp = torch.nn.functional.normalize(torch.randn(B, P, 4, generator=g), dim=-1)
    tp = torch.randn(B, P, 3, generator=g) * spread
    regime = "random"
    if rng.random() < 0.35:
        # predictions near the ground truth, at the distances where a gradient still has a float32-grade value.  What the
        # terms are made of cancels there: 1 - |dot| ~ 1.5 eps^2 against the 4 x 2^-24 rounding of a float32 dot product,
        # posed-cloud differences ~ 0.3 eps against the 2e-8 rounding of their operands.  At eps = 0.1 that is 2e-5 and 1e-6
        # relative, inside the 1e-4 ceiling; at the eps = 0 / 1e-6 / 1e-3 / 0.02 of `case_loss` the float32 CPU reference is
        # itself 1e-4 .. 1.4 away from float64 (measured, LABBOOK 2026-10-20) and no float32 code can meet the ceiling, so
        # those draws stay with the `loss` and `repro` families, which check what is exact there (arg-mins, bits).
        eps = float(rng.choice([0.1, 0.25]))
        qp = torch.nn.functional.normalize(qg + eps * torch.randn(B, P, 4, generator=g), dim=-1)
        tp = sb["part_trans"].cpu() + eps * torch.randn(B, P, 3, generator=g)
        regime = f"near-gt eps={eps}"
    rot_type = str(rng.choice(["quat", "rmat"]))
    training = bool(rng.random() < 0.6)
    route = str(rng.choice(["brute", "grid", "leaf", "auto"]))
    to_rot = (lambda q: R.quat_to_rmat(q.double()).float()) if rot_type == "rmat" else (lambda q: q)
    batch = {"pcs": sb["part_pcs"].cpu(), "valids": v.cpu(), "rot_pred": to_rot(qp).contiguous(), "trans_pred": tp.contiguous(),
             "rot_gt": to_rot(qg).contiguous(), "trans_gt": sb["part_trans"].cpu()}
    go = torch.rand(5, B, generator=g) + 0.5
    os.environ.pop("MPA_PART_SEARCH", None)
    hip = H.hip_run(batch, go, rot_type, training, route, dev)
    what = f"B={B} P={P} N={N} {rot_type} training={training} {route} spread={spread} {regime}"
    live = [b for b in range(B) if bool((batch["valids"][b] > 0).any())]
    ok = bool(torch.isfinite(hip["grad_rot"]).all()) and bool(torch.isfinite(hip["grad_trans"]).all())
    for b in range(B):  # a sample without a valid part: exactly no gradient (include/mpa_hip.h)
        if b not in live:
            ok = ok and bool((hip["grad_rot"][b] == 0).all()) and bool((hip["grad_trans"][b] == 0).all())
    samples = None if len(live) == B else live
    pick = (lambda t: t) if samples is None else (lambda t: t[samples])
    r64 = R.tensors(*R.run(batch, hip["idx"], go, rot_type, training, torch.float64, samples=samples), samples=samples)
    r32 = R.tensors(*R.run(batch, hip["idx"], go, rot_type, training, torch.float32, samples=samples), samples=samples)
    got = R.tensors(hip["losses"] if samples is None else hip["losses"][:, samples], pick(hip["grad_rot"]),
                    pick(hip["grad_trans"]), samples=samples)
    # every tensor, CEIL and MULT as they stand.  (Known, and left to be reported: with B = 1 a loss term is one float32
    # scalar; where the float32 reference lands within 0.1 ulp of float64 on most tensors the bar falls below float32's half
    # ulp and a value one ulp off misses it -- 2 of 404 seeds, LABBOOK 2026-10-20.)
    rows, failed = A.check(got, r32, r64)
    if failed:
        what += " " + "; ".join(failed[:4])
    return ok and not failed, what


def case_chamfer(rng):
    B = int(rng.integers(1, 6))
    n1, n2 = int(rng.integers(1, 1500)), int(rng.integers(1, 1500))
    a = rng.standard_normal((B, n1, 3)).astype(np.float32) * float(rng.choice([1e-3, 1.0, 100.0]))
    b = rng.standard_normal((B, n2, 3)).astype(np.float32) * float(rng.choice([1e-3, 1.0, 100.0]))
    if rng.random() < 0.3:
        b[:, : min(n1, n2)] = a[:, : min(n1, n2)]  # zero distances and ties
    if rng.random() < 0.2:
        a = np.round(a * 4) / 4  # lattice: many exact ties
        b = np.round(b * 4) / 4
    ref = oc.chamfer_forward(a, b)
    ok = True
    for variant in (0, 1, 2):
        out = C.chamfer_forward(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), variant=variant)
        ok = ok and all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(out, ref))
    return ok, f"B={B} n1={n1} n2={n2}"


def _wild_cloud(rng, B, n):
    """A cloud meant to break a spatial index: a mixture of components at random scales / offsets, then corruptions."""
    x = np.empty((B, n, 3), np.float32)
    for b in range(B):
        k = int(rng.integers(1, 5))
        centres = rng.standard_normal((k, 3)) * float(rng.choice([0.0, 0.3, 3.0, 300.0]))
        scales = 10.0 ** rng.uniform(-3, 1, (k, 1))
        pick = rng.integers(0, k, n)
        pts = centres[pick] + rng.standard_normal((n, 3)) * scales[pick]
        shape = rng.random()
        if shape < 0.15:
            pts[:, int(rng.integers(3))] = float(rng.standard_normal())  # a plane
        elif shape < 0.25:
            pts = centres[0] + np.outer(rng.standard_normal(n), rng.standard_normal(3))  # a line
        elif shape < 0.35:
            pts = np.round(pts * 4) / 4  # a lattice: exact ties
        x[b] = pts.astype(np.float32)
        if rng.random() < 0.4 and n >= 8:  # far outliers
            m = int(rng.integers(1, max(2, n // 10)))
            x[b, rng.integers(0, n, m)] *= np.float32(10.0 ** rng.integers(1, 8))
        if rng.random() < 0.4 and n >= 8:  # runs of one repeated point (the padded parts of shape_cd_loss)
            for _ in range(int(rng.integers(1, 6))):
                s0 = int(rng.integers(0, n - 1))
                x[b, s0:s0 + int(rng.integers(2, max(3, n // 3)))] = (np.float32(1e3) * rng.choice([0.0, 1.0])
                                                                      + rng.standard_normal(3).astype(np.float32))
        if rng.random() < 0.1:  # scattered duplicates of other points
            m = max(1, n // 5)
            x[b, rng.integers(0, n, m)] = x[b, rng.integers(0, n, m)]
        if rng.random() < 0.06:  # what sends a sample to the exhaustive scan
            x[b, int(rng.integers(n)), int(rng.integers(3))] = rng.choice([np.nan, np.inf, -np.inf, 3e16, -2e20])
    return x


def case_cgrid(rng):
    B = int(rng.integers(1, 10))
    big = rng.random() < 0.5
    n1 = int(rng.integers(1, 6000 if big else 700))
    n2 = int(rng.integers(1, 6000 if big else 700))
    a, b = _wild_cloud(rng, B, n1), _wild_cloud(rng, B, n2)
    if rng.random() < 0.25:
        m = min(n1, n2)
        b[:, :m] = a[:, :m]  # coincident clouds: zero distances everywhere
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    with np.errstate(all="ignore"):
        fast = C.chamfer_forward(ta, tb, variant=3)
        slow = C.chamfer_forward(ta, tb, variant=2)
    ok = all(torch.equal(f, s) or np.array_equal(f.cpu().numpy(), s.cpu().numpy(), equal_nan=True) for f, s in zip(fast, slow))
    if ok and B * n1 * n2 <= 4_000_000:
        ref = oc.chamfer_forward(a, b)
        ok = all(np.array_equal(g.cpu().numpy(), w, equal_nan=True) for g, w in zip(fast, ref))
    return ok, f"B={B} n1={n1} n2={n2}"


def case_cgate(rng):
    """The matrix-core gated search (variant 4, csrc/gate_nn.hip) on the clouds built to break a spatial index — here: to
    break a BOUND (scales from 1e-3 to 1e8 in one cloud, offsets of hundreds of units, planes, lines, lattices, runs of
    repeated points, coincident clouds, NaN / inf / huge coordinates), 1 to 3000 points, several LDS panels per cloud."""
    B = int(rng.integers(1, 10))
    big = rng.random() < 0.4
    n1 = int(rng.integers(1, 3000 if big else 700))
    n2 = int(rng.integers(1, 3000 if big else 700))
    a, b = _wild_cloud(rng, B, n1), _wild_cloud(rng, B, n2)
    r = rng.random()
    if r < 0.25:
        m = min(n1, n2)
        b[:, :m] = a[:, :m]  # coincident clouds: zero distances everywhere
    elif r < 0.35:
        b[:] = b[:, :1]  # one distinct target (the zero-padded parts of the per-part call)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    with np.errstate(all="ignore"):
        fast = C.chamfer_forward(ta, tb, variant=4)
        slow = C.chamfer_forward(ta, tb, variant=2)
    ok = all(torch.equal(f, s) or np.array_equal(f.cpu().numpy(), s.cpu().numpy(), equal_nan=True) for f, s in zip(fast, slow))
    if ok and B * n1 * n2 <= 4_000_000:
        ref = oc.chamfer_forward(a, b)
        ok = all(np.array_equal(g.cpu().numpy(), w, equal_nan=True) for g, w in zip(fast, ref))
    return ok, f"B={B} n1={n1} n2={n2}"


def case_knn3g(rng):
    """C = 3 kNN: the gated search (dg_knn3_gate.h) vs the exhaustive knn3_kernel on the same wild clouds, index for index."""
    n, N = int(rng.integers(1, 6)), int(rng.integers(20, 1025))
    x = torch.from_numpy(_wild_cloud(rng, n, N))
    rows = torch.cat([x.reshape(n * N, 3), torch.zeros(n * N, 1)], dim=1).to(dev).contiguous()
    os.environ["MPA_KNN3"] = "gate"
    got = knn_exact(rows, n, N, 3).cpu()
    os.environ["MPA_KNN3"] = "scan"
    want = knn_exact(rows, n, N, 3).cpu()
    os.environ.pop("MPA_KNN3")
    return bool(torch.equal(got, want)), f"n={n} N={N}"


def case_knn(rng):
    Cw = int(rng.choice([3, 3, 64, 128]))
    n, N = int(rng.integers(1, 6)), int(rng.integers(20, 1025))
    x = torch.from_numpy(rng.standard_normal((n, N, Cw)).astype(np.float32)) * (0.3 if Cw == 3 else 1.0)
    if Cw > 3 and rng.random() < 0.5:
        x = torch.where(x > 0, x, 0.2 * x)  # activations after a LeakyReLU, as the encoder's stages see them
    if rng.random() < 0.15:
        x[:, 1::2] = x[:, 0::2][:, : x[:, 1::2].shape[1]]  # duplicated points
    rows = x.reshape(n * N, Cw)
    if Cw == 3:
        rows = torch.cat([rows, torch.zeros(n * N, 1)], dim=1)
    got = knn_exact(rows.to(dev).contiguous(), n, N, Cw).cpu().view(n, N, 20).long()
    want = torch.from_numpy(oracle_knn(x.numpy())).long()
    return bool(torch.equal(got, want)), f"C={Cw} n={n} N={N}"


def case_glue(rng):
    rel = lambda a, b: float((a.double() - b).abs().max() / (b.abs().max() + 1e-12))
    fails = []

    def check(name, got, want, tol, lib32=None, scale=None, flips=0):
        """Within tol (relative to the largest entry) of float64.  For sums that cancel, `scale` is the entry-wise sum of
        the absolute addends (the error of ANY float32 evaluation is relative to that) or `lib32` the float32 library
        result (no further from float64 than twice that); `flips`: entries a ReLU on the rounding edge may move."""
        d = (got.double() - want).abs()
        lim = tol * want.abs().max() + 1e-12
        if scale is not None:
            lim = lim + 1e-5 * scale
        nbad = int((d > lim).sum())
        if nbad == 0 or nbad <= flips:
            return
        if lib32 is not None and float(d.max()) <= 2.0 * float((lib32.double() - want).abs().max()) + 1e-12:
            return
        fails.append(f"{name} {rel(got, want):.1e} ({nbad} entries)")

    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    R, K, N = int(rng.integers(1, 900)), int(rng.integers(1, 17)), int(rng.integers(1, 400))
    x = torch.randn(R, K, generator=g).to(dev).requires_grad_()
    w = torch.randn(N, K, generator=g).to(dev).requires_grad_()
    b = torch.randn(N, generator=g).to(dev).requires_grad_()
    go = torch.randn(R, N, generator=g).to(dev)
    out = narrow_linear_relu(x, w, b)
    out.backward(go)
    xd, wd, bd = (t.detach().double().requires_grad_() for t in (x, w, b))
    want = torch.relu(xd @ wd.t() + bd)
    want.backward(go.double())
    x3, w3, b3 = (t.detach().clone().requires_grad_() for t in (x, w, b))
    torch.relu(x3 @ w3.t() + b3).backward(go)  # float32 library ops: a ReLU on the rounding edge flips there too
    check("nl out", out.detach(), want.detach(), 1e-5)
    check("nl gx", x.grad, xd.grad, 1e-4, x3.grad, flips=2 * K)   # (one or two flipped (row, channel) entries)
    check("nl gw", w.grad, wd.grad, 1e-4, w3.grad, flips=2 * K)
    check("nl gb", b.grad, bd.grad, 1e-4, b3.grad, flips=2)
    S, P, F = int(rng.integers(1, 9)), int(rng.integers(1, 25)), 4 * int(rng.integers(1, 40))
    a = torch.randn(S, P, F, generator=g).to(dev).requires_grad_()
    c = torch.randn(S, P, F, generator=g).to(dev).requires_grad_()
    gw = torch.randn(S, P, P, 2 * F, generator=g).to(dev)
    swap = bool(rng.random() < 0.5)
    pr = pair_rows(a, c, swap=swap)
    pr.backward(gw)
    ad, cd = a.detach().double().requires_grad_(), c.detach().double().requires_grad_()
    halves = [ad[:, :, None].expand(S, P, P, F), cd[:, None].expand(S, P, P, F)]
    wantp = torch.cat(halves[::-1] if swap else halves, dim=-1)
    wantp.backward(gw.double())
    if not torch.equal(pr.detach().double(), wantp.detach()):
        fails.append("pr out")
    check("pr ga", a.grad, ad.grad, 1e-5)
    check("pr gb", c.grad, cd.grad, 1e-5)
    Cc = int(rng.integers(1, 300))
    e = torch.randn(S, P, P, Cc, generator=g).to(dev).requires_grad_()
    r = (torch.rand(S, P, P, generator=g) * (torch.rand(S, P, P, generator=g) < 0.7)).to(dev).requires_grad_()
    gm = torch.randn(S, P, Cc, generator=g).to(dev)
    rm = relation_mean(e, r)
    rm.backward(gm)
    ed, rd = e.detach().double().requires_grad_(), r.detach().double().requires_grad_()
    wantm = (ed * rd[..., None]).sum(dim=2) / (rd.sum(dim=-1, keepdim=True) + 1e-6)
    wantm.backward(gm.double())
    e3, r3 = e.detach().clone().requires_grad_(), r.detach().clone().requires_grad_()
    ((e3 * r3[..., None]).sum(dim=2) / (r3.sum(dim=-1, keepdim=True) + 1e-6)).backward(gm)
    check("rm out", rm.detach(), wantm.detach(), 1e-5)
    check("rm ge", e.grad, ed.grad, 1e-5)
    # (a row with ONE weight: the weight's gradient is the difference of two equal sums — any float32 evaluation is only
    # accurate relative to the sum of the absolute addends)
    den = rd.detach().sum(dim=-1, keepdim=True) + 1e-6
    addends = ((gm.double() / den)[:, :, None, :].abs() * (ed.detach().abs() + wantm.detach().abs()[:, :, None, :])).sum(-1)
    check("rm gr", r.grad, rd.grad, 1e-4, r3.grad, scale=addends)
    Rh, Kh = int(rng.integers(1, 3000)), 4 * int(rng.integers(1, 200))
    h = torch.randn(Rh, Kh, generator=g).to(dev).requires_grad_()
    wh = (torch.randn(1, Kh, generator=g) * 0.1).to(dev).requires_grad_()
    bh = torch.randn(1, generator=g).to(dev).requires_grad_()
    mk = (torch.rand(Rh, generator=g) < 0.6).float().to(dev)
    gh = torch.randn(Rh, generator=g).to(dev)
    rh = relation_head(h, wh, bh, mk)
    rh.backward(gh)
    hd, whd, bhd = (t.detach().double().requires_grad_() for t in (h, wh, bh))
    wanth = torch.sigmoid(hd @ whd.t() + bhd).view(-1) * mk.double()
    wanth.backward(gh.double())
    check("rh out", rh.detach(), wanth.detach(), 1e-5)
    check("rh gh", h.grad, hd.grad, 1e-4)
    dzs = (gh.double() * mk.double() * (torch.sigmoid(hd.detach() @ whd.detach().t() + bhd.detach()).view(-1)
                                        * (1 - torch.sigmoid(hd.detach() @ whd.detach().t() + bhd.detach()).view(-1)))).abs()
    check("rh gw", wh.grad, whd.grad, 1e-4, scale=(dzs[:, None] * hd.detach().abs()).sum(0, keepdim=True))
    check("rh gb", bh.grad, bhd.grad, 1e-4, scale=dzs.sum().view(1))
    return not fails, f"nl {R}x{K}x{N} pr {S}x{P}x{F} rm C={Cc} rh {Rh}x{Kh}: {fails}"


def case_nets(rng):
    from multi_part_assembly_amd.encoder import PointNet
    from multi_part_assembly_amd.regressor import PoseRegressor
    from multi_part_assembly_amd.transformer import TransformerEncoder
    from oracle import nets as on
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    rel = lambda a, b: float((a.double().cpu() - b.double().cpu()).abs().max() / (b.double().abs().max() + 1e-12))
    fails = []

    def check(name, hip, o32, o64, tol=2e-4):
        e, e32 = rel(hip, o64), rel(o32, o64)
        if not (e < tol or e <= 2.0 * e32 + 1e-6):
            fails.append(f"{name} {e:.1e} (float32 oracle {e32:.1e})")

    def oracle_grads(fn, sd, leaves, dtype):
        sdc = {k: v.detach().cpu().to(dtype if v.is_floating_point() else v.dtype).clone() for k, v in sd.items()}
        params = {k: sdc[k].requires_grad_() for k in sd if sd[k].is_floating_point() and "running" not in k}
        ls = [t.detach().cpu().to(dtype).requires_grad_() for t in leaves]
        outs, loss = fn(sdc, ls)
        loss.backward()
        return outs, ls, params

    if rng.random() < 0.5:
        M, N, F = int(rng.integers(1, 7)), int(rng.choice([20, 64, 150, 333])), int(rng.choice([64, 128, 256]))
        enc = PointNet(F).to(dev).train()
        with torch.no_grad():
            for i in range(1, 6):
                bn = getattr(enc, f"bn{i}")
                bn.weight.copy_(torch.randn(bn.weight.shape, generator=g))  # negative weights: the max becomes a min
                bn.bias.copy_(torch.randn(bn.bias.shape, generator=g) * 0.1)
        pts = torch.randn(M, N, 3, generator=g).to(dev)
        v = (torch.rand(M, generator=g) < 0.8).float()
        v[int(rng.integers(M))] = 1.0
        w = torch.randn(M, F, generator=g)
        sd0 = {k: t.clone() for k, t in enc.state_dict().items()}
        out = enc.forward_parts(pts, v.to(dev))
        (out * w.to(dev)).sum().backward()
        keep = v.bool()

        jit = [0.0]

        def fn(sd, ls, dtype=None):
            xin = pts.cpu().to(next(iter(sd.values())).dtype)[keep]
            if jit[0]:
                xin = xin * (1.0 + jit[0] * torch.randn(xin.shape, generator=g).to(xin.dtype))
            o = on.pointnet(xin, sd)
            return [o], (o * w[keep].to(o.dtype)).sum()
        o32, _, p32 = oracle_grads(fn, sd0, [], torch.float32)
        o64, _, p64 = oracle_grads(fn, sd0, [], torch.float64)
        check("pointnet feat", out.detach().cpu()[keep], o32[0].detach(), o64[0].detach())
        if float(out.detach().cpu()[~keep].abs().sum()) != 0.0:
            fails.append("pointnet padded rows")
        for k, p in enc.named_parameters():
            check("pointnet grad " + k, p.grad, p32[k].grad, p64[k].grad, tol=1e-3)
        if fails:  # is the float64 network itself discontinuous here (a ReLU / max on the rounding edge)?
            for trial in range(10):
                jit[0] = 2e-6 if trial < 5 else 2e-5
                _, _, pj = oracle_grads(fn, sd0, [], torch.float64)
                if any(rel(pj[k].grad, p64[k].grad) > 1e-3 for k in p64):
                    edge.append(f"pointnet {M}x{N}x{F}")
                    fails.clear()
                    break
        what = f"pointnet {M}x{N}x{F} valid {int(v.sum())}"
    else:
        B, P, D = int(rng.integers(1, 9)), int(rng.integers(2, 21)), int(rng.choice([64, 128, 256]))
        L, H = int(rng.integers(1, 5)), int(rng.choice([4, 8]))
        extra_w = int(rng.choice([0, 7, 39]))
        tf = TransformerEncoder(D, H, 4 * D, L, norm_first=True, dropout=0.0).to(dev).train()
        head = PoseRegressor(D + extra_w).to(dev).train()
        x = torch.randn(B, P, D, generator=g).to(dev).requires_grad_()
        extra = torch.randn(B, P, extra_w, generator=g)
        valid = torch.arange(P)[None] < torch.randint(1, P + 1, (B, 1), generator=g)
        wr, wt = torch.randn(B, P, 4, generator=g), torch.randn(B, P, 3, generator=g)
        rot, trans = head(torch.cat([tf(x, valid.to(dev)), extra.to(dev)], dim=-1))
        ((rot * wr.to(dev)).sum() + (trans * wt.to(dev)).sum()).backward()
        sd = {"tf." + k: t for k, t in tf.state_dict().items()} | {"head." + k: t for k, t in head.state_dict().items()}

        jit = [0.0]

        def fn(sdc, ls):
            dt = ls[0].dtype
            tok = ls[0] if not jit[0] else ls[0] * (1.0 + jit[0] * torch.randn(ls[0].shape, generator=g).to(dt))
            feats = on.transformer_encoder(tok, valid, sdc, "tf.", L, H)
            r, t = on.pose_head(torch.cat([feats, extra.to(dt)], dim=-1), sdc, "head.")
            return [r, t], (r * wr.to(dt)).sum() + (t * wt.to(dt)).sum()
        o32, l32, p32 = oracle_grads(fn, sd, [x], torch.float32)
        o64, l64, p64 = oracle_grads(fn, sd, [x], torch.float64)
        vm = valid[..., None]
        check("rot", rot.detach().cpu() * vm, o32[0].detach() * vm, o64[0].detach() * vm)
        check("trans", trans.detach().cpu() * vm, o32[1].detach() * vm, o64[1].detach() * vm)
        check("grad tokens", x.grad, l32[0].grad, l64[0].grad, tol=1e-3)
        for k, p in list(tf.named_parameters()):
            check("grad tf." + k, p.grad, p32["tf." + k].grad, p64["tf." + k].grad, tol=1e-3)
        for k, p in list(head.named_parameters()):
            check("grad head." + k, p.grad, p32["head." + k].grad, p64["head." + k].grad, tol=1e-3)
        if fails:
            for trial in range(10):
                jit[0] = 2e-6 if trial < 5 else 2e-5
                _, lj, pj = oracle_grads(fn, sd, [x], torch.float64)
                if rel(lj[0].grad, l64[0].grad) > 1e-3 or any(rel(pj[k].grad, p64[k].grad) > 1e-3 for k in p64):
                    edge.append(f"transformer {B}x{P}x{D}")
                    fails.clear()
                    break
        what = f"transformer {B}x{P}x{D} L={L} H={H} head +{extra_w}"
    return not fails, what + ": " + str(fails)


def case_dgcnn(rng):
    import copy
    import torch.nn.functional as Fn
    from multi_part_assembly_amd.encoder import DGCNN
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))
    n, N, feat = int(rng.integers(1, 6)), int(rng.integers(20, 401)), int(rng.choice([64, 128, 256]))
    enc = DGCNN(feat)
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.weight[::5] *= -1.0  # negative scales take the min branch of the aggregation
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    enc = enc.to(dev).train()
    x = (torch.randn(n, N, 3, generator=g) * 0.2).to(dev)
    w = torch.randn(n, feat, generator=g).to(dev)
    xa = x.clone().requires_grad_()
    enc.graph_hooks = {"export": True}
    out = enc(xa)
    (out * w).sum().backward()
    graphs = [t.clone() for t in enc.graph_hooks["exported"]]
    enc.graph_hooks = None

    def formulation(ref, xin):  # dgcnn.py:8-109 on materialised edge tensors, graphs given
        h, stages = xin, []
        for l, conv in enumerate((ref.conv1, ref.conv2, ref.conv3, ref.conv4)):
            C = h.shape[-1]
            idx = graphs[l].view(n, N, 20).long()
            flat = (idx + torch.arange(n, device=dev).view(-1, 1, 1) * N).view(-1)
            nbr = h.reshape(n * N, C)[flat].view(n, N, 20, C)
            ctr = h[:, :, None].expand(n, N, 20, C)
            edge = torch.cat((nbr - ctr, ctr), dim=3).permute(0, 3, 1, 2)
            bn = conv[1]
            e = Fn.leaky_relu(Fn.batch_norm(Fn.conv2d(edge, conv[0].weight), None, None, bn.weight, bn.bias, True, 0.1, bn.eps), 0.2)
            h = e.max(dim=-1)[0].permute(0, 2, 1)
            stages.append(h)
        y = Fn.conv1d(torch.cat(stages, dim=2).permute(0, 2, 1), ref.conv5[0].weight)
        y = Fn.leaky_relu(Fn.batch_norm(y, None, None, ref.bn5.weight, ref.bn5.bias, True, 0.1, ref.bn5.eps), 0.2)
        return ref.out_fc(torch.cat((y.max(dim=-1)[0], y.mean(dim=-1)), dim=1))

    def run(dtype, jitter=0.0):
        ref = copy.deepcopy(enc).to(dtype)
        ref.zero_grad()
        xin = x.detach().to(dtype).clone()
        if jitter:
            xin = xin * (1.0 + jitter * torch.randn(xin.shape, generator=g).to(dev).to(dtype))
        xin = xin.requires_grad_()
        o = formulation(ref, xin)
        (o * w.to(dtype)).sum().backward()
        return o.detach(), xin.grad, {k: p.grad for k, p in ref.named_parameters()}

    o32, gx32, p32 = run(torch.float32)
    o64, gx64, p64 = run(torch.float64)
    fails = []

    def check(name, hip, a32, a64, tol):
        e, e32 = rel(hip, a64), rel(a32, a64)
        if not (e < tol or e <= 2.0 * e32 + 1e-6):
            fails.append(f"{name} {e:.1e} (float32 formulation {e32:.1e})")

    check("feat", out.detach(), o32, o64, 2e-4)
    check("grad x", xa.grad, gx32, gx64, 1e-3)
    for k, p in enc.named_parameters():
        if p.grad is None or p64[k] is None:
            if (p.grad is None) != (p64[k] is None):
                fails.append(f"grad {k}: present on one side only")
            continue
        check("grad " + k, p.grad, p32[k], p64[k], 1e-3)
    if fails:  # a max over the 20 neighbours / a LeakyReLU on the rounding edge?
        for trial in range(10):
            _, gj, pj = run(torch.float64, 2e-6 if trial < 5 else 2e-5)
            if rel(gj, gx64) > 1e-3 or any(rel(pj[k], p64[k]) > 1e-3 for k in p64 if p64[k] is not None):
                edge.append(f"dgcnn {n}x{N}x{feat}")
                fails.clear()
                break
    return not fails, f"dgcnn {n}x{N}x{feat}: {fails}"


def _whole_step(rng, g, cfg, B, P, N, oracle_total, label, make=None, reseed=None):
    """forward_pass + backward of build_model(cfg) on the HIP path against oracle_total(sd, cpu_batch) -> scalar in float64."""
    from multi_part_assembly_amd.pn_transformer import build_model
    rel = lambda a, b: float((a.double().cpu() - b.double().cpu()).abs().max() / (b.double().abs().max() + 1e-12))
    model = build_model(cfg)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    names = [k for k, _ in model.named_parameters()]
    if make is None:
        batch = synthetic.make_batch(B, P, N, preset="everyday", seed=int(rng.integers(1 << 30)), device=dev,
                                     num_parts=[int(rng.integers(2, P + 1)) for _ in range(B)])
    else:
        batch = make()
    batch.pop("num_parts", None)
    model.to(dev).train()
    if reseed is not None:  # models that draw noise: every evaluation sees the same draws
        torch.manual_seed(reseed)
    loss = model.training_step(batch, 0)
    loss.backward()
    hip = {k: p.grad.detach().cpu().double() for k, p in model.named_parameters() if p.grad is not None}

    def oracle(dt, jitter=0.0):
        sd = {k: (v.clone().to(dt) if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
        params = {k: sd[k].requires_grad_() for k in names}
        cb = {k: (v.cpu().to(dt) if v.is_floating_point() else v.cpu()) for k, v in batch.items() if hasattr(v, "cpu")}
        if jitter:
            cb["part_pcs"] = cb["part_pcs"] * (1.0 + jitter * torch.randn(cb["part_pcs"].shape, generator=g).to(dt))
        if reseed is not None:
            torch.manual_seed(reseed)
        total = oracle_total(sd, cb)
        total.backward()
        return float(total.detach()), {k: p.grad.double() for k, p in params.items() if p.grad is not None}

    l32, g32 = oracle(torch.float32)
    l64, g64 = oracle(torch.float64)
    fails = []
    if abs(float(loss.detach()) - l64) > 2.0 * abs(l32 - l64) + 1e-4 * abs(l64):
        fails.append(f"loss {float(loss.detach()):.7f} vs {l64:.7f} (float32 oracle {l32:.7f})")
    for k, b in g64.items():
        if float(b.abs().max()) < 1e-10:  # a bias in front of a BatchNorm: structurally zero
            continue
        if k not in hip:
            fails.append(f"grad {k} missing")
            continue
        e, e32 = rel(hip[k], b), rel(g32[k], b)
        if not (e < 2e-4 or e <= 2.0 * e32 + 1e-6):
            fails.append(f"grad {k} {e:.1e} (float32 oracle {e32:.1e})")
    if fails:  # a nearest neighbour of the Chamfer matching, a kNN graph, a max over the points or a ReLU on the rounding edge?
        for trial in range(8):
            _, gj = oracle(torch.float64, 2e-6 if trial < 4 else 2e-5)
            if any(rel(gj[k], g64[k]) > 1e-3 for k in g64 if float(g64[k].abs().max()) >= 1e-10):
                edge.append(f"{label} {B}x{P}x{N}")
                fails.clear()
                break
    return not fails, f"{label} B={B} P={P} N={N}: {fails[:6]}"


def case_step(rng):
    from multi_part_assembly_amd import config
    from oracle import nets as on
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    B, P, N = int(rng.integers(1, 5)), int(rng.integers(2, 9)), int(rng.choice([32, 64, 100, 200]))
    cfg = config.pn_transformer_everyday()
    cfg.model.pc_feat_dim = int(rng.choice([128, 256]))
    cfg.model.transformer_heads = int(rng.choice([4, 8]))
    cfg.model.transformer_feat_dim = int(rng.choice([256, 512]))
    cfg.model.transformer_layers = int(rng.integers(1, 4))
    cfg.data.max_num_part = P
    return _whole_step(rng, g, cfg, B, P, N,
                       lambda sd, cb: on.pn_transformer_loss(sd, cb, cfg.model.transformer_layers, cfg.model.transformer_heads)[0]["loss"],
                       f"pn_transformer D={cfg.model.pc_feat_dim} L={cfg.model.transformer_layers}")


def case_gnn(rng):
    from multi_part_assembly_amd import config
    from oracle import callers as oc
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    B, P, N = int(rng.integers(1, 4)), int(rng.integers(2, 9)), int(rng.choice([32, 64, 100, 200]))
    cfg = config.dgl_dgcnn_everyday()
    cfg.model.encoder = str(rng.choice(["dgcnn", "pointnet"]))
    cfg.data.max_num_part = P
    return _whole_step(rng, g, cfg, B, P, N,
                       lambda sd, cb: oc.dgl_loss(sd, cb, cfg.model.gnn_iter, cfg.model.encoder, True, {})["loss"],
                       f"dgl + {cfg.model.encoder}")


def case_global(rng):
    from multi_part_assembly_amd import config
    from oracle import callers as oc
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    B, P, N = int(rng.integers(1, 5)), int(rng.integers(2, 7)), int(rng.choice([32, 64, 100, 200]))
    cfg = config.global_partnet_chair()
    cfg.data.max_num_part = P
    loss_cfg = {k: cfg.loss[k] for k in cfg.loss}
    bseed = int(rng.integers(1 << 30))
    make = lambda: synthetic.make_semantic_batch(B, P, N, seed=bseed, device=dev, num_part_category=cfg.data.num_part_category)
    return _whole_step(rng, g, cfg, B, P, N,
                       lambda sd, cb: oc.global_loss(sd, cb, loss_cfg, cfg.loss.sample_iter, cfg.loss.noise_dim, cfg.model.encoder,
                                                     True, {})["loss"],
                       "b-global (semantic: matching, min-of-N sampling, noise)", make=make, reseed=int(rng.integers(1 << 30)))


def case_adam(rng):
    """The fused optimiser against torch.optim.Adam / AdamW (+ clip_grad_norm_) over a few steps on random tensor sets."""
    from multi_part_assembly_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    shapes = [tuple(int(v) for v in rng.integers(1, 40, size=int(rng.integers(1, 4)))) for _ in range(int(rng.integers(1, 9)))]
    ref_p = [torch.randn(*sh, generator=g).to(dev) for sh in shapes]
    wd = float(rng.choice([0.0, 0.0, 0.01, 0.1]))
    lr = float(rng.choice([1e-4, 1e-3, 1e-2]))
    clip = float(rng.choice([0.0, 0.0, 0.05, 5.0]))
    mine = [torch.nn.Parameter(p.clone()) for p in ref_p]
    theirs = [torch.nn.Parameter(p.clone()) for p in ref_p]
    opt = FusedAdam(mine, lr=lr, weight_decay=wd, clip_grad=clip if clip > 0 else None)
    topt = (torch.optim.AdamW if wd > 0 else torch.optim.Adam)(theirs, lr=lr, weight_decay=wd)
    for step in range(int(rng.integers(1, 8))):
        opt.zero_grad()
        topt.zero_grad()
        scale = float(rng.choice([1e-3, 1.0, 30.0]))
        for a, b in zip(mine, theirs):
            gr = torch.randn(a.shape, generator=g).to(dev) * scale
            a.grad.copy_(gr)
            b.grad = gr.clone()
        if clip > 0:
            torch.nn.utils.clip_grad_norm_(theirs, clip)
        opt.step()
        topt.step()
    ok = all(bool(((a.detach() - b.detach()).abs() <= 1e-5 * b.detach().abs() + 1e-6 * lr / 1e-3 + 1e-7).all()) for a, b in zip(mine, theirs))
    return ok, f"adam {len(shapes)} tensors wd={wd} lr={lr} clip={clip}"


def case_graph(rng):
    """A HIP-graph replay of the whole training step walks the same parameter trajectory, bit for bit, as eager launches."""
    from multi_part_assembly_amd import config
    from multi_part_assembly_amd.pn_transformer import build_model
    from multi_part_assembly_amd.trainer import Trainer
    B, P, N = int(rng.integers(1, 5)), int(rng.integers(2, 9)), int(rng.choice([32, 64, 100, 200]))
    which = str(rng.choice(["pn_transformer", "dgl"]))
    cfg = config.pn_transformer_everyday() if which == "pn_transformer" else config.dgl_dgcnn_everyday()
    cfg.data.max_num_part = P
    cfg.optimizer.lr_scheduler = ""
    if which == "pn_transformer":
        cfg.model.transformer_layers = int(rng.integers(1, 3))
    batch = synthetic.make_batch(B, P, N, preset="everyday", seed=int(rng.integers(1 << 30)), device=dev,
                                 num_parts=[int(rng.integers(2, P + 1)) for _ in range(B)])
    batch.pop("num_parts", None)
    seed = int(rng.integers(1 << 30))
    finals, losses = [], []
    for use_graph in (False, True):
        torch.manual_seed(seed)
        model = build_model(cfg).to(dev)
        tr = Trainer(model, cfg, use_graph=use_graph, graph_warmup=1)
        ls = [float(tr.train_step(batch)) for _ in range(4)]
        torch.cuda.synchronize()
        finals.append(tr.flat.flat_param.clone())
        losses.append(ls)
    ok = torch.equal(finals[0], finals[1]) and losses[0] == losses[1]
    return bool(ok), f"graph vs eager {which} B={B} P={P} N={N}: losses {losses[0][-1]} / {losses[1][-1]}"


def case_repro(rng):
    from multi_part_assembly_amd.encoder import DGCNN, PointNet
    from multi_part_assembly_amd.gru import gru_recurrent
    from multi_part_assembly_amd.loss import geometric_assembly_loss
    from multi_part_assembly_amd.mlp import mlp_layer
    from multi_part_assembly_amd.regressor import PoseRegressor
    from multi_part_assembly_amd.transformer import TransformerEncoder
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    fails = []

    def twice(name, module_params, run):
        res = []
        for _ in range(2):
            for p in module_params:
                p.grad = None
            outs, leaves = run()
            res.append([o.detach().clone() for o in outs] + [t.grad.clone() for t in leaves if t.grad is not None]
                       + [p.grad.clone() for p in module_params if p.grad is not None])
        if len(res[0]) != len(res[1]) or not all(torch.equal(a, b) for a, b in zip(*res)):
            fails.append(name)

    which = int(rng.integers(0, 6))
    if which == 0:
        M, N, F = int(rng.integers(1, 12)), int(rng.choice([64, 333, 1000])), int(rng.choice([128, 256]))
        enc = PointNet(F).to(dev).train()
        pts = torch.randn(M, N, 3, generator=g).to(dev)
        v = (torch.rand(M, generator=g) < 0.8).float().to(dev)
        w = torch.randn(M, F, generator=g).to(dev)

        def run():
            out = enc.forward_parts(pts, v)
            (out * w).sum().backward()
            return [out], []
        twice(f"pointnet {M}x{N}x{F}", list(enc.parameters()), run)
    elif which == 1:
        M, N, F = int(rng.integers(1, 8)), int(rng.choice([40, 200, 1000])), int(rng.choice([64, 128]))
        enc = DGCNN(F).to(dev).train()
        pts = (torch.randn(M, N, 3, generator=g) * 0.3).to(dev)
        v = (torch.rand(M, generator=g) < 0.8).float().to(dev)
        w = torch.randn(M, F, generator=g).to(dev)

        def run():
            out = enc.forward_parts(pts, v)
            (out * w).sum().backward()
            return [out], []
        twice(f"dgcnn {M}x{N}x{F}", list(enc.parameters()), run)
    elif which == 2:
        B, P, D = int(rng.integers(1, 33)), int(rng.integers(2, 21)), int(rng.choice([64, 128, 256]))
        tf = TransformerEncoder(D, int(rng.choice([4, 8])), 4 * D, int(rng.integers(1, 5)), norm_first=True, dropout=0.0).to(dev).train()
        head = PoseRegressor(D + int(rng.choice([0, 7, 39]))).to(dev).train()
        x = torch.randn(B, P, D, generator=g).to(dev).requires_grad_()
        extra = torch.randn(B, P, head.fc_layers[0].in_features - D, generator=g).to(dev)
        valid = (torch.arange(P)[None] < torch.randint(1, P + 1, (B, 1), generator=g)).to(dev)

        def run():
            x.grad = None
            rot, trans = head(torch.cat([tf(x, valid), extra], dim=-1))
            (rot.sum() + trans.square().sum()).backward()
            return [rot, trans], [x]
        twice(f"transformer + head {B}x{P}x{D}", list(tf.parameters()) + list(head.parameters()), run)
    elif which == 3:
        R, K, N = int(rng.integers(1, 3000)), 64 * int(rng.integers(1, 9)), 64 * int(rng.integers(1, 9))
        lin = torch.nn.Linear(K, N).to(dev)
        bn = torch.nn.BatchNorm1d(N).to(dev).train() if rng.random() < 0.7 and R > 1 else None
        x = torch.randn(R, K, generator=g).to(dev).requires_grad_()
        w = torch.randn(R, N, generator=g).to(dev)

        def run():
            x.grad = None
            if bn is not None:
                bn.running_mean.zero_(), bn.running_var.fill_(1.0), bn.num_batches_tracked.zero_()
            out = mlp_layer(x, lin.weight, lin.bias, bn, relu=True)
            (out * w).sum().backward()
            return [out], [x]
        twice(f"mlp layer {R}x{K}x{N}", list(lin.parameters()) + (list(bn.parameters()) if bn is not None else []), run)
    elif which == 4:
        H, B, T = int(rng.choice([128, 256])), int(rng.integers(1, 41)), int(rng.integers(1, 30))
        gi = torch.randn(2, B, T, 3 * H, generator=g).to(dev).requires_grad_()
        h0 = torch.randn(2, B, H, generator=g).to(dev)
        whh = (torch.randn(2, 3 * H, H, generator=g) * 0.05).to(dev).requires_grad_()
        bhh = torch.randn(2, 3 * H, generator=g).to(dev).requires_grad_()
        w = torch.randn(2, B, T, H, generator=g).to(dev)

        def run():
            gi.grad = whh.grad = bhh.grad = None
            out = gru_recurrent(gi, h0, whh, bhh)
            (out * w).sum().backward()
            return [out], [gi, whh, bhh]
        twice(f"gru {H}x{B}x{T}", [], run)
    else:
        B, P, N = int(rng.integers(1, 17)), int(rng.integers(1, 21)), int(rng.choice([64, 500, 1000]))
        batch = synthetic.make_batch(B, P, N, seed=int(rng.integers(1 << 30)), device=dev,
                                     num_parts=[int(rng.integers(1, P + 1)) for _ in range(B)])
        q = torch.nn.functional.normalize(torch.randn(B, P, 4, generator=g), dim=-1).to(dev).requires_grad_()
        t = (torch.randn(B, P, 3, generator=g) * 0.4).to(dev).requires_grad_()

        def run():
            q.grad = t.grad = None
            terms, _ = geometric_assembly_loss(batch["part_pcs"], t, Rotation3D(q), batch["part_trans"],
                                               Rotation3D(batch["part_quat"]), batch["part_valids"], training=True)
            sum(v.sum() for v in terms.values()).backward()
            return list(terms.values()), [q, t]
        twice(f"loss {B}x{P}x{N}", [], run)
    return not fails, str(fails)


families = [("loss", case_loss), ("chamfer", case_chamfer), ("knn", case_knn), ("glue", case_glue), ("repro", case_repro),
            ("nets", case_nets), ("dgcnn", case_dgcnn), ("step", case_step),
            ("gnn", case_gnn), ("global", case_global),
            ("adam", case_adam), ("graph", case_graph), ("cgrid", case_cgrid), ("cgate", case_cgate), ("knn3g", case_knn3g),
            ("lossgrad", case_lossgrad)]  # (a case is a function of (seed, position): new families go to the end)


def run_case(name, seed):
    """One case of family `name`: (ok, description).  A case is a function of (family, seed) only."""
    fam = [k for k, _ in families].index(name)
    rng = np.random.default_rng([seed, fam])
    torch.manual_seed(seed * 16 + fam)  # module initialisations draw from the global generator
    try:
        return families[fam][1](rng)
    except Exception as exc:  # a refused shape is a finding too
        return False, f"exception {type(exc).__name__}: {exc}"


def main(argv):
    budget = float(argv[1]) if len(argv) > 1 else 240.0
    seed0 = int(argv[2]) if len(argv) > 2 else 0
    only = argv[3].split(",") if len(argv) > 3 else None  # families to run (default: all)
    counts = {k: 0 for k, _ in families}
    t_end = time.time() + budget
    seed = seed0
    while time.time() < t_end:
        for name, _ in families:
            if only is not None and name not in only:
                continue
            ok, what = run_case(name, seed)
            counts[name] += 1
            if not ok:
                bad.append((name, seed, what))
                print(f"MISMATCH {name} seed {seed}: {what}", flush=True)
        seed += 1
    if edge and os.environ.get("MPA_FUZZ_LIST_EDGE"):
        from collections import Counter
        print("set aside by kind:", dict(Counter(e.split()[0] for e in edge)))
        print("set aside:", "; ".join(edge[:60]))
    if edge:
        print(f"nets / dgcnn / step / gnn / global: {len(edge)} cases set aside: the float64 oracle's own gradients move by > 1e-3 "
              f"under a 2e-6 .. 2e-5 relative input change (a ReLU / max on the rounding edge)")
    for name, _ in families:
        print(f"{name}: {counts[name]} random cases (seeds {seed0}..{seed - 1}), {sum(1 for b in bad if b[0] == name)} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
