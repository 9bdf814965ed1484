"""csrc/eval_metrics.hip at the edges of its envelope, against tests/eval_ref.py (a float64 restatement that
tests/test_eval_ref.py holds against the reference's recorded outputs on the CPU): every path of `nn_sum` (clouds smaller
than a wave, the scalar target tail at N % 4 = 1, 2, 3, the second sweep at 1024 < N <= 2048), the 0.01 threshold from both
sides, rotations at the asin pole / at the 360 - d wrap / on each `matrix_to_quat` candidate, `batch_metrics_kernel`
beyond one block, samples without a valid part, `valids` other than 0 or 1, the connectivity kernel's flags and sizes,
and the input forms the wrapper accepts.  tests/test_eval_metrics_gpu.py keeps the two recorded shapes.

Conditions on the inputs (distance of a value from the threshold, gap between arg-max candidates, which branch a case
takes) are asserted on the float64 reference values, never assumed."""
import ctypes
import math
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import eval_ref
from multi_part_assembly_amd import _lib, eval_utils
from multi_part_assembly_amd.chamfer import chamfer_distance
from multi_part_assembly_amd.rotation import Rotation3D, quat_to_matrix
from multi_part_assembly_amd.transforms import transform_pc

pytestmark = pytest.mark.gpu

KINDS = ("quat", "rmat")
EPS = 2.0 ** -24  # one float32 rounding, relative
METRICS = ("mse", "rmse", "mae")
NOISE = (0.0, 0.01, 0.3)  # prediction noise per part slot, cycled: exact, near, far (make_golden_eval.py's mix)


# ---- shared pieces --------------------------------------------------------------------------------------------------------------
def _rotations(pr_q, gt_q, kind, dev):
    """Rotation3D pair of one kind from float32 CPU quaternions; 'rmat' through the CPU quat_to_matrix, so a part whose two
    quaternions are equal gets two equal matrices."""
    if kind == "quat":
        return Rotation3D(pr_q.to(dev)), Rotation3D(gt_q.to(dev))
    return Rotation3D(quat_to_matrix(pr_q).to(dev), "rmat"), Rotation3D(quat_to_matrix(gt_q).to(dev), "rmat")


def _fused(d, per_part=False):
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # inside the envelope: the fused path, silently
        return eval_utils.assembly_metrics(d["pts"], d["pr_t"], d["gt_t"], d["pr_r"], d["gt_r"], d["valids"],
                                           ret_per_part=per_part)


def _bits_equal(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in eval_utils.METRIC_KEYS) and list(a) == list(b)


def _posed(d):
    """The two posed float32 clouds of the package's own pose operator, [B, P, N, 3] each (the kernel's header: its
    coordinates are those of `pose_apply`)."""
    return transform_pc(d["pr_t"], d["pr_r"], d["pts"]), transform_pc(d["gt_t"], d["gt_r"], d["pts"])


def _check_trans(got, d):
    """Translation metrics against the float64 restatement: rtol 1e-5 (the bound tests/test_eval_metrics_gpu.py applies
    against the reference's recorded values); NaN exactly where the restatement has 0 / 0."""
    ref = eval_ref.trans_metrics(d["pr_t"], d["gt_t"], d["valids"])
    for m in METRICS:
        np.testing.assert_allclose(got[f"trans_{m}"].double().cpu().numpy(), ref[m].numpy(), rtol=1e-5, atol=0.0,
                                   equal_nan=True, err_msg=f"trans_{m}")


def _check_rot(got, d, kind):
    """The rule of test_rot_metrics_error_against_float64: kernel error <= max(2 x the error of the unchanged
    eval_utils.rot_metrics, 4 float32 ulp of the value), both against the float64 restatement; exactly 0 where the
    restatement is exactly 0, NaN exactly where it is NaN.  -> per-sample errors in ulp {metric: (kernel, composition)}."""
    ref = eval_ref.rot_metrics(d["pr_r"].rot, d["gt_r"].rot, kind, d["valids"])
    ulps = {}
    for m in METRICS:
        r = ref[m].numpy()
        mine = got[f"rot_{m}"].double().cpu().numpy()
        comp = eval_utils.rot_metrics(d["pr_r"], d["gt_r"], d["valids"], m).double().cpu().numpy()
        nan, zero = np.isnan(r), r == 0.0
        assert (np.isnan(mine) == nan).all(), (m, mine, r)
        assert (mine[zero] == 0.0).all(), (m, mine[zero])
        sel = ~nan & ~zero
        ulp = np.ones_like(r)
        ulp[sel] = np.spacing(np.abs(r[sel]).astype(np.float32)).astype(np.float64)
        e_mine = np.where(sel, np.abs(mine - r), 0.0)
        e_comp = np.where(sel, np.nan_to_num(np.abs(comp - r), nan=0.0), 0.0)
        assert (e_mine <= np.maximum(2 * e_comp, 4 * ulp)).all(), (m, (e_mine / ulp).max(), (e_comp / ulp).max())
        ulps[m] = (e_mine / ulp, e_comp / ulp)
    return ulps


def _check_part_acc(got, per_part64, valids):
    """Part accuracy against the integer counts, exactly — after asserting on the float64 values that no part with
    valids == 1 lies within 1e-3 (relative) of the threshold, 100x what the two float32 sums can move a value."""
    v = eval_ref.f64(valids)
    assert eval_ref.threshold_margin(per_part64[v == 1]) > 1e-3
    ok, n = eval_ref.part_acc_counts(per_part64, v)
    np.testing.assert_array_equal(got["part_acc"].cpu().numpy(), eval_ref.ratio32(ok, n))
    return ok, n


def _random_batch(B, P, N, seed, kind, dev, valids=None):
    """Clouds of scale 0.2, ground-truth poses, predictions with the NOISE mix (slot (b, p) takes NOISE[(b + p) % 3]);
    parts with noise 0 carry the ground truth's bits.  Slots with valids == 0 hold large finite junk everywhere."""
    g = torch.Generator().manual_seed(seed)
    if valids is None:
        valids = torch.ones(B, P)
    pts = torch.randn(B, P, N, 3, generator=g) * 0.2
    scale = torch.tensor([[NOISE[(b + p) % 3] for p in range(P)] for b in range(B)])[..., None]
    gt_t = torch.randn(B, P, 3, generator=g) * 0.3
    pr_t = gt_t + scale * torch.randn(B, P, 3, generator=g)
    gt_q = F.normalize(torch.randn(B, P, 4, generator=g), dim=-1)
    pr_q = torch.where(scale == 0, gt_q, F.normalize(gt_q + scale * torch.randn(B, P, 4, generator=g), dim=-1))
    pad = valids == 0
    junk = lambda t: torch.where(pad.reshape(B, P, *[1] * (t.dim() - 2)), torch.randn(t.shape, generator=g) * 1e3, t)
    pts, gt_t, pr_t, gt_q, pr_q = junk(pts), junk(gt_t), junk(pr_t), junk(gt_q), junk(pr_q)
    pr_r, gt_r = _rotations(pr_q, gt_q, kind, dev)
    return dict(pts=pts.to(dev), valids=valids.to(dev), gt_t=gt_t.to(dev), pr_t=pr_t.to(dev), pr_r=pr_r, gt_r=gt_r,
                exact=(scale[..., 0] == 0) & ~pad)


# ---- a. point counts ----------------------------------------------------------------------------------------------------------------
# 1-5: clouds far smaller than a wave, every N % 4; 63-65 and 255-257: the wave and the block; 1023-1025: the end of the first
# sweep of 4 x 256 queries; 1500, 2046-2048: the second sweep (up to 8 terms per thread), again with every N % 4.
POINT_COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1500, 2046, 2047, 2048)


def point_count_batch(N, kind, dev):
    B, P = (3, 4) if N <= 257 else (2, 3)
    valids = torch.ones(B, P)
    valids[1, P - 1] = 0.0  # one padded slot
    return _random_batch(B, P, N, 4000 + N, kind, dev, valids)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", POINT_COUNTS)
def test_point_counts(cuda_device, N, kind):
    d = point_count_batch(N, kind, cuda_device)
    B, P = d["valids"].shape
    got, per_part = _fused(d, per_part=True)
    assert per_part.shape == (B, P) and all(got[k].shape == (B,) for k in eval_utils.METRIC_KEYS)
    valid = (d["valids"] == 1).cpu()
    exact = d["exact"]
    assert exact.any() and (~valid).any() and (valid & ~exact).any()
    mine = per_part.double().cpu()

    # the Chamfer operator's own float32 distances, averaged in float64: the kernel's minima are those distances bit for
    # bit and its two sums are <= 8 terms per thread + 6 wave levels + 3 waves + a division + the final addition = 20
    # float32 roundings of positive terms (the kernel's header; 8 terms per thread only at N > 1792)
    a, b = _posed(d)
    d1, d2 = chamfer_distance(a.flatten(0, 1), b.flatten(0, 1))
    op = (d1.double().mean(1) + d2.double().mean(1)).view(B, P).cpu()
    sel = valid & ~exact
    assert (op[sel] > 0).all()
    rel_op = float(((mine - op).abs() / op)[sel].max())
    # float64 brute force on the same float32 posed coordinates: each distance (dx*dx + dy*dy) + dz*dz carries at most 5
    # roundings, the rounded differences counted, on top of the 20 of the sums; 32 covers the second-order terms
    ref = eval_ref.chamfer_per_part(a.cpu(), b.cpu())
    assert (ref[sel] > 0).all()
    rel_ref = float(((mine - ref).abs() / ref)[sel].max())
    print(f"N={N} {kind}: per-part Chamfer, worst relative error {rel_op:.3e} against the operator (bound {20 * EPS:.2e}), "
          f"{rel_ref:.3e} against float64 (bound {32 * EPS:.2e})")
    assert rel_op <= 20 * EPS
    assert rel_ref <= 32 * EPS

    # identical poses: both clouds carry the same bits, every minimum is 0; padded slots are written as 0
    assert (ref[exact] == 0).all() and (op[exact] == 0).all()
    assert torch.equal(per_part.cpu()[exact], torch.zeros(int(exact.sum())))
    assert torch.equal(per_part.cpu()[~valid], torch.zeros(int((~valid).sum())))

    ok, n = _check_part_acc(got, ref, d["valids"])
    assert 0 < int(ok.sum()) < int(n.sum())  # correct and wrong parts in every batch
    _check_trans(got, d)
    _check_rot(got, d, kind)

    again, per_part2 = _fused(d, per_part=True)
    assert _bits_equal(got, again) and torch.equal(per_part.view(torch.int32), per_part2.view(torch.int32))


# ---- b. the threshold, from both sides ------------------------------------------------------------------------------------------
def lattice(N):
    """The first N points of a centred cubic lattice of spacing 0.25 (every coordinate exact in float32)."""
    k = next(k for k in range(1, 64) if k ** 3 >= N)
    ax = (torch.arange(k, dtype=torch.float64) - (k - 1) / 2) * 0.25
    return torch.cartesian_prod(ax, ax, ax)[:N].float()


SHIFT_DIR = torch.tensor([0.6, -0.64, 0.48], dtype=torch.float64)  # a unit vector


def threshold_batch(N, shared_rotation, kind, dev):
    """B = 2, P = 3.  Both copies of a part share the rotation and differ by a translation d with 2 |d|^2 = 0.01 (1 -+ 1e-3):
    |d| = 0.0707 is below half the lattice spacing, every point's nearest neighbour is its own image, the per-part value
    is 2 |d|^2.  Slot (b, p) lies below the threshold when b + p is even."""
    B, P = 2, 3
    below = torch.tensor([[(b + p) % 2 == 0 for p in range(P)] for b in range(B)])
    target = 0.01 * (1 + 1e-3 * (1 - 2 * below.double()))
    g = torch.Generator().manual_seed(5100 + N)
    gt_t = torch.randn(B, P, 3, generator=g) * 0.3
    signs = torch.tensor([[[1.0, 1, 1], [-1, 1, 1], [1, -1, 1]], [[1, 1, -1], [-1, -1, 1], [-1, 1, -1]]], dtype=torch.float64)
    delta = (target / 2).sqrt()[..., None] * SHIFT_DIR * signs
    pr_t = (gt_t.double() + delta).float()
    q = F.normalize(torch.tensor([0.8, 0.3, -0.4, 0.33]), dim=-1) if shared_rotation else torch.tensor([1.0, 0, 0, 0])
    q = q.repeat(B, P, 1)
    pr_r, gt_r = _rotations(q, q.clone(), kind, dev)
    pts = lattice(N).repeat(B, P, 1, 1)
    return dict(pts=pts.to(dev), valids=torch.ones(B, P, device=dev), gt_t=gt_t.to(dev), pr_t=pr_t.to(dev), pr_r=pr_r,
                gt_r=gt_r, below=below, target=target)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shared_rotation", [False, True], ids=["identity", "rotated"])
@pytest.mark.parametrize("N", [257, 1025])
def test_threshold_from_both_sides(cuda_device, N, shared_rotation, kind):
    d = threshold_batch(N, shared_rotation, kind, cuda_device)
    got, per_part = _fused(d, per_part=True)
    a, b = _posed(d)
    ref = eval_ref.chamfer_per_part(a.cpu(), b.cpu())
    # the construction holds on the float32 clouds the kernel sees: each value within 1e-4 (relative) of its target, so
    # 0.9e-3 away from the threshold on the intended side — about 400x the 32 * 2^-24 = 1.9e-6 bound below
    assert float(((ref - d["target"]).abs() / d["target"]).max()) < 1e-4, ref
    assert ((ref < 0.01) == d["below"]).all() and eval_ref.threshold_margin(ref) > 0.9e-3
    mine = per_part.double().cpu()
    rel = float(((mine - ref).abs() / ref).max())
    print(f"N={N} {kind} {'rotated' if shared_rotation else 'identity'}: per-part values {mine.flatten().tolist()}, worst "
          f"relative error against float64 {rel:.3e}")
    assert rel <= 32 * EPS
    assert ((per_part.cpu() < 0.01) == d["below"]).all()
    want = np.array([2, 1], np.float32) / np.float32(3)  # slots below the threshold: (0,0), (0,2) and (1,1)
    np.testing.assert_array_equal(got["part_acc"].cpu().numpy(), want)
    ok, n = eval_ref.part_acc_counts(ref, d["valids"])
    assert ok.tolist() == [2, 1] and n.tolist() == [3, 3]  # the restatement counts the same
    _check_trans(got, d)


# ---- c. hard rotations, one part per sample ------------------------------------------------------------------------------------
def _axis_angle(axis, deg):
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    h = math.radians(deg) / 2
    return torch.cat([torch.tensor([math.cos(h)], dtype=torch.float64), math.sin(h) * a]).float()


S45 = math.sin(math.radians(45.0))
POLE = torch.tensor([S45, 0.0, S45, 0.0])  # (cos 45, 0, sin 45, 0): 2 (w y - x z) = 0.99999997 in float64
GENERIC = _axis_angle([0.3, -0.5, 0.8], 40.0)
GENERIC2 = _axis_angle([-0.6, 0.2, 0.5], 75.0)

QUAT_CASES = [  # name, predicted, ground truth (float32 quaternions; nothing is normalised)
    ("pole", POLE, GENERIC),
    ("pole as ground truth", GENERIC2, POLE),
    ("pole x 1.001 (clamped)", POLE * 1.001, GENERIC),
    ("negative pole x 1.001 (clamped)", torch.tensor([S45, 0.0, -S45, 0.0]) * 1.001, GENERIC),
    ("pole + 1e-4 in x and z", POLE + torch.tensor([0.0, 1e-4, 0.0, 1e-4]), GENERIC),
    ("+-179 deg about x (wrap)", torch.tensor([math.cos(math.radians(89.5)), math.sin(math.radians(89.5)), 0.0, 0.0]),
     torch.tensor([-math.cos(math.radians(89.5)), math.sin(math.radians(89.5)), 0.0, 0.0])),
    ("q against -q", GENERIC2, -GENERIC2),
    ("norms 0.6 and 1.7", GENERIC * 0.6, GENERIC2 * 1.7),
    ("negative w", -GENERIC, GENERIC2),
    ("identity", torch.tensor([1.0, 0, 0, 0]), torch.tensor([1.0, 0, 0, 0])),
]

_M = lambda q: quat_to_matrix(q)
# (No pole among the matrices: there |w| = |y| and |x| = |z|, so two candidates of matrix_to_quaternion always tie.)
RMAT_CASES = [  # name, predicted, ground truth (float32 matrices from quat_to_matrix)
    ("180 deg about x (candidate 1)", _M(_axis_angle([1, 0, 0], 180.0)), _M(GENERIC)),
    ("180 deg about y (candidate 2)", _M(_axis_angle([0, 1, 0], 180.0)), _M(GENERIC)),
    ("180 deg about z (candidate 3)", _M(_axis_angle([0, 0, 1], 180.0)), _M(GENERIC)),
    ("179.9 deg", _M(_axis_angle([0.8, 0.5, 0.33], 179.9)), _M(GENERIC2)),
    ("generic 40 deg (candidate 0)", _M(GENERIC), _M(GENERIC2)),
    ("0.3 R", 0.3 * _M(GENERIC), _M(GENERIC2)),
    ("all-zero matrix (norm 0.5 -> identity)", torch.zeros(3, 3), _M(GENERIC2)),
    ("identity", torch.eye(3), torch.eye(3)),
]


def hard_rotation_batch(kind, dev):
    cases = QUAT_CASES if kind == "quat" else RMAT_CASES
    B, N = len(cases), 8
    g = torch.Generator().manual_seed(6100)
    pts = torch.randn(B, 1, N, 3, generator=g) * 0.2
    gt_t = torch.randn(B, 1, 3, generator=g) * 0.3
    pr_t = gt_t + 0.05 * torch.randn(B, 1, 3, generator=g)
    pr = torch.stack([c[1] for c in cases])[:, None].to(dev)
    gt = torch.stack([c[2] for c in cases])[:, None].to(dev)
    return dict(pts=pts.to(dev), valids=torch.ones(B, 1, device=dev), gt_t=gt_t.to(dev), pr_t=pr_t.to(dev),
                pr_r=Rotation3D(pr, kind), gt_r=Rotation3D(gt, kind), names=[c[0] for c in cases])


def check_hard_rotation_conditions(d, kind):
    """What each case is there for, asserted on the float64 reference values of the tensors the kernel receives."""
    names = d["names"]
    at = lambda s: next(i for i, n in enumerate(names) if n.startswith(s))
    pr, gt = d["pr_r"].rot[:, 0], d["gt_r"].rot[:, 0]
    qp, qg = eval_ref.to_quat(pr, kind), eval_ref.to_quat(gt, kind)
    arg = lambda q: 2 * (q[:, 0] * q[:, 2] - q[:, 1] * q[:, 3])  # the argument of asin
    ref = eval_ref.rot_metrics(pr[:, None], gt[:, None], kind, d["valids"])
    assert float(ref["mae"][at("identity")]) == 0.0
    if kind == "quat":
        assert torch.equal(eval_ref.f64(pr), torch.stack([c[1] for c in QUAT_CASES]).double())  # no case was sanitised away
        assert 1 - 1e-6 < float(arg(qp)[at("pole")]) < 1 and 1 - 1e-6 < float(arg(qg)[at("pole as")]) < 1  # on the inside
        assert float(arg(qp)[at("pole x 1.001")]) > 1.001 and float(arg(qp)[at("negative pole")]) < -1.001  # the clamp is taken
        assert 0.999 < float(arg(qp)[at("pole + 1e-4")]) < 1 - 1e-9
        i = at("+-179")
        ex = eval_ref.euler_zyx_deg(torch.stack([qp[i], qg[i]]))[:, 0]
        assert float((ex[0] - ex[1]).abs()) > 357.9  # 360 - d is taken ...
        np.testing.assert_allclose(float(ref["mae"][i]), 2.0 / 3.0, rtol=1e-6)  # ... and 358 deg wraps to 2 deg
        assert float(ref["mse"][at("q against")]) == 0.0
        norms = eval_ref.f64(torch.stack([pr[at("norms")], gt[at("norms")]])).norm(dim=-1)
        np.testing.assert_allclose(norms.numpy(), [0.6, 1.7], rtol=1e-6)
        assert float(qp[at("negative w"), 0]) < -0.5
        return
    # no arg-max tie decides a case: the two largest candidate magnitudes of every matrix differ by at least 1e-3.  The
    # all-zero matrix is the one exception (all four are 1): each of its candidates is a quaternion of norm 0.5, which the
    # constructor rule replaces by the identity whichever is taken.
    zero = at("all-zero")
    for side in (pr, gt):
        top = eval_ref.matrix_candidates(side).sort(-1, descending=True)[0]
        gap = top[:, 0] - top[:, 1]
        assert float(gap[[i for i in range(len(names)) if not (side is pr and i == zero)]].min()) >= 1e-3
    picks = eval_ref.matrix_candidates(pr).argmax(-1).tolist()
    assert [picks[at(s)] for s in ("180 deg about x", "180 deg about y", "180 deg about z", "generic 40")] == [1, 2, 3, 0]
    assert set(picks) == {0, 1, 2, 3}
    assert qp[zero].tolist() == [1.0, 0.0, 0.0, 0.0]  # the constructor rule fires here ...
    raw = eval_ref.rotation.matrix_to_quaternion(eval_ref.f64(pr))
    assert float(raw[zero].norm()) == 0.5
    # ... and nowhere else: sum_k s_k = 4 puts the chosen component at >= 0.5, so a scaled rotation keeps its quaternion
    others = [i for i in range(len(names)) if i != zero]
    assert float(raw[others].norm(dim=-1).min()) > 0.5 and torch.equal(qp[others], raw[others])
    assert float(raw[at("0.3 R")].norm()) < 0.9  # (not a unit quaternion either)


@pytest.mark.parametrize("kind", KINDS)
def test_hard_rotations(cuda_device, kind):
    """Measured on an MI355X: see the LABBOOK entry on these tests for the errors in ulp per case."""
    d = hard_rotation_batch(kind, cuda_device)
    check_hard_rotation_conditions(d, kind)
    got = _fused(d)
    ulps = _check_rot(got, d, kind)
    for i, name in enumerate(d["names"]):
        print(f"{kind} / {name}: error against float64 in ulp (mse, rmse, mae): kernel "
              + ", ".join(f"{ulps[m][0][i]:.2f}" for m in METRICS) + "; composition "
              + ", ".join(f"{ulps[m][1][i]:.2f}" for m in METRICS))
    print(f"{kind}: worst kernel error {max(float(ulps[m][0].max()) for m in METRICS):.2f} ulp, worst composition error "
          f"{max(float(ulps[m][1].max()) for m in METRICS):.2f} ulp")
    _check_trans(got, d)
    assert _bits_equal(got, _fused(d))


# ---- d. batch reduction --------------------------------------------------------------------------------------------------------
def reduction_batch(B, P, N, kind, dev):
    """`valids` with every kind of entry: sample B - 2 has no valid part (with B = 37 its rows sit on both sides of the
    boundary between the two blocks of batch_metrics_kernel: 7 * 37 = 259 threads), samples 1 and 4 mod 7 carry a 0.5
    and a 2.0, sample 2 mod 7 a padded slot (where P > 1)."""
    valids = torch.ones(B, P)
    for b in range(B):
        if b % 7 == 1:
            valids[b, 0] = 0.5
        elif b % 7 == 4:
            valids[b, P - 1] = 2.0
        elif b % 7 == 2 and P > 1:
            valids[b, P - 1] = 0.0
    valids[B - 2] = 0.0
    d = _random_batch(B, P, N, 7000 + B, kind, dev, valids)
    d["empty"] = B - 2
    return d


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,P,N", [(37, 2, 8), (300, 1, 4)])
def test_batch_reduction_and_valids_values(cuda_device, B, P, N, kind):
    d = reduction_batch(B, P, N, kind, cuda_device)
    v = d["valids"].cpu()
    assert (v == 0.5).any() and (v == 2.0).any() and 7 * B > 256
    got, per_part = _fused(d, per_part=True)
    e = d["empty"]
    for k in eval_utils.METRIC_KEYS:  # no valid part: 0 / 0 in all seven outputs, as the composition gives
        assert math.isnan(float(got[k][e])), k
    a, b = _posed(d)
    ref = eval_ref.chamfer_per_part(a.cpu(), b.cpu())
    ok, n = _check_part_acc(got, ref, v)  # counts valids == 1 only; NaN where there is none
    assert int((n == 0).sum()) >= 1 and 0 < int(ok.sum()) < int(n.sum())
    _check_trans(got, d)  # the six means weight by the value of valids
    _check_rot(got, d, kind)
    finite = torch.ones(B, dtype=torch.bool)
    finite[e] = False
    for m in METRICS:
        assert torch.isfinite(got[f"trans_{m}"].cpu()[finite]).all() and torch.isfinite(got[f"rot_{m}"].cpu()[finite]).all()

    comp = eval_utils._assembly_metrics_composed(d["pts"], d["pr_t"], d["gt_t"], d["pr_r"], d["gt_r"], d["valids"])
    np.testing.assert_array_equal(got["part_acc"].cpu().numpy(), comp["part_acc"].cpu().numpy())  # (NaN equals NaN here)
    for m in METRICS:
        np.testing.assert_allclose(got[f"trans_{m}"].cpu().numpy(), comp[f"trans_{m}"].cpu().numpy(), rtol=1e-5, atol=0.0,
                                   equal_nan=True, err_msg=m)
        assert torch.equal(torch.isnan(got[f"rot_{m}"]), torch.isnan(comp[f"rot_{m}"])), m

    # the neighbours of the empty sample are unaffected by it: the same batch with that sample made valid
    f = dict(d)
    f["valids"] = d["valids"].clone()
    f["valids"][e] = 1.0
    other = _fused(f)
    for k in eval_utils.METRIC_KEYS:
        assert torch.equal(got[k].cpu()[finite].view(torch.int32), other[k].cpu()[finite].view(torch.int32)), k
        assert math.isfinite(float(other[k][e])), k


# ---- e. connectivity ------------------------------------------------------------------------------------------------------------
FLAGS = torch.tensor([0.0, 0.5, 1.0, 2.0])
CONTACT_SHAPES = {(1, 1): 8101, (2, 3): 8201, (3, 7): 8301, (5, 15): 8401, (4, 20): 8501}  # (B, P): seed; B P P = 1 ... 1600


def contact_batch(B, P, seed, flags=FLAGS):
    """Random flags from `flags` (independently for [b, i, j] and [b, j, i]), contact coordinates and poses scaled so that
    about half of the contacts come closer than 0.01."""
    g = torch.Generator().manual_seed(seed)
    contact = torch.zeros(B, P, P, 4)
    contact[..., 0] = flags[torch.randint(0, len(flags), (B, P, P), generator=g)]
    if B * P * P == 1:
        contact[..., 0] = 1.0
    contact[..., 1:] = torch.randn(B, P, P, 3, generator=g) * 0.12
    trans = torch.randn(B, P, 3, generator=g) * 0.03
    q = F.normalize(torch.randn(B, P, 4, generator=g), dim=-1)
    return contact, trans, q


def _connectivity(contact, trans, q, kind, dev):
    rot = Rotation3D(q.to(dev)) if kind == "quat" else Rotation3D(quat_to_matrix(q).to(dev), "rmat")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = eval_utils.calc_connectivity_acc(trans.to(dev), rot, contact.to(dev), fused=True)
    return got, rot


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,P", list(CONTACT_SHAPES))
def test_connectivity_flags_and_sizes(cuda_device, B, P, kind):
    contact, trans, q = contact_batch(B, P, CONTACT_SHAPES[(B, P)])
    flag = contact[..., 0]
    if P > 1:
        assert ((flag == 1) & (flag.transpose(1, 2) != 1)).any()  # asymmetric: [b, i, j] set, [b, j, i] not
        assert (flag == 0.5).any() and (flag == 2.0).any() and (flag == 0.0).any()
    got, rot = _connectivity(contact, trans, q, kind, cuda_device)
    hits, contacts, dist = eval_ref.connectivity(trans, rot.rot, kind, contact)
    assert contacts == int((flag == 1).sum()) >= 1
    # float32 posing and distances move a value of 0.01 by ~1e-6 relative; nothing lies within 1e-3 of the threshold
    assert eval_ref.threshold_margin(dist) > 1e-3
    if contacts >= 10:
        assert 0.25 <= hits / contacts <= 0.75  # the threshold decides something
    print(f"B={B} P={P} {kind}: {hits} of {contacts} contacts hit, margin {eval_ref.threshold_margin(dist):.2e}")
    assert got.shape == (B,) and got.dtype == torch.float32
    np.testing.assert_array_equal(got.cpu().numpy(), np.full(B, eval_ref.ratio32(hits, contacts)))
    again, _ = _connectivity(contact, trans, q, kind, cuda_device)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))


@pytest.mark.parametrize("kind", KINDS)
def test_connectivity_without_a_flag_of_exactly_one_is_nan(cuda_device, kind):
    contact, trans, q = contact_batch(3, 7, 8601, flags=torch.tensor([0.0, 0.5, 2.0]))
    assert not (contact[..., 0] == 1).any() and (contact[..., 0] != 0).any()
    got, _ = _connectivity(contact, trans, q, kind, cuda_device)
    assert got.shape == (3,) and torch.isnan(got).all()  # 0 / 0, as the composition gives


@pytest.mark.parametrize("kind", KINDS)
def test_connectivity_one_hit_and_one_miss_is_a_half(cuda_device, kind):
    """Identity poses: contact (0, 0, 1) pairs a point with itself (distance 0); contact (0, 0, 2) pairs (0.1, 0.1, 0.1) with
    (0.5, 0.5, 0.5), whose sign-flipped copies stay 3 * 0.4^2 = 0.48 apart.  Neither mirrored flag is set."""
    B, P = 2, 3
    contact = torch.zeros(B, P, P, 4)
    contact[0, 0, 1] = torch.tensor([1.0, 0.1, 0.1, 0.1])
    contact[0, 1, 0] = torch.tensor([0.5, 0.1, 0.1, 0.1])
    contact[0, 0, 2] = torch.tensor([1.0, 0.1, 0.1, 0.1])
    contact[0, 2, 0] = torch.tensor([2.0, 0.5, 0.5, 0.5])
    trans, q = torch.zeros(B, P, 3), torch.tensor([1.0, 0, 0, 0]).repeat(B, P, 1)
    got, rot = _connectivity(contact, trans, q, kind, cuda_device)
    hits, contacts, dist = eval_ref.connectivity(trans, rot.rot, kind, contact)
    assert (hits, contacts) == (1, 2) and dist[0] == 0.0 and abs(float(dist[1]) - 0.48) < 1e-6
    assert got.tolist() == [0.5, 0.5]


# ---- f. the wrapper's input forms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_wrapper_input_forms_give_the_same_bits(cuda_device, kind):
    B, P, N = 3, 4, 37
    valids = torch.ones(B, P)
    valids[0, 3] = valids[2, 2] = 0.0
    d = _random_batch(B, P, N, 9100, kind, cuda_device, valids)
    base, base_pp = _fused(d, per_part=True)

    def same(**changed):
        got, pp = _fused({**d, **changed}, per_part=True)
        return _bits_equal(base, got) and torch.equal(base_pp.view(torch.int32), pp.view(torch.int32))

    transposed = d["pts"].transpose(1, 2).contiguous().transpose(1, 2)  # [B, P, N, 3] view of a [B, N, P, 3] tensor
    assert not transposed.is_contiguous() and torch.equal(transposed, d["pts"])
    assert same(pts=transposed)
    wide = torch.full((B, P, N + 5, 4), 1e3, device=cuda_device)
    wide[:, :, 2:N + 2, :3] = d["pts"]
    sliced = wide[:, :, 2:N + 2, :3]  # a slice of a larger tensor
    assert not sliced.is_contiguous()
    assert same(pts=sliced)
    assert same(valids=d["valids"].bool())
    assert same(valids=d["valids"].double())
    assert same(pr_t=d["pr_t"].double(), gt_t=d["gt_t"].double())
    strided = d["valids"].t().contiguous().t()
    assert not strided.is_contiguous()
    assert same(valids=strided)


@pytest.mark.parametrize("kind", KINDS)
def test_workspace_size_and_a_nan_filled_workspace_leaves_no_trace(cuda_device, kind):
    """Every workspace entry the second kernel reads is written by the first, padded slots included (a NaN left in one
    would come through `value * valids` even at valids == 0)."""
    B, P, N = 3, 4, 37
    valids = torch.ones(B, P)
    valids[0, 3] = valids[2, 2] = 0.0
    d = _random_batch(B, P, N, 9100, kind, cuda_device, valids)
    base, base_pp = _fused(d, per_part=True)
    L = _lib.lib()
    nbytes = ctypes.c_int64()
    for b, p in ((B, P), (1, 1), (37, 2), (300, 20)):
        _lib.check(L.mpa_assembly_metrics_workspace(b, p, ctypes.byref(nbytes)), "mpa_assembly_metrics_workspace")
        assert nbytes.value == 56 * b * p  # 7 rows of float64 per part slot
    _lib.check(L.mpa_assembly_metrics_workspace(B, P, ctypes.byref(nbytes)), "mpa_assembly_metrics_workspace")
    nan = float("nan")
    ws = torch.full((nbytes.value // 8 + 16,), nan, dtype=torch.float64, device=cuda_device)
    out = torch.full((len(eval_utils.METRIC_KEYS), B), nan, dtype=torch.float32, device=cuda_device)
    per_part = torch.full((B, P), nan, dtype=torch.float32, device=cuda_device)
    args = [t.contiguous() for t in (d["pts"], d["pr_t"], d["gt_t"], d["pr_r"].rot, d["gt_r"].rot, d["valids"])]
    fn = L.mpa_assembly_metrics_rmat if kind == "rmat" else L.mpa_assembly_metrics
    with torch.cuda.device(cuda_device):
        st = fn(*[_lib.ptr(a) for a in args], B, P, N, _lib.ptr(ws), _lib.ptr(out), _lib.ptr(per_part),
                _lib.current_stream(cuda_device))
    _lib.check(st, "mpa_assembly_metrics")
    torch.cuda.synchronize(cuda_device)
    for i, k in enumerate(eval_utils.METRIC_KEYS):
        assert torch.isfinite(out[i]).all(), k
        assert torch.equal(out[i].view(torch.int32), base[k].view(torch.int32)), k
    assert torch.equal(per_part.view(torch.int32), base_pp.view(torch.int32))
    used = nbytes.value // 8
    assert torch.isfinite(ws[:used]).all() and torch.isnan(ws[used:]).all()  # all of it written, nothing beyond it
