"""The backward of the fused assembly loss (csrc/assembly_loss.hip: assembly_backward_kernel, assembly_backward_mat_kernel<9>,
assembly_backward_finish_kernel) against the float64 evaluation of tests/assembly_loss_ref.py with the nearest-neighbour
selections held to the HIP path's own, under the bars of tests/anchored.py.

Per case: forward and backward through the C ABI on poisoned workspaces (tests/assembly_loss_hip.py), the four arg-min
arrays read from the head of the int workspace, the pinned reference on the CPU in float32 and in float64 with those arrays, and
anchored.check over `gq.b<k>` / `gt.b<k>` of every sample and the five loss terms — per sample, so that a sample with a
large gradient cannot hide another; in cases H and I the row of the special part is a tensor of its own.  Nothing in a bar
comes from the HIP path.  A pinned comparison would accept a search that picks the wrong neighbour, so wherever
B P N <= 20 000 the float64 exhaustive scan runs on the CPU and at most 1e-3 of the valid queries may select differently.

The cases (R.CASES; the smallest shapes at which each path can go wrong):

  A  quat  N below a wave / a block, the unrolled scan's clamp at P = 3, 5, 7; non-prefix masks, a single-part sample
  B  quat  the last unsliced size (N = 896), the first sliced one (897 = 4 x 224 + 1), uneven slices
  C  rmat  S = 1 / 2 / 4 on both sides of N = 896 | 897 and 1920 | 1921; N = 2049 above the leaf limit
  D  both  P = 1, 2, 63, 64 (about 40 valid parts, non-prefix)
  E  both  training = False: the eval normalisation, unsliced and sliced
  F  both  every search route (R.ROUTE_CASES): gradients and posed clouds bit-equal across routes
  G  quat  dot < 0 and dot == 0 in the closed-form rotation term; zeroed term weights
  H  both  a padded slot that is somebody's nearest neighbour (branch C with valid == false), unsliced and sliced
  I  quat  a part whose stored indices are all -1
  J  both  a sample without a valid part: its gradients are exactly zero (include/mpa_hip.h)

Case I squares a translation of 1e20: `trans_loss` of that sample is 1e40, +inf in any float32 evaluation; it is asserted to
be +inf and left out of the relative comparison (`Case.overflow`), its gradient 2e20 / nv is compared like every other.  The
N stored distances of 1e32 make that sample's `transform_pt_cd_loss` about 2.5e31: the term is compared one sample at a time
there (`Case.per_sample`).

Measured on one MI355X (LABBOOK 2026-10-20, fourth entry): worst deviation from float64 4.0e-7 where the float32 reference
has the same; at most 3.21 of the 8 x max(e32, median e32) the bars allow; 0 differing arg-mins; 40 tests in 3 s.
"""
import pytest
import torch

import anchored as A
import assembly_loss_hip as H
import assembly_loss_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _at_most_16_threads():
    old = torch.get_num_threads()
    torch.set_num_threads(min(16, old))
    yield
    torch.set_num_threads(old)


def _say(capsys, text):
    with capsys.disabled():
        print("\n  " + text, end="")


def _anchor(case, batch, go, rows, hip, capsys, label=None, samples=None):
    """anchored.assert_anchored of the HIP outputs against the pinned reference on the HIP path's own arg-mins."""
    pick = (lambda t: t) if samples is None else (lambda t: t[samples])
    kw = {"rows": rows, "samples": samples, "overflow": case.overflow, "per_sample": case.per_sample}
    r64 = R.tensors(*R.run(batch, hip["idx"], go, case.rot_type, case.training, torch.float64, samples=samples), **kw)
    r32 = R.tensors(*R.run(batch, hip["idx"], go, case.rot_type, case.training, torch.float32, samples=samples), **kw)
    got = R.tensors(hip["losses"] if samples is None else hip["losses"][:, samples], pick(hip["grad_rot"]),
                    pick(hip["grad_trans"]), **kw)
    A.assert_anchored(got, r32, r64, label or case.id, capsys)


def _pin(case, batch, hip, capsys):
    B, P, N = case.shape
    if B * P * N > R.PIN_SCAN_LIMIT:
        return
    diff, total = R.pin_disagreement(batch, hip["idx"], case.rot_type)
    _say(capsys, f"{case.id}: {diff} of {total} valid queries select another target than the float64 exhaustive scan")
    assert diff <= R.PIN_SHARE * total, (diff, total)


def _finite(hip):
    assert bool(torch.isfinite(hip["grad_rot"]).all()) and bool(torch.isfinite(hip["grad_trans"]).all())


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_loss_backward_is_anchored(cuda_device, capsys, case):
    batch, go, rows = case.build()
    B, P, N = case.shape
    v = batch["valids"] > 0
    hip = H.hip_run(batch, go, case.rot_type, case.training, "grid", cuda_device)
    _finite(hip)
    samples = None
    if case.kind == "padnear":  # not vacuous: a valid GT point's nearest predicted point is the padded slot's fill point
        for b, pad in rows:
            hits = int(((hip["idx"][3][b] // N == pad) & v[b][:, None]).sum())
            _say(capsys, f"{case.id}: sample {b}: {hits} GT points have the padded slot {pad} as nearest neighbour")
            assert hits >= 1
    elif case.kind == "far":
        (b, p), = rows
        assert bool((hip["idx"][2][b, p] == -1).all())
        for term, k in case.overflow:  # the squared 1e20 translation: +inf in float32
            assert hip["losses"][term, k] == float("inf")
    elif case.kind == "empty":
        e = R.EMPTY_SAMPLE
        assert not v[e].any()
        assert bool((hip["grad_rot"][e] == 0).all()) and bool((hip["grad_trans"][e] == 0).all())
        # its loss terms as include/mpa_hip.h documents them (and as the reference gives them): the valid means are 0 / 0; the
        # whole-shape term divides by P N in training, by the valid count in evaluation
        r32 = R.run(batch, hip["idx"], go, case.rot_type, case.training, torch.float32)[0][:, e]
        for i, name in enumerate(R.LOSS_TERMS):
            want_zero = case.training and name == "transform_pt_cd_loss"
            got_e = float(hip["losses"][i, e])
            assert (got_e == 0.0) if want_zero else (got_e != got_e), (name, got_e)
            assert (float(r32[i]) == 0.0) if want_zero else bool(torch.isnan(r32[i])), (name, float(r32[i]))
        samples = [b for b in range(B) if b != e]
    # padded slots that nobody selects take exactly no gradient
    unhit = ~v
    for b, pad in (rows if case.kind == "padnear" else ()):
        unhit[b, pad] = False
    assert bool((hip["grad_rot"][unhit] == 0).all()) and bool((hip["grad_trans"][unhit] == 0).all())
    _anchor(case, batch, go, rows, hip, capsys, samples=samples)
    _pin(case, batch, hip, capsys)


@pytest.mark.parametrize("case", R.ROUTE_CASES, ids=lambda c: c.id)
def test_loss_backward_behind_every_search_route(cuda_device, capsys, monkeypatch, case):
    """The backward reads the four posed clouds by index: behind the leaf pose kernel (k-d order) and the per-sample auto
    route they must be in original point order all the same.  Every route is anchored, and the gradients and the clouds
    of the valid parts (slots R1 / R2 / S1 / S2 of the float workspace) are bit-equal across routes."""
    batch, go, rows = case.build()
    v = batch["valids"] > 0
    first = case.shape == R.ROUTE_CASES[0].shape
    routes = [(r, None) for r in R.ROUTES]
    if first:  # the per-part term on the gated search and on the scan / leaves of the route
        routes = [(r, part) for r in R.ROUTES for part in ("gate", "scan")]
    base = None
    for route, part in routes:
        if part is not None:
            monkeypatch.setenv("MPA_PART_SEARCH", part)
        hip = H.hip_run(batch, go, case.rot_type, case.training, route, cuda_device)
        _finite(hip)
        if base is None:
            base = hip
            _anchor(case, batch, go, rows, hip, capsys, label=f"{case.id} {route}/{part}")
            _pin(case, batch, hip, capsys)
            continue
        for k in range(4):
            assert torch.equal(hip["idx"][k][v], base["idx"][k][v]), (route, part, k)
            assert torch.equal(hip["clouds"][k][v], base["clouds"][k][v]), (route, part, k)
        assert torch.equal(hip["grad_rot"], base["grad_rot"]) and torch.equal(hip["grad_trans"], base["grad_trans"]), (route, part)
    monkeypatch.delenv("MPA_PART_SEARCH", raising=False)


@pytest.mark.parametrize("rot_type,shape", [("quat", (2, 4, 897)), ("rmat", (2, 2, 1923))])
def test_wrapper_gives_the_bits_of_the_raw_calls(cuda_device, monkeypatch, rot_type, shape):
    """`geometric_assembly_loss` followed by autograd against the raw forward + backward calls."""
    from multi_part_assembly_amd.loss import LOSS_TERMS, geometric_assembly_loss
    from multi_part_assembly_amd.rotation import Rotation3D
    monkeypatch.delenv("MPA_SHAPE_SEARCH", raising=False)
    case = next(c for c in R.CASES if c.rot_type == rot_type and c.shape == shape)
    batch, go, _ = case.build()
    hip = H.hip_run(batch, go, rot_type, True, "grid", cuda_device)
    d = lambda k: batch[k].to(cuda_device)
    rp, tp = d("rot_pred").requires_grad_(), d("trans_pred").requires_grad_()
    terms, _ = geometric_assembly_loss(d("pcs"), tp, Rotation3D(rp, rot_type), d("trans_gt"), Rotation3D(d("rot_gt"), rot_type),
                                       d("valids"), training=True, search="grid")
    losses = torch.stack([terms[k] for k in LOSS_TERMS])
    (losses * go.to(cuda_device)).sum().backward()
    assert torch.equal(losses.detach().cpu(), hip["losses"])
    assert torch.equal(rp.grad.cpu(), hip["grad_rot"]) and torch.equal(tp.grad.cpu(), hip["grad_trans"])
