"""CPU checks of the PointNet++ feature-propagation operators and of the modules built on them: the numpy restatement
(`three_nn`, `three_interpolate`, `three_interpolate_backward` of multi_part_assembly_amd/pointnet2_ref.py) against
independent formulations of the definitions in include/mpa_hip.h, the C boundary of csrc/pointnet2_interp.hip (symbols,
argument refusals, the workspace query), the host path of the wrappers, and `PointnetFPModule`, `PointnetSAModuleMSG` and
`PointNet2MSG` against tests/golden/pointnet2_fp_msg.npz, the record of the reference's own modules run over this package's
operator module (tests/golden/make_golden_pointnet2_fp_msg.py) — nothing here launches a kernel."""
import copy
import ctypes
import sys
import warnings

import numpy as np
import pytest
import torch

import anchored
from conftest import GOLDEN
from multi_part_assembly_amd import _build, _lib, pointnet2_ref as ref, pointnet2_utils as pu
from multi_part_assembly_amd.pointnet2 import (PointNet2MSG, PointNet2SSG, PointnetFPModule, PointnetSAModule,
                                               PointnetSAModuleMSG)

sys.path.insert(0, str(GOLDEN))
import param_fill  # noqa: E402

f32 = np.float32
U = 2.0 ** -24
REL = 1e-5


def cloud_pair(kind, M, n, m, seed):
    """(unknown [M, n, 3], known [M, m, 3]) float32."""
    rng = np.random.RandomState(seed)
    if kind == "random":
        return rng.rand(M, n, 3).astype(f32) - f32(0.5), rng.rand(M, m, 3).astype(f32) - f32(0.5)
    if kind == "lattice":                                   # 27 sites: nearly every choice is decided by the tie rule
        return ((rng.randint(1, 4, size=(M, n, 3)) * f32(0.25)).astype(f32),
                (rng.randint(1, 4, size=(M, m, 3)) * f32(0.25)).astype(f32))
    if kind == "duplicated":                                # every known point twice (once, for the odd one out)
        k = rng.rand(M, m, 3).astype(f32) - f32(0.5)
        k[:, m // 2:] = k[:, :m - m // 2]
        return rng.rand(M, n, 3).astype(f32) - f32(0.5), k
    if kind == "same":                                      # unknown = known (cycled): zero distances
        k = rng.rand(M, m, 3).astype(f32) - f32(0.5)
        return np.ascontiguousarray(k[:, np.arange(n) % m]), k
    raise ValueError(kind)


KINDS = ("random", "lattice", "duplicated", "same")


def sq_dist(unknown, known):
    """d [M, n, m] in the dtype of the inputs, the definition's expression."""
    u, k = unknown[:, :, None, :], known[:, None, :, :]
    return ((u[..., 0] - k[..., 0]) * (u[..., 0] - k[..., 0]) + (u[..., 1] - k[..., 1]) * (u[..., 1] - k[..., 1])) \
        + (u[..., 2] - k[..., 2]) * (u[..., 2] - k[..., 2])


# ---- three_nn ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_three_nn_equals_a_stable_sort_of_the_same_distances(kind):
    for s, (n, m) in enumerate(((1, 3), (7, 5), (40, 12), (65, 130))):
        unknown, known = cloud_pair(kind, 2, n, m, 10 + s)
        dist, idx = ref.three_nn(unknown, known)
        assert dist.dtype == f32 and idx.dtype == np.int32 and dist.shape == idx.shape == (2, n, 3)
        d = sq_dist(unknown, known)
        assert d.dtype == f32
        order = np.argsort(d, axis=2, kind="stable")[..., :3]
        assert np.array_equal(idx, order), (kind, n, m)
        assert np.array_equal(dist, np.sqrt(np.take_along_axis(d, order, axis=2)))
        if kind in ("lattice", "duplicated") and m >= 12:
            assert (dist[..., 0] == dist[..., 1]).any()                      # ties were decided
            assert (idx[..., 0] < idx[..., 1])[dist[..., 0] == dist[..., 1]].all()
    d64, i64 = ref.three_nn(unknown.astype(np.float64), known.astype(np.float64))
    assert d64.dtype == np.float64 and i64.dtype == np.int32
    assert np.array_equal(i64, np.argsort(sq_dist(unknown.astype(np.float64), known.astype(np.float64)), axis=2,
                                          kind="stable")[..., :3])


def test_three_nn_with_fewer_than_three_known_points_and_with_nan():
    unknown, known = cloud_pair("random", 2, 9, 3, 1)
    for m in (1, 2, 3):
        dist, idx = ref.three_nn(unknown, known[:, :m])
        d = np.sqrt(np.sort(sq_dist(unknown, known[:, :m]), axis=2))
        assert np.array_equal(dist[..., :m], d)
        assert np.isinf(dist[..., m:]).all() and (dist[..., m:] > 0).all() and not idx[..., m:].any()
    unknown, known = cloud_pair("random", 2, 30, 8, 2)
    known[0, 2], known[1, 0, 1], known[1, 7] = np.nan, np.nan, np.nan
    dist, idx = ref.three_nn(unknown, known)
    assert not np.isin(idx[0], [2]).any() and not np.isin(idx[1], [0, 7]).any()
    assert np.isfinite(dist).all()
    clean = np.delete(known[0], 2, axis=0)[None]                              # the scan without the point: the same bests
    assert np.array_equal(ref.three_nn(unknown[:1], clean)[0], dist[:1])
    known[:] = np.nan                                                         # nothing is ever inserted
    dist, idx = ref.three_nn(unknown, known)
    assert np.isinf(dist).all() and not idx.any()


# ---- three_interpolate -------------------------------------------------------------------------------------------------
def interp_case(M, C, m, n, seed, out_of_range=False):
    rng = np.random.RandomState(seed)
    feat = (rng.randn(M, C, m) * 10.0 ** rng.randint(-2, 3, size=(M, C, 1))).astype(f32)
    idx = rng.randint(0, m, size=(M, n, 3)).astype(np.int32)
    if m > 2:
        idx[idx == m - 1] = 0                                # known point m - 1: no referrer
        idx[idx == m - 2] = 1
        idx[0, n - 1, 2] = m - 2                             # known point m - 2 of cloud 0: one referrer
    if M > 1:
        idx[1] = min(1, m - 1)                               # one known point named 3 n times
    w = rng.rand(M, n, 3).astype(f32)
    w = (w / w.sum(axis=2, keepdims=True)).astype(f32)
    g = (rng.randn(M, C, n) * 10.0 ** rng.randint(-2, 3, size=(M, 1, n))).astype(f32)
    if out_of_range:
        flat = idx.reshape(-1)
        flat[::7] = np.array([-1, m, 2 ** 31 - 1, -2 ** 31, m + 100000], dtype=np.int64)[np.arange(len(flat[::7])) % 5]
    return feat, idx, w, g


def test_three_interpolate_is_three_products_and_two_sums_within_one_rounding_each():
    for s, (M, C, m, n) in enumerate(((1, 1, 1, 1), (2, 5, 12, 40), (3, 7, 64, 33))):
        feat, idx, w, _ = interp_case(M, C, m, n, s)
        out = ref.three_interpolate(feat, idx, w)
        assert out.dtype == f32 and out.shape == (M, C, n)
        f64 = np.take_along_axis(feat.astype(np.float64)[:, :, None, :], idx.astype(np.int64).reshape(M, 1, 1, -1),
                                 axis=3).reshape(M, C, n, 3)
        terms = f64 * w.astype(np.float64)[:, None]
        exact = np.einsum("bcjk->bcj", terms)
        bound = 3 * U / (1 - 3 * U) * np.abs(terms).sum(-1)                   # a product and two sums on every term
        assert np.all(np.abs(out.astype(np.float64) - exact) <= bound)
        t = (np.take_along_axis(feat[:, :, None, :], idx.astype(np.int64).reshape(M, 1, 1, -1), axis=3).reshape(M, C, n, 3)
             * w[:, None]).astype(f32)
        assert np.array_equal(out, (t[..., 0] + t[..., 1]) + t[..., 2])        # the written order, operation by operation
        o64 = ref.three_interpolate(feat.astype(np.float64), idx, w.astype(np.float64))
        assert o64.dtype == np.float64 and np.all(np.abs(o64 - exact) <= 4 * 2.0 ** -53 * np.abs(terms).sum(-1))


def test_three_interpolate_backward_is_a_sequential_sum_within_its_bound():
    """The bound of tests/test_pointnet2_ops.py: |fl(sum) - sum| <= L u sum|terms| for L terms added one after the other;
    the terms are the float32 products, each the correctly rounded product of its factors."""
    M, C, m, n = 2, 3, 11, 70
    feat, idx, w, g = interp_case(M, C, m, n, 4)
    got = ref.three_interpolate_backward(g, idx, w, m)
    assert got.dtype == f32 and got.shape == (M, C, m)
    terms = (np.repeat(g, 3, axis=2) * w.reshape(M, 1, -1)).astype(f32)       # [M, C, 3 n], position 3 j + k
    assert np.array_equal(terms, (np.repeat(g, 3, axis=2).astype(np.float64) * w.reshape(M, 1, -1).astype(np.float64)).astype(f32))
    flat = idx.reshape(M, -1)
    longest = 0
    for b in range(M):
        for i in range(m):
            sel = flat[b] == i
            L = int(sel.sum())
            longest = max(longest, L)
            t64 = terms[b][:, sel].astype(np.float64)
            assert np.all(np.abs(got[b, :, i].astype(np.float64) - t64.sum(axis=1)) <= L * U * np.abs(t64).sum(axis=1)), (b, i, L)
            seq = np.zeros(C, dtype=f32)
            for p in np.flatnonzero(sel):
                seq = seq + terms[b][:, p]
            assert np.array_equal(got[b, :, i], seq)
    assert longest == 3 * n and np.all(got[:, :, m - 1] == 0) and (flat[0] == m - 2).sum() == 1
    g64 = ref.three_interpolate_backward(g.astype(np.float64), idx, w.astype(np.float64), m)
    assert g64.dtype == np.float64 and np.allclose(g64, got, rtol=1e-4, atol=1e-4 * np.abs(got).max())


def test_out_of_range_indices_read_zero_and_contribute_nothing():
    M, C, m, n = 2, 4, 9, 25
    feat, idx, w, g = interp_case(M, C, m, n, 5, out_of_range=True)
    ok = (idx >= 0) & (idx < m)
    assert (~ok).sum() >= 5
    out = ref.three_interpolate(feat, idx, w)
    back = ref.three_interpolate_backward(g, idx, w, m)
    # the same call with those positions pointed at a zero column m of a padded cloud, and that column's sums dropped
    safe = np.where(ok, idx, m).astype(np.int32)
    padded = np.concatenate([feat, np.zeros((M, C, 1), dtype=f32)], axis=2)
    assert np.array_equal(out, ref.three_interpolate(padded, safe, w))
    assert np.array_equal(back, ref.three_interpolate_backward(g, safe, w, m + 1)[:, :, :m])
    none = np.full_like(idx, -5)
    assert not ref.three_interpolate(feat, none, w).any() and not ref.three_interpolate_backward(g, none, w, m).any()


def test_wrappers_run_the_restatement_on_host_tensors_and_differentiate():
    feat, idx, w, g = interp_case(2, 5, 12, 40, 6)
    unknown, known = cloud_pair("random", 2, 40, 12, 6)
    dist, nn_idx = pu.three_nn(torch.from_numpy(unknown).double().requires_grad_(), torch.from_numpy(known).requires_grad_())
    assert dist.dtype == torch.float32 and nn_idx.dtype == torch.int32            # cast to float32, as custom_fwd upstream
    assert not dist.requires_grad and not nn_idx.requires_grad
    want = ref.three_nn(unknown, known)
    assert np.array_equal(dist.numpy(), want[0]) and np.array_equal(nn_idx.numpy(), want[1])
    tf = torch.from_numpy(feat).requires_grad_()
    tw = torch.from_numpy(w).requires_grad_()
    out = pu.three_interpolate(tf, torch.from_numpy(idx), tw)
    assert np.array_equal(out.detach().numpy(), ref.three_interpolate(feat, idx, w))
    out.backward(torch.from_numpy(g))
    assert np.array_equal(tf.grad.numpy(), ref.three_interpolate_backward(g, idx, w, 12)) and tw.grad is None
    assert np.array_equal(pu.three_interpolate(tf, torch.from_numpy(idx).long(), tw.double()).detach().numpy(), out.detach().numpy())
    with pytest.raises(ValueError, match="three_nn"):
        pu.three_nn(torch.zeros(2, 4, 2), torch.zeros(2, 4, 3))
    with pytest.raises(ValueError, match="three_interpolate"):
        pu.three_interpolate(tf, torch.from_numpy(idx[:, :5]), tw)
    for name in ("three_nn", "three_interpolate", "ThreeNN", "ThreeInterpolate"):
        assert name in pu.__all__ and hasattr(pu, name)


# ---- the C boundary ----------------------------------------------------------------------------------------------------
NAMES = ["mpa_three_nn", "mpa_three_interpolate_forward", "mpa_three_interpolate_workspace", "mpa_three_interpolate_backward"]


@pytest.fixture(scope="module")
def L():
    _build.build()
    return _lib.lib()


def test_symbols_are_declared_on_both_sides_and_the_version_stays(L):
    declared = _lib.declared_functions()
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name)
    assert L.mpa_abi_version() == 10 == _lib.ABI_VERSION


def test_arguments_are_refused_before_the_device_is_touched(L):
    err = L.mpa_last_error
    p = 4096                                                                  # a non-null, 256-byte aligned address: never dereferenced
    assert L.mpa_three_nn(p, p, -1, 4, 4, p, p, None) == -1 and b"negative" in err()
    assert L.mpa_three_nn(p, p, 2, -4, 4, p, p, None) == -1 and b"negative" in err()
    assert L.mpa_three_nn(p, p, 2, 4, -4, p, p, None) == -1 and b"negative" in err()
    assert L.mpa_three_nn(p, p, 2, 4, 0, p, p, None) == -1 and b"m=0" in err()
    assert L.mpa_three_nn(p, p, 2, 0, 4, p, p, None) == -1 and b"n=0" in err()
    assert L.mpa_three_nn(None, None, 0, 4, 0, None, None, None) == 0
    assert L.mpa_three_nn(p, p, 1 << 10, 699051, 4, p, p, None) == -1 and b"2^31" in err()     # 3 M n = 2^31 + 1024
    assert L.mpa_three_nn(p, p, 4, 1, 1 << 28, p, p, None) == -1 and b"2^31" in err()          # 3 M m
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert L.mpa_three_nn(args[0], args[1], 2, 4, 4, args[2], args[3], None) == -1 and b"null" in err()
    fwd = L.mpa_three_interpolate_forward
    assert fwd(p, p, p, 2, 3, -4, 5, p, None) == -1 and b"negative" in err()
    assert fwd(p, p, p, 2, -3, 4, 5, p, None) == -1 and b"negative" in err()
    assert fwd(p, p, p, 1 << 11, 1 << 10, 4, 1 << 10, p, None) == -1 and b"2^31" in err()     # M C n = 2^31
    assert fwd(p, p, p, 1 << 11, 1 << 10, 1 << 10, 4, p, None) == -1 and b"2^31" in err()     # M C m = 2^31
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert fwd(args[0], args[1], args[2], 2, 3, 4, 5, args[3], None) == -1 and b"null" in err()
    assert fwd(None, None, None, 2, 0, 4, 5, None, None) == 0 and fwd(None, None, None, 0, 3, 4, 5, None, None) == 0
    bwd = L.mpa_three_interpolate_backward
    assert bwd(p, p, p, 2, 3, 5, -4, p, p, None) == -1 and b"negative" in err()
    assert bwd(p, p, p, 1 << 11, 1 << 10, 1 << 10, 4, p, p, None) == -1 and b"2^31" in err()
    assert bwd(p, p, p, 2, 3, 5, 4, None, p, None) == -1 and b"null" in err()
    assert bwd(p, p, p, 2, 3, 5, 4, p, None, None) == -1 and b"null" in err()
    assert bwd(None, p, p, 2, 3, 5, 4, p, p, None) == -1 and b"null" in err()
    assert bwd(p, None, p, 2, 3, 5, 4, p, p, None) == -1 and b"null" in err()
    assert bwd(p, p, None, 2, 3, 5, 4, p, p, None) == -1 and b"null" in err()
    assert bwd(p, p, p, 2, 3, 5, 4, p + 128, p, None) == -1 and b"256-byte aligned" in err()
    assert bwd(None, None, None, 0, 3, 5, 4, None, None, None) == 0 and bwd(None, None, None, 2, 3, 5, 0, None, None, None) == 0


def test_the_workspace_query_is_pure_arithmetic(L):
    n = ctypes.c_int64(-1)
    # per cloud: start and cursor of m + 1 words and the list of 3 n words, each rounded up to 64 words
    assert L.mpa_three_interpolate_workspace(352, 1000, 128, ctypes.byref(n)) == 0 and n.value == 4 * 352 * (192 + 192 + 3008)
    assert L.mpa_three_interpolate_workspace(3, 21, 63, ctypes.byref(n)) == 0 and n.value == 4 * 3 * 64 * 3
    assert n.value % 256 == 0
    assert L.mpa_three_interpolate_workspace(3, -21, 63, ctypes.byref(n)) == -1 and b"negative" in L.mpa_last_error()
    assert L.mpa_three_interpolate_workspace(3, 21, 63, None) == -1 and b"null" in L.mpa_last_error()
    assert L.mpa_three_interpolate_workspace(1 << 20, 1 << 10, 4, ctypes.byref(n)) == -1 and b"2^31" in L.mpa_last_error()
    assert _lib.query("mpa_three_interpolate_workspace", 2, 7, 3) == 4 * 2 * 64 * 3
    assert _lib.query("mpa_three_interpolate_workspace", 2, 7, 3) == _lib.query("mpa_group_points_workspace", 2, 3, 7, 3)


# ---- the modules against the record of the reference's own ------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture(golden):
    return golden("pointnet2_fp_msg")


def fp_module(fixture):
    fp = PointnetFPModule([32, 32, 16])
    fp.load_state_dict({k[len("fp.sd."):]: torch.from_numpy(v) for k, v in fixture.items() if k.startswith("fp.sd.")})
    return fp.train()


def fp_tensors(fixture, device="cpu"):
    return {k: torch.from_numpy(fixture[f"fp.{k}"]).to(device) for k in ("unknown", "known", "unknow_feats", "known_feats", "w")}


def fp_pass(fp, x):
    """One training forward + backward and one eval forward -> the records of the fixture's FP case."""
    rec = {}
    hooks = [fp.mlp[0].register_forward_hook(lambda m, i, o: rec.__setitem__("out.interp", i[0].squeeze(-1)))]
    hooks += [fp.mlp[j].register_forward_hook(lambda m, i, o, j=j: rec.__setitem__(f"out.pre.{j}", o.detach().squeeze(-1).clone()))
              for j in (1, 4)]
    uf, kf = x["unknow_feats"].clone().requires_grad_(), x["known_feats"].clone().requires_grad_()
    rec["out.dist"], idx = pu.three_nn(x["unknown"], x["known"])
    out = fp(x["unknown"], x["known"], uf, kf)
    (out * x["w"]).sum().backward()
    for h in hooks:
        h.remove()
    fp.eval()
    with torch.no_grad():
        rec["out.eval"] = fp(x["unknown"], x["known"], uf, kf)
    fp.train()
    rec.update({"out.train": out, "gin.unknow_feats": uf.grad, "gin.known_feats": kf.grad})
    rec.update({f"stat.{k}": v for k, v in fp.state_dict().items() if "running_" in k})
    rec.update({f"grad.{k}": p.grad for k, p in fp.named_parameters()})
    return {k: v.detach().clone() for k, v in rec.items()}, idx


def test_fp_module_matches_every_record_of_the_reference_module(fixture):
    fp = fp_module(fixture)
    assert list(fp.state_dict()) == fixture["fp.names"].tolist()
    assert [",".join(map(str, v.shape)) for v in fp.state_dict().values()] == fixture["fp.shapes"].tolist()
    assert {k.split(".")[1] for k in fp.state_dict()} == {"0", "1", "3", "4"}
    rec, idx = fp_pass(fp, fp_tensors(fixture))
    assert np.array_equal(idx.numpy(), fixture["fp.idx"])
    want = {k[len("fp.f32."):] for k in fixture if k.startswith("fp.f32.")}
    assert set(rec) == want and rec["out.train"].shape == (3, 16, 40)
    for k, v in rec.items():                                                   # (the FP records keep their shapes)
        want_k = fixture["fp.f32." + k]
        assert want_k.dtype == f32 and want_k.shape == tuple(v.shape), k
        assert np.abs(v.numpy() - want_k).max() < REL * np.abs(want_k).max(), k
    twin = PointnetFPModule([32, 32, 16])                                      # a state_dict round trip
    twin.load_state_dict(copy.deepcopy(fp.state_dict()))
    x = fp_tensors(fixture)
    fp.eval(), twin.eval()
    with torch.no_grad():
        assert torch.equal(twin(x["unknown"], x["known"], x["unknow_feats"], x["known_feats"]),
                           fp(x["unknown"], x["known"], x["unknow_feats"], x["known_feats"]))


def test_fp_module_without_known_points_and_without_own_features(fixture):
    x = fp_tensors(fixture)
    fp = fp_module(fixture).eval()
    one = x["known_feats"][:, :, :1].contiguous()                             # [M, C2, 1]: one feature vector per cloud
    with torch.no_grad():
        out = fp(x["unknown"], None, x["unknow_feats"], one)
        want = fp.mlp(torch.cat([one.expand(3, 24, 40), x["unknow_feats"]], dim=1).unsqueeze(-1)).squeeze(-1)
    assert out.shape == (3, 16, 40) and torch.equal(out, want)
    bare = PointnetFPModule([24, 16], bn=False)
    assert list(bare.state_dict()) == ["mlp.0.weight", "mlp.0.bias"]
    assert bare(x["unknown"], x["known"], None, x["known_feats"]).shape == (3, 16, 40)


def test_no_relu_decision_of_the_fp_case_is_a_coin_toss(fixture):
    """The seed condition of the generator, on the float64 record: every pre-activation at least 100 x FLIP_PREACT of its
    channel's largest away from zero."""
    for j in (1, 4):
        pre = np.abs(fixture[f"fp.f64.out.pre.{j}"])
        assert pre.dtype == np.float64 and pre.shape == (3, (32, 16)[j == 4], 40)
        assert float((pre / pre.max(axis=(0, 2), keepdims=True)).min()) >= 100 * anchored.FLIP_PREACT


MSG_LEVEL0 = dict(npoint=512, radii=[0.1, 0.2, 0.4], nsamples=[16, 32, 128], mlps=[[0, 32, 32, 64], [0, 64, 64, 128], [0, 64, 96, 128]])


def msg_encoder(fixture):
    enc = PointNet2MSG(64)
    param_fill.fill_parameters(enc, int(fixture["msg.seed"]))
    return enc.train()


@pytest.fixture(scope="module")
def msg_run(fixture):
    enc = msg_encoder(fixture)
    pts = torch.from_numpy(fixture["msg.points"]).requires_grad_()
    levels = []
    out = enc(pts, record=levels)
    (out * torch.from_numpy(fixture["msg.w"])).sum().backward()
    enc.eval()
    with torch.no_grad():
        out_eval = enc(pts.detach())
    return enc, out, out_eval, levels, pts.grad


def test_msg_state_dict_names_and_shapes_equal_the_reference(fixture):
    sd = PointNet2MSG(64).state_dict()
    assert list(sd) == fixture["msg.names"].tolist()
    assert [",".join(map(str, v.shape)) for v in sd.values()] == fixture["msg.shapes"].tolist()
    for i, scales in enumerate((3, 3, 1)):
        for s in range(scales):
            for j in (0, 1, 3, 4, 6, 7):
                assert f"SA_modules.{i}.mlps.{s}.{j}.weight" in sd
    assert sd["SA_modules.1.mlps.2.0.weight"].shape == (128, 323, 1, 1)
    assert sd["SA_modules.2.mlps.0.0.weight"].shape == (256, 643, 1, 1)
    assert isinstance(PointNet2MSG(64), PointNet2SSG) and PointNet2MSG.host_sync_per_forward is True


def test_msg_encoder_matches_every_record_of_the_reference_encoder(fixture, msg_run):
    enc, out, out_eval, levels, gin = msg_run
    assert out.shape == (2, 64) and out.dtype == torch.float32
    got = {"out.train": out, "out.eval": out_eval, "gin.points": gin}
    assert [None if x is None else tuple(x.shape) for x, _ in levels] == [(2, 512, 3), (2, 128, 3), None]
    assert [tuple(f.shape) for _, f in levels] == [(2, 320, 512), (2, 640, 128), (2, 64, 1)]
    for i, (new_xyz, feats) in enumerate(levels):
        if new_xyz is not None:
            got[f"new_xyz.{i}"] = new_xyz
        got[f"features.{i}"] = feats
    got.update({f"stat.{k}": v for k, v in enc.state_dict().items() if "running_" in k})
    grads = {k: p.grad for k, p in enc.named_parameters()}
    got.update({f"grad.{k}": v for k, v in grads.items()})
    want = {k[len("msg.f32."):].split("#")[0] for k in fixture if k.startswith("msg.f32.")}
    assert set(got) == want
    for k, v in got.items():
        floor = 0.0
        if k.startswith("grad.") and k.endswith(".bias"):  # zero up to rounding in front of a normalisation: relative to the layer's weights
            floor = float(grads[k[len("grad."):-len("bias")] + "weight"].abs().max())
        param_fill.compare(fixture, "msg.f32.", k, v.detach().numpy(), REL, floor=floor)


def test_sa_module_msg_alone_matches_the_record_and_leaves_its_arguments(fixture):
    args = copy.deepcopy(MSG_LEVEL0)
    module = PointnetSAModuleMSG(**args)
    assert args == MSG_LEVEL0                                                   # (upstream adds 3 to every first width)
    assert sorted({k.rsplit(".", 1)[0] for k in module.state_dict()}) == sorted(
        f"mlps.{s}.{j}" for s in range(3) for j in (0, 1, 3, 4, 6, 7))
    module.load_state_dict(msg_encoder(fixture).SA_modules[0].state_dict())
    new_xyz, feats = module.train()(torch.from_numpy(fixture["msg.points"]), None)
    param_fill.compare(fixture, "msg.f32.", "new_xyz.0", new_xyz.numpy(), REL)
    param_fill.compare(fixture, "msg.f32.", "features.0", feats.detach().numpy(), REL)
    with pytest.raises(ValueError):
        PointnetSAModuleMSG(8, [0.1], [4, 4], [[0, 8]])
    single = PointnetSAModule(mlp=[0, 8, 8], npoint=4, radius=0.3, nsample=2)
    assert isinstance(single, PointnetSAModuleMSG) and list(single.state_dict())[0] == "mlps.0.0.weight"
    assert single.mlps[0][0].in_channels == 3 and len(single.groupers) == 1


def test_msg_forward_parts_runs_the_valid_parts_only():
    enc = PointNet2MSG(32).train()
    twin = copy.deepcopy(enc)
    g = torch.Generator().manual_seed(0)
    pcs = torch.rand(4, 80, 3, generator=g) + 0.2
    pcs[1] = float("nan")                                     # a padded slot is never read
    valids = torch.tensor([1.0, 0.0, 1.0, 1.0])
    out = enc.forward_parts(pcs, valids)
    assert out.shape == (4, 32) and torch.isfinite(out).all() and float(out[1].detach().abs().max()) == 0.0
    assert torch.equal(twin(pcs[[0, 2, 3]]), out[[0, 2, 3]])


def test_msg_fused_evaluation_takes_the_library_chain_with_one_warning(fixture):
    enc = msg_encoder(fixture).eval()
    pts = torch.from_numpy(fixture["msg.points"])
    with torch.no_grad():
        want = enc(pts)
        enc.set_eval_mlp("fused")
        with pytest.warns(UserWarning, match="3 scales"):
            got = enc(pts)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            again = enc(pts)
    assert torch.equal(got, want) and torch.equal(again, want)
