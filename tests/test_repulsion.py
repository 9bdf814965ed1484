"""The repulsion loss without a GPU: the numpy restatement (`repulsion_ref`) against the reference's recorded run and a
float64 brute force, its diagonal constant, the exactness of the bounding-box prune, a sample without a valid part, the
ABI's refusals, the host path of `loss.repulsion_cd_loss(fused=True)`, and the configuration keys of the model term."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from multi_part_assembly_amd import _build, _lib, config, eval_utils
from multi_part_assembly_amd import loss as loss_mod
from multi_part_assembly_amd import repulsion_ref as rr
from tool_loader import load_tool

F32 = np.float32


def make_case(seed, B=3, P=4, N=40, spread=0.25, size=0.15):
    """Clouds of half-width `size` around centres drawn `spread` wide: some pairs interpenetrate, some are far apart."""
    rng = np.random.RandomState(seed)
    pcs = (rng.uniform(-1, 1, (B, P, N, 3)) * size + rng.uniform(-1, 1, (B, P, 1, 3)) * spread).astype(F32)
    return pcs, np.ones((B, P), dtype=F32)


def lattice_case(B=2, P=3, N=64):
    """Points on a grid of step 1/8 (every distance exact in float32, ties everywhere); the parts are shifted copies."""
    g = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3)[:N].astype(F32) / 8
    pcs = np.stack([np.stack([g + F32(0.125) * ((b + p) % 3) for p in range(P)]) for b in range(B)]).astype(F32)
    return pcs, np.ones((B, P), dtype=F32)


def duplicated_case(seed=3, B=2, P=3, N=48):
    """Every point appears four times in its part, and part 1 is a copy of part 0 (cd = 0 exactly)."""
    pcs, valids = make_case(seed, B, P, N // 4, spread=0.1)
    pcs = np.tile(pcs, (1, 1, 4, 1))
    pcs[:, 1] = pcs[:, 0]
    return pcs, valids


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300))


def clear_of_the_hinge(pcs, valids, thre, margin=1e-4):
    """No valid pair's float64 cd lies within margin * thre of thre."""
    _, cd, _ = rr.repulsion_cd(pcs, valids, thre, dtype=np.float64, prune=False)
    for b in range(pcs.shape[0]):
        for i, j in rr.pair_slots(pcs.shape[1]):
            if valids[b, i] == 1 and valids[b, j] == 1 and abs(cd[b, i, j] - thre) <= margin * thre:
                return False
    return True


# ---- the restatement against the reference's record and a brute force -------------------------------------------------------
def test_restatement_equals_the_reference_record(golden, capsys):
    """tests/golden/repulsion.npz: the reference's own function on the CPU.  The float64 restatement reproduces the recorded
    anchor bit for bit; the reference's float32 run and the float32 restatement both sit within 1e-5 of it (two float32
    evaluations of sums of ~65 squared distances: a few 2^-24 each)."""
    z = golden("repulsion")
    pcs, valids, w = z["pcs"], z["valids"], z["w"]
    assert valids.tolist() == [[1, 1, 1, 1], [1, 0, 1, 1]] and z["carriers"].min() > 0
    for k, thre in enumerate(z["thre"]):
        assert clear_of_the_hinge(pcs, valids, float(thre))
        l64, c64, _ = rr.repulsion_cd(pcs, valids, thre, dtype=np.float64, prune=False)
        g64 = rr.repulsion_cd_grad(pcs, valids, thre, w, dtype=np.float64, prune=False)
        assert np.array_equal(l64, z["f64.loss"][k]) and np.array_equal(g64, z["f64.grad"][k])
        assert np.array_equal(c64, z["f64.cd"][k])
        l32, _, _ = rr.repulsion_cd(pcs, valids, thre)
        g32 = rr.repulsion_cd_grad(pcs, valids, thre, w)
        assert l32.dtype == F32 and g32.dtype == F32
        e32 = (rel(l32, l64), rel(g32, g64))
        eref = (rel(z["ref.loss"][k], l64), rel(z["ref.grad"][k], g64))
        with capsys.disabled():
            print(f"\n  thre {thre:g}: e32 loss {e32[0]:.2e} grad {e32[1]:.2e}; reference loss {eref[0]:.2e} grad {eref[1]:.2e}",
                  end="")
        assert max(e32) <= 1e-5 and max(eref) <= 1e-5
        assert np.all(g64[valids != 1] == 0) and int((np.abs(z["ref.grad"][k]).sum(-1) > 0).sum()) == z["carriers"][k]


@pytest.mark.parametrize("case", ["random", "lattice", "duplicated", "masked"])
def test_restatement_equals_float64_brute_force(case):
    """The algebra: unordered pairs twice plus `thre` per valid part against the reference's P x P formulation."""
    if case == "lattice":
        pcs, valids = lattice_case()
    elif case == "duplicated":
        pcs, valids = duplicated_case()
    else:
        pcs, valids = make_case(11, B=3, P=5, N=33)
    if case == "masked":
        valids[0] = [1, 0, 1, 1, 0]
        valids[1] = [0, 0, 1, 0, 0]
    for thre in (0.02, 0.1, 0.5):
        want = rr.brute_force(pcs, valids, thre)
        for prune in (False, True):
            got, _, _ = rr.repulsion_cd(pcs, valids, thre, dtype=np.float64, prune=prune)
            assert rel(got, want) < 1e-12, (case, thre, prune)
        got32, _, _ = rr.repulsion_cd(pcs, valids, thre)
        assert rel(got32, want) < 1e-5


def test_search_follows_the_chamfer_contract():
    """First index on ties, both directions; identical parts give cd = 0 and the identity lists."""
    pcs, _ = duplicated_case()
    d1, i1, d2, i2 = rr.pair_search(pcs[0, 0], pcs[0, 1])
    n = pcs.shape[2] // 4
    assert np.all(d1 == 0) and np.all(d2 == 0)
    assert np.array_equal(i1, np.arange(4 * n) % n) and np.array_equal(i2, np.arange(4 * n) % n)  # the first of four copies
    far = np.full((3, 3), 1e17, dtype=F32)
    d1, i1, _, _ = rr.pair_search(np.zeros((2, 3), F32), far)  # d overflows past 1e32
    assert np.all(d1 == F32(1e32)) and np.all(i1 == -1)


def test_ordered_sum_is_a_sum():
    rng = np.random.RandomState(0)
    for n in (1, 2, 63, 64, 65, 257, 1000, 2048):
        v = rng.rand(n).astype(F32)
        assert abs(float(rr.ordered_sum(v)) - float(v.astype(np.float64).sum())) <= 1e-6 * n
        assert rr.ordered_sum(v).dtype == F32
        assert rr.ordered_sum(v.astype(np.float64)) == pytest.approx(v.astype(np.float64).sum(), rel=1e-14)


def test_diagonal_constant():
    """Parts far apart: nothing but the diagonal's `thre` per valid part is left, loss = thre / nv."""
    pcs, valids = make_case(5, B=3, P=4, N=16, size=0.01, spread=0.0)
    pcs += (np.arange(4, dtype=F32) * 10)[None, :, None, None]
    valids[1] = [1, 0, 1, 0]
    valids[2] = [0, 0, 0, 1]
    for thre in (0.01, 0.3):
        for prune in (True, False):
            loss, cd, flag = rr.repulsion_cd(pcs, valids, thre, prune=prune)
            nv = valids.sum(1).astype(F32)
            assert np.array_equal(loss, (nv * F32(thre)) / (nv * nv))
            assert np.allclose(loss, thre / nv, rtol=1e-6)
            assert not (flag == rr.HINGED).any() and (prune or (cd[0] > 0).sum() == 12)


def test_prune_never_fires_on_a_hinged_pair():
    """Property: whenever the box gap is >= thre, the float32 cd of the full search is >= thre (the hinge is exactly zero),
    so loss and gradient are the same bits with and without the prune.  Random boxes at all scales of gap / thre."""
    rng = np.random.RandomState(42)
    fired = 0
    for trial in range(300):
        N = int(rng.choice([1, 3, 17, 64]))
        a = (rng.uniform(-1, 1, (N, 3)) * rng.uniform(0.01, 0.3)).astype(F32)
        b = (rng.uniform(-1, 1, (N, 3)) * rng.uniform(0.01, 0.3) + rng.uniform(-1, 1, 3) * 0.5).astype(F32)
        g = rr.box_gap(a, b)
        d = rr.pair_distances(a, b)
        assert g.dtype == F32 and (d >= g).all()  # the gap is a lower bound of every COMPUTED distance
        for thre in (F32(g), np.nextafter(F32(g), F32(np.inf)), F32(g) * F32(0.5), F32(0.05)):
            if thre <= 0:
                continue
            if rr.pruned(a, b, thre):
                fired += 1
                d1, _, d2, _ = rr.pair_search(a, b)
                assert not (F32(thre) - (rr.mean(d1) + rr.mean(d2)) > 0)
    assert fired > 200
    pcs, valids = make_case(9, B=4, P=5, N=24, spread=0.4, size=0.1)
    for thre in (0.01, 0.05, 0.3):
        full, pruned = rr.repulsion_cd(pcs, valids, thre, prune=False), rr.repulsion_cd(pcs, valids, thre, prune=True)
        assert np.array_equal(full[0], pruned[0])
        assert (pruned[2] == rr.NOT_SEARCHED).sum() > (full[2] == rr.NOT_SEARCHED).sum() or thre == 0.3
        assert np.array_equal(full[2] == rr.HINGED, pruned[2] == rr.HINGED)
        w = np.ones(4, F32)
        assert np.array_equal(rr.repulsion_cd_grad(pcs, valids, thre, w, prune=False),
                              rr.repulsion_cd_grad(pcs, valids, thre, w, prune=True))


@pytest.mark.parametrize("N", [64, 2048])
def test_prune_on_facing_box_faces(N):
    """The adversarial case: all points of both parts lie on the facing faces of their boxes, opposite each other, so every
    nearest distance EQUALS the gap g and cd = 2 g to rounding -- the smallest cd a gap of g allows.  With thre = g (and one
    ulp either side) the pruned pair's hinge thre - cd is not positive, at the largest N of the envelope too."""
    rng = np.random.RandomState(N)
    yz = rng.uniform(-1, 1, (N, 2)).astype(F32)
    for s in (F32(0.1), F32(0.3333333), F32(1e-3)):
        a = np.concatenate([np.zeros((N, 1), F32), yz], 1)
        b = np.concatenate([np.full((N, 1), s, F32), yz], 1)
        g = rr.box_gap(a, b)
        assert g == s * s
        d1, i1, d2, i2 = rr.pair_search(a, b)
        assert np.all(d1 == g) and np.all(d2 == g) and np.array_equal(i1, np.arange(N))
        cd = rr.mean(d1) + rr.mean(d2)
        for thre in (np.nextafter(g, F32(0)), g, np.nextafter(g, F32(1))):
            assert rr.pruned(a, b, thre) == bool(g >= thre)
            if rr.pruned(a, b, thre):
                assert cd >= thre and not (thre - cd > 0)
        assert cd >= F32(2) * g * F32(1 - N * 2.0 ** -24)


def test_sample_without_a_valid_part():
    pcs, valids = make_case(2, B=2, P=3, N=8)
    valids[1] = 0
    pcs[1] = np.nan
    for dtype in (np.float32, np.float64):
        loss, cd, flag = rr.repulsion_cd(pcs, valids, 0.5, dtype=dtype)
        assert np.isfinite(loss[0]) and np.isnan(loss[1]) and not flag[1].any() and np.all(cd[1] == 0)
        grad = rr.repulsion_cd_grad(pcs, valids, 0.5, np.ones(2), dtype=dtype)
        assert np.all(grad[1] == 0) and np.abs(grad[0]).max() > 0


def test_gradient_is_the_derivative():
    """Central differences of the float64 restatement (points in general position: the arg-mins do not move)."""
    pcs, valids = make_case(21, B=1, P=3, N=6, spread=0.05)
    valids[0, 1] = 1
    w = np.array([1.7])
    x = pcs.astype(np.float64)
    grad = rr.repulsion_cd_grad(x, valids, 0.2, w, dtype=np.float64, prune=False)
    assert np.abs(grad).max() > 0
    rng = np.random.RandomState(0)
    for _ in range(12):
        p, n, k = rng.randint(3), rng.randint(6), rng.randint(3)
        h = 1e-6
        up, dn = x.copy(), x.copy()
        up[0, p, n, k] += h
        dn[0, p, n, k] -= h
        num = w[0] * (rr.repulsion_cd(up, valids, 0.2, dtype=np.float64, prune=False)[0][0]
                      - rr.repulsion_cd(dn, valids, 0.2, dtype=np.float64, prune=False)[0][0]) / (2 * h)
        assert num == pytest.approx(grad[0, p, n, k], rel=1e-5, abs=1e-9)


# ---- the ABI and the Python entry without a GPU -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    return _build.build()


def test_abi_refuses_bad_arguments_without_a_gpu(built):
    L = _lib.lib()
    n, f, a, b = (ctypes.c_int64() for _ in range(4))
    ref = lambda *x: [ctypes.byref(v) for v in x]
    assert L.mpa_repulsion_cd_workspace(2, 3, 5, *ref(n, f, a, b)) == 0
    assert (n.value, f.value, a.value, b.value) == (1024, 0, 512, 768)  # 6 slots: flags, hinges, two lists of 6 x 5 x 2 bytes
    assert L.mpa_repulsion_cd_workspace(32, 20, 1000, *ref(n, f, a, b)) == 0
    assert 2 * 32 * 190 * 1000 * 2 <= n.value <= 2 * 32 * 190 * 1000 * 2 + 32 * 190 * 5 + 1024
    assert L.mpa_repulsion_cd_workspace(4, 1, 7, *ref(n), None, None, None) == 0 and n.value == 0
    assert L.mpa_repulsion_cd_workspace(2, 65, 5, *ref(n, f, a, b)) == -1 and b"P=65" in L.mpa_last_error()
    assert L.mpa_repulsion_cd_workspace(2, 3, 2049, *ref(n, f, a, b)) == -1 and b"N=2049" in L.mpa_last_error()
    assert L.mpa_repulsion_cd_workspace(2, 3, 0, *ref(n, f, a, b)) == -1 and b"N=0" in L.mpa_last_error()
    thre = ctypes.c_float(0.1)
    assert L.mpa_repulsion_cd_forward(None, None, thre, -1, 3, 5, None, None, None, None, None) == -1
    assert b"negative" in L.mpa_last_error()
    assert L.mpa_repulsion_cd_forward(None, None, thre, 2, 0, 5, None, None, None, None, None) == -1
    assert L.mpa_repulsion_cd_forward(None, None, thre, 2, 3, 5, None, None, None, None, None) == -1
    assert b"null" in L.mpa_last_error()
    assert L.mpa_repulsion_cd_forward(None, None, thre, 0, 3, 5, None, None, None, None, None) == 0
    assert L.mpa_repulsion_cd_backward(None, None, None, 2, 3, 5, None, None, None) == -1 and b"null" in L.mpa_last_error()
    assert L.mpa_repulsion_cd_backward(None, None, None, 2, 3, 4096, None, None, None) == -1
    assert b"N=4096" in L.mpa_last_error()
    assert L.mpa_repulsion_cd_backward(None, None, None, 0, 3, 5, None, None, None) == 0


def test_python_entry_on_host_tensors(monkeypatch):
    """fused=True outside the kernel's reach warns once and takes the restatement: value, cd and gradient."""
    monkeypatch.setattr(eval_utils, "_warned", set())
    pcs, valids = make_case(4, B=2, P=3, N=9, spread=0.05)
    valids[1, 0] = 0
    x = torch.from_numpy(pcs).requires_grad_()
    with pytest.warns(UserWarning, match="repulsion_cd_loss"):
        loss = loss_mod.repulsion_cd_loss(x, torch.from_numpy(valids), 0.2, fused=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # once
        loss2, cd = loss_mod.repulsion_cd_loss(x, torch.from_numpy(valids), 0.2, fused=True, ret_cd=True)
    want = rr.repulsion_cd(pcs, valids, 0.2)
    assert np.array_equal(loss.detach().numpy(), want[0]) and np.array_equal(loss2.detach().numpy(), want[0])
    assert np.array_equal(cd.numpy(), rr.repulsion_cd(pcs, valids, 0.2, prune=False)[1]) and not cd.requires_grad
    w = torch.tensor([0.5, 2.0])
    (grad,) = torch.autograd.grad((loss * w).sum(), x)
    assert np.array_equal(grad.numpy(), rr.repulsion_cd_grad(pcs, valids, 0.2, w.numpy()))
    assert not loss_mod.repulsion_supported(x) and not loss_mod.repulsion_supported(torch.zeros(1, 2, 3))
    with pytest.raises(ValueError, match=r"\[B, P, N, 3\]"):
        loss_mod.repulsion_cd_loss(torch.zeros(2, 3, 4), torch.ones(2, 3), 0.1, fused=True)
    with pytest.raises(ValueError, match="valids"):
        loss_mod.repulsion_cd_loss(torch.zeros(2, 3, 4, 3), torch.ones(2, 4), 0.1, fused=True)
    with pytest.raises(ValueError, match="outside"):
        loss_mod.repulsion_cd_search(x, torch.from_numpy(valids), 0.1)


# ---- the model term's configuration --------------------------------------------------------------------------------------------
def _model(cfg):
    from multi_part_assembly_amd.pn_transformer import build_model
    return build_model(cfg)


def test_term_is_off_unless_asked_for(monkeypatch):
    from multi_part_assembly_amd import base_model
    for preset in ("pn_transformer_everyday", "dgl_everyday", "dgl_partnet_chair"):
        cfg = getattr(config, preset)()
        assert not any("repulsion" in k for k in cfg.loss)  # no preset turns the term on or ships a threshold
        model = _model(cfg)
        assert model.use_repulsion_loss is False
        called = []
        monkeypatch.setattr(base_model, "transform_pc", lambda *a, **k: called.append(1))
        terms = {"trans_loss": 1, "rot_pt_cd_loss": 2, "transform_pt_cd_loss": 3}
        model._add_repulsion_loss(terms, None, None, None, None)
        assert list(terms) == ["trans_loss", "rot_pt_cd_loss", "transform_pt_cd_loss"] and not called
        cfg.loss.use_repulsion_loss = False
        assert _model(cfg).use_repulsion_loss is False


def test_term_needs_its_threshold_and_weight(monkeypatch):
    from multi_part_assembly_amd import base_model
    cfg = config.pn_transformer_everyday()
    cfg.loss.use_repulsion_loss = True
    with pytest.raises(ValueError, match="repulsion_thre"):
        _model(cfg)
    cfg.loss.repulsion_thre = 0.2
    with pytest.raises(ValueError, match="repulsion_loss_w"):
        _model(cfg)
    cfg.loss.repulsion_loss_w = 3.0
    model = _model(cfg)
    assert model.use_repulsion_loss is True
    # the term on host tensors: the posed prediction through the restatement, appended behind the existing keys
    monkeypatch.setattr(eval_utils, "_warned", set())
    monkeypatch.setattr(base_model, "transform_pc", lambda trans, rot, pc, rot_type=None: pc + trans[:, :, None, :])
    pcs, valids = make_case(4, B=2, P=3, N=9, spread=0.05)
    trans = torch.tensor(np.random.RandomState(0).uniform(-0.02, 0.02, (2, 3, 3)).astype(F32), requires_grad=True)
    terms = {"trans_loss": torch.zeros(2)}
    with pytest.warns(UserWarning, match="repulsion_cd_loss"):
        model._add_repulsion_loss(terms, trans, None, torch.from_numpy(pcs), torch.from_numpy(valids))
    assert list(terms) == ["trans_loss", "repulsion_loss"] and terms["repulsion_loss"].shape == (2,)
    posed = pcs + trans.detach().numpy()[:, :, None, :]
    assert np.array_equal(terms["repulsion_loss"].detach().numpy(), rr.repulsion_cd(posed, valids, 0.2)[0])
    terms["repulsion_loss"].sum().backward()
    assert trans.grad is not None and trans.grad.abs().max() > 0
    assert float(cfg.loss["repulsion_loss_w"]) == 3.0  # what `loss_function` reads through the `<term>_w` rule


def test_train_tool_sets_the_three_keys():
    train = load_tool("train")
    base = ["--preset", "pn_transformer_everyday", "--synthetic"]
    cfg = train.configure(train.parse_args(base))
    assert "use_repulsion_loss" not in cfg.loss and cfg.loss == config.pn_transformer_everyday().loss
    cfg = train.configure(train.parse_args(base + ["--repulsion", "0.02", "1.5"]))
    assert cfg.loss.use_repulsion_loss is True and cfg.loss.repulsion_thre == 0.02 and cfg.loss.repulsion_loss_w == 1.5
    with pytest.raises(SystemExit):
        train.parse_args(base + ["--repulsion", "0.02"])
