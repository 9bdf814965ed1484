"""csrc/repulsion.hip on the MI355X: nearest neighbours equal to `chamfer_distance` and loss / cd / flags equal to the
float32 restatement, bit for bit, at the edges of the envelope, on ties, on both sides of the prune and of the hinge, eager
and captured; the gradient against the float64 restatement under the bars of tests/anchored.py; the term in a model step."""
import warnings

import numpy as np
import pytest
import torch

import anchored
from multi_part_assembly_amd import config, eval_utils, synthetic
from multi_part_assembly_amd import loss as L
from multi_part_assembly_amd import repulsion_ref as rr
from multi_part_assembly_amd.chamfer import chamfer_forward
from multi_part_assembly_amd.pn_transformer import build_model
from multi_part_assembly_amd.trainer import Trainer
from multi_part_assembly_amd.transforms import transform_pc
from test_repulsion import clear_of_the_hinge, duplicated_case, lattice_case, make_case

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
F32 = np.float32


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F32 else a


def same_bits(a, b):
    """Equal bit for bit; a NaN equals a NaN (the host's 0 / 0 and the device's differ in the sign bit)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != F32:
        return np.array_equal(a, b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


def search(dev, pcs, valids, thre, ret_cd=False):
    """The forward on sentinel-filled outputs -> numpy dict (loss, flag, idx1, idx2, dist1, dist2[, cd])."""
    B, P, N, _ = pcs.shape
    out = {"loss": torch.full((B,), 7.0, device=dev)}
    if ret_cd:
        out["cd"] = torch.full((B, P, P), 7.0, device=dev)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = L.repulsion_cd_search(T(pcs, dev), T(valids, dev), thre, ret_cd=ret_cd, out=out)
    assert res["loss"] is out["loss"] and (not ret_cd or res["cd"] is out["cd"])
    return {k: v.cpu().numpy() for k, v in res.items() if k not in ("workspace", "dists")}


def check_against_restatement(dev, pcs, valids, thre, ret_cd, chamfer=True):
    """loss, flags (and cd) equal the float32 restatement's bits; d1 / d2 / indices of every searched pair equal
    `chamfer_distance` on that pair, bit for bit (and the restatement's).  Returns the device results."""
    got = search(dev, pcs, valids, thre, ret_cd)
    loss, cd, flag, found = rr.repulsion_cd(pcs, valids, thre, prune=not ret_cd, details=True)
    assert same_bits(got["loss"], loss), (got["loss"], loss)
    assert np.array_equal(got["flag"], flag)
    if ret_cd:
        assert same_bits(got["cd"], cd)
    slots = rr.pair_slots(pcs.shape[1])
    keys = sorted(found)
    for (b, i, j) in keys:
        k = slots.index((i, j))
        d1, i1, d2, i2 = found[(b, i, j)]
        assert same_bits(got["dist1"][b, k], d1) and same_bits(got["dist2"][b, k], d2), (b, i, j)
        assert np.array_equal(got["idx1"][b, k], i1) and np.array_equal(got["idx2"][b, k], i2), (b, i, j)
    if chamfer and keys:
        a = T(np.stack([pcs[b, i] for b, i, _ in keys]), dev)
        c = T(np.stack([pcs[b, j] for b, _, j in keys]), dev)
        cd1, ci1, cd2, ci2 = (t.cpu().numpy() for t in chamfer_forward(a, c))
        for n, (b, i, j) in enumerate(keys):
            k = slots.index((i, j))
            assert same_bits(got["dist1"][b, k], cd1[n]) and same_bits(got["dist2"][b, k], cd2[n])
            assert np.array_equal(got["idx1"][b, k], ci1[n]) and np.array_equal(got["idx2"][b, k], ci2[n])
    return got


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257])
@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_kernel_equals_restatement_and_chamfer(cuda_device, P, N):
    pcs, valids = make_case(100 * P + N, B=3, P=P, N=N, size=0.12, spread=0.3)
    thre = 0.08
    assert clear_of_the_hinge(pcs, valids, thre)
    got = check_against_restatement(cuda_device, pcs, valids, thre, ret_cd=False)
    check_against_restatement(cuda_device, pcs, valids, thre, ret_cd=True)
    assert P < 2 or N < 2 or (got["flag"] == rr.HINGED).any()  # the case decides something


@pytest.mark.parametrize("P,N", [(64, 32), (2, 2048)])
def test_edges_of_the_envelope(cuda_device, P, N):
    pcs, valids = make_case(P + N, B=2, P=P, N=N, size=0.1, spread=0.3)
    valids[1, P // 2:] = 0
    thre = 0.05
    assert clear_of_the_hinge(pcs, valids, thre)
    check_against_restatement(cuda_device, pcs, valids, thre, ret_cd=False)
    if N == 2048:
        check_against_restatement(cuda_device, pcs, valids, thre, ret_cd=True)


@pytest.mark.parametrize("case", ["lattice", "duplicated", "identical"])
def test_exact_ties(cuda_device, case):
    if case == "lattice":
        pcs, valids = lattice_case()
    elif case == "duplicated":
        pcs, valids = duplicated_case()
    else:
        pcs, valids = make_case(1, B=2, P=3, N=70)
        pcs[:, 1:] = pcs[:, :1]
    for thre in (0.03, 0.4):  # (cd of identical parts is 0: far from any thre)
        assert clear_of_the_hinge(pcs, valids, thre)
        check_against_restatement(cuda_device, pcs, valids, thre, ret_cd=False)
        check_against_restatement(cuda_device, pcs, valids, thre, ret_cd=True)


def test_both_sides_of_the_prune_and_of_the_hinge(cuda_device):
    """Two boxes a gap s apart along x with all points on the facing faces: g = s * s exactly and cd = 2 g to rounding.
    thre just below / at / above g moves the pair across the prune; thre around 2 g moves it across the hinge."""
    N, s = 65, F32(0.25)
    rng = np.random.RandomState(0)
    yz = rng.uniform(-1, 1, (N, 2)).astype(F32)
    a = np.concatenate([np.zeros((N, 1), F32), yz], 1)
    b = np.concatenate([np.full((N, 1), s, F32), yz], 1)
    pcs, valids = np.stack([a, b])[None], np.ones((1, 2), F32)
    g = rr.box_gap(a, b)
    assert g == s * s
    seen = set()
    for thre in (np.nextafter(g, F32(0)), g, np.nextafter(g, F32(1)), F32(1.5) * g, F32(1.999) * g, F32(2.001) * g, F32(3) * g):
        assert clear_of_the_hinge(pcs, valids, float(thre))
        got = check_against_restatement(cuda_device, pcs, valids, float(thre), ret_cd=False)
        assert got["flag"][0, 0] == (rr.NOT_SEARCHED if g >= thre else rr.HINGED if thre > 2 * g else rr.SEARCHED)
        seen.add(int(got["flag"][0, 0]))
        full = check_against_restatement(cuda_device, pcs, valids, float(thre), ret_cd=True)
        assert same_bits(full["loss"], got["loss"])  # the prune changes no result
    assert seen == {0, 1, 2}


def test_masks_nan_in_padded_slots_and_repeated_runs(cuda_device):
    pcs, valids = make_case(7, B=4, P=5, N=65, spread=0.2)
    valids[0] = [1, 0, 1, 1, 0]   # no prefix
    valids[1] = [0, 0, 1, 0, 0]   # one valid part
    valids[2] = 0                 # none
    thre = 0.1
    assert clear_of_the_hinge(pcs, valids, thre)
    dev = cuda_device
    for ret_cd in (False, True):
        want = check_against_restatement(dev, pcs, valids, thre, ret_cd)
        assert np.isnan(want["loss"][2]) and want["loss"][1] == F32(thre) and np.isfinite(want["loss"][[0, 3]]).all()
        dirty = pcs.copy()
        dirty[valids != 1] = np.nan
        got = check_against_restatement(dev, dirty, valids, thre, ret_cd, chamfer=False)
        again = search(dev, dirty, valids, thre, ret_cd)
        for k in ("loss", "flag") + (("cd",) if ret_cd else ()):
            assert same_bits(got[k], want[k]) and same_bits(again[k], want[k]), k
    # backward: every element written (sentinel-free), zeros in padded slots and for the sample without a valid part
    x = T(dirty, dev).requires_grad_()
    w = torch.tensor([1.0, 2.0, 3.0, 0.5], device=dev)
    grads = []
    for _ in range(2):
        loss = L.repulsion_cd_loss(x, T(valids, dev), thre, fused=True)
        (g,) = torch.autograd.grad((loss * w)[[0, 1, 3]].sum() + 0 * loss[2], x)
        grads.append(g.cpu().numpy())
    assert same_bits(grads[0], grads[1])
    assert np.all(grads[0][valids != 1] == 0) and np.all(grads[0][1] == 0) and np.all(grads[0][2] == 0)
    assert np.isfinite(grads[0]).all() and np.abs(grads[0][0]).max() > 0
    want = rr.repulsion_cd_grad(pcs, valids, thre, np.array([1.0, 2.0, 3.0, 0.5], F32))
    assert same_bits(grads[0], want)  # the restatement's order of the sums is the kernel's
    # the raw call on a sentinel-filled gradient: every element is written
    from multi_part_assembly_amd import _lib
    res = L.repulsion_cd_search(T(dirty, dev), T(valids, dev), thre)
    raw = torch.full((4, 5, 65, 3), 7.0, device=dev)
    _lib.launch("mpa_repulsion_cd_backward", dev, w, T(dirty, dev), T(valids, dev), 4, 5, 65, res["workspace"], raw)
    assert same_bits(raw.cpu().numpy(), rr.repulsion_cd_grad(pcs, valids, thre, w.cpu().numpy()))


def _anchor(pcs, valids, thre, w):
    """(r32, r64) of the restatement on the CPU: loss and gradient of sum(w * loss)."""
    out = []
    for dtype in (np.float32, np.float64):
        loss, _, _ = rr.repulsion_cd(pcs, valids, thre, dtype=dtype, prune=False)
        grad = rr.repulsion_cd_grad(pcs, valids, thre, w, dtype=dtype, prune=False)
        out.append({"loss": torch.from_numpy(loss.astype(np.float64)), "grad": torch.from_numpy(grad.astype(np.float64))})
    return out


@pytest.mark.parametrize("shape", [(3, 4, 33), (2, 5, 130), (2, 3, 257)])
def test_gradient_against_float64_and_fused_against_composed(cuda_device, shape, capsys):
    """Loss and d / d pcs against the float64 restatement's under min(1e-4, 8 max(e32, median e32)), e32 from the float32
    CPU restatement; the composition (fused=False) on the device is held to the same bars."""
    B, P, N = shape
    pcs, valids = make_case(31 + N, B=B, P=P, N=N, size=0.12, spread=0.15)
    valids[0, 1] = 0
    thre = 0.06
    assert clear_of_the_hinge(pcs, valids, thre)
    w = np.linspace(0.5, 1.5, B).astype(F32)
    r32, r64 = _anchor(pcs, valids, thre, w)
    assert float(r64["grad"].abs().max()) > 0
    for fused in (True, False):
        x = T(pcs, cuda_device).requires_grad_()
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            loss = L.repulsion_cd_loss(x, T(valids, cuda_device), thre, fused=fused)
        (g,) = torch.autograd.grad((loss * T(w, cuda_device)).sum(), x)
        g = g.clone()
        g[T(valids, cuda_device) != 1] = 0  # (the composition's padded rows carry nothing either; pinned for both)
        anchored.assert_anchored({"loss": loss.detach(), "grad": g}, r32, r64, f"repulsion {shape} fused={fused}", capsys)


def test_golden_record_on_the_device(golden, cuda_device, capsys):
    z = golden("repulsion")
    pcs, valids, w = z["pcs"], z["valids"], z["w"]
    for k, thre in enumerate(z["thre"]):
        r32, _ = _anchor(pcs, valids, float(thre), w)
        r64 = {"loss": torch.from_numpy(z["f64.loss"][k]), "grad": torch.from_numpy(z["f64.grad"][k])}
        x = T(pcs, cuda_device).requires_grad_()
        loss = L.repulsion_cd_loss(x, T(valids, cuda_device), float(thre), fused=True)
        (g,) = torch.autograd.grad((loss * T(w, cuda_device)).sum(), x)
        anchored.assert_anchored({"loss": loss.detach(), "grad": g}, r32, r64, f"repulsion record thre={thre:g}", capsys)
        ref = {"loss": torch.from_numpy(z["ref.loss"][k]), "grad": torch.from_numpy(z["ref.grad"][k])}
        assert anchored.err(ref["loss"], r64["loss"]) <= 1e-5 and anchored.err(ref["grad"], r64["grad"]) <= 1e-5


def test_captured_call_equals_eager(cuda_device):
    dev = cuda_device
    pcs, valids = make_case(77, B=3, P=4, N=130, spread=0.15)
    valids[2, 0] = 0
    x, v = T(pcs, dev).requires_grad_(), T(valids, dev)
    w = torch.tensor([1.0, 0.5, 2.0], device=dev)

    def run():
        loss = L.repulsion_cd_loss(x, v, 0.07, fused=True)
        (g,) = torch.autograd.grad((loss * w).sum(), x)
        return loss.detach(), g

    eager = [t.clone() for t in run()]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for t in out:
        t.fill_(7.0)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    assert float(eager[1].abs().max()) > 0


def test_refusals_fall_back_to_the_composition_with_one_warning(cuda_device, monkeypatch):
    monkeypatch.setattr(eval_utils, "_warned", set())
    dev = cuda_device
    pcs, valids = make_case(5, B=1, P=2, N=2049, size=0.1, spread=0.05)  # one point past the envelope
    x, v = T(pcs, dev), T(valids, dev)
    with pytest.warns(UserWarning, match="repulsion_cd_loss"):
        got = L.repulsion_cd_loss(x, v, 0.05, fused=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # once
        again, cd = L.repulsion_cd_loss(x.double(), v, 0.05, fused=True, ret_cd=True)  # (not float32: refused too)
        want = L.repulsion_cd_loss(x, v, 0.05)
    assert torch.equal(got, want) and torch.allclose(again.float(), want, rtol=1e-6) and cd.shape == (1, 2, 2)
    loss64, _, _ = rr.repulsion_cd(pcs, valids, 0.05, dtype=np.float64, prune=False)
    assert anchored.err(got, torch.from_numpy(loss64)) <= 1e-5


# ---- the term in a model step -----------------------------------------------------------------------------------------------
def _no_dropout(model):
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0


def _cfg(name, rot_type, term):
    cfg = getattr(config, name)()
    cfg.model.rot_type = rot_type
    cfg.data.max_num_part = 6
    cfg.optimizer.lr_scheduler = ""
    if "transformer_layers" in cfg.model:
        cfg.model.transformer_layers = 2
    if term == "on":
        cfg.loss.use_repulsion_loss, cfg.loss.repulsion_thre, cfg.loss.repulsion_loss_w = True, 0.05, 2.0
    elif term == "false":
        cfg.loss.use_repulsion_loss = False
    return cfg


def _trainer(name, rot_type, term, dev, **kw):
    cfg = _cfg(name, rot_type, term)
    torch.manual_seed(3)
    model = build_model(cfg).to(dev)
    _no_dropout(model)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return Trainer(model, cfg, **kw)


def _batch(dev, seed=5):
    return synthetic.make_batch(4, max_parts=6, num_points=256, seed=seed, device=dev)


STEPS = [(name, rot) for name in ("pn_transformer_everyday", "dgl_everyday") for rot in ("quat", "rmat")]


@pytest.mark.parametrize("name,rot_type", STEPS)
def test_step_terms_equal_the_composed_branch(cuda_device, name, rot_type, capsys):
    """forward_pass with the term on: every loss term of the fused branch against the composed branch (fused_loss = False)
    of a twin model; the repulsion term of both against the float64 restatement on the posed prediction, under the bars."""
    dev = cuda_device
    batch = _batch(dev)
    res = {}
    for fused in (True, False):
        model = _trainer(name, rot_type, "on", dev).model
        model.fused_loss = fused
        model.train()
        torch.manual_seed(11)
        res[fused] = {k: v.detach() for k, v in model.forward_pass(batch, mode="train").items()}
    assert list(res[True]) == list(res[False]) and "repulsion_loss" in res[True]
    keys = list(res[True])
    assert keys.index("repulsion_loss") == 1 + max(keys.index(k) for k in L.LOSS_TERMS)  # right behind the existing terms
    for k in res[True]:
        a, b = float(res[True][k]), float(res[False][k])
        assert abs(a - b) <= anchored.CEIL * abs(b), (k, a, b)
    # the term itself on one posed prediction
    model = _trainer(name, rot_type, "on", dev).model.train()
    if name.startswith("pn_"):  # (one prediction per forward; the graph network returns one per iteration)
        with torch.no_grad():
            pred = model.forward(batch)
        posed = transform_pc(pred["trans"], pred["rot"], batch["part_pcs"])
        valids = batch["part_valids"].cpu().numpy()
        l32, _, _ = rr.repulsion_cd(posed.cpu().numpy(), valids, 0.05)
        l64, _, _ = rr.repulsion_cd(posed.cpu().numpy(), valids, 0.05, dtype=np.float64, prune=False)
        r32, r64 = {"loss": torch.from_numpy(l32)}, {"loss": torch.from_numpy(l64)}
        for fused in (True, False):
            got = L.repulsion_cd_loss(posed, batch["part_valids"], 0.05, fused=fused)
            anchored.assert_anchored({"loss": got}, r32, r64, f"{name} {rot_type} term fused={fused}", capsys)


@pytest.mark.parametrize("name,rot_type", STEPS)
def test_captured_step_with_the_term_equals_eager(cuda_device, name, rot_type):
    batch = _batch(cuda_device, seed=8)
    eager = _trainer(name, rot_type, "on", cuda_device)
    graph = _trainer(name, rot_type, "on", cuda_device, use_graph=True, graph_warmup=1)
    for _ in range(3):
        le, lg = eager.train_step(batch), graph.train_step(batch)
        assert float(lg) == float(le)
    assert graph._graph is not None
    assert torch.equal(graph.flat.flat_param, eager.flat.flat_param)


@pytest.mark.parametrize("name,rot_type", STEPS)
def test_term_off_is_bit_equal_to_a_model_without_the_keys(cuda_device, name, rot_type):
    batch = _batch(cuda_device, seed=9)
    plain, off, on = (_trainer(name, rot_type, t, cuda_device) for t in ("absent", "false", "on"))
    for _ in range(2):
        lp, lo, ln = (t.train_step(batch) for t in (plain, off, on))
        assert float(lp) == float(lo)
    assert torch.equal(plain.flat.flat_param, off.flat.flat_param)
    assert float(ln) != float(lp) and not torch.equal(on.flat.flat_param, plain.flat.flat_param)  # the term does act
    keys = lambda t: list(t.model.train().forward_pass(batch, mode="train"))
    assert keys(plain) == keys(off) and "repulsion_loss" not in keys(plain) and "repulsion_loss" in keys(on)


def test_semantic_min_of_n_step_carries_the_term(cuda_device):
    """A semantic model (matching + min-of-5 sampling): the term is one more `[sample_iter, B]` row of the weighted total."""
    dev = cuda_device

    def trainer(term):
        cfg = config.dgl_partnet_chair()
        cfg.data.max_num_part = 3
        cfg.optimizer.lr_scheduler = ""
        if term:
            cfg.loss.use_repulsion_loss, cfg.loss.repulsion_thre, cfg.loss.repulsion_loss_w = True, 0.05, 2.0
        torch.manual_seed(3)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return cfg, Trainer(build_model(cfg).to(dev), cfg)

    cfg, on = trainer(True)
    _, off = trainer(False)
    batch = synthetic.make_semantic_batch(4, 3, 128, seed=5, device=dev, num_part_category=cfg.data.num_part_category)
    assert on.model.sample_iter == 5
    on.model.train()
    torch.manual_seed(1)
    res = on.model.forward_pass(batch, mode="train")
    off.model.train()
    torch.manual_seed(1)
    ref = off.model.forward_pass(batch, mode="train")
    assert "repulsion_loss" in res and "repulsion_loss" not in ref
    assert torch.isfinite(res["loss"]).item() and float(res["repulsion_loss"].detach()) > 0
    loss = on.train_step(batch)
    assert torch.isfinite(loss).item() and torch.isfinite(on.flat.flat_grad).all().item()


def test_benchmark_shape_once(cuda_device):
    """B = 32 x P = 20 x N = 1000, the benchmark's synthetic batch posed by its ground truth: the fused loss against the
    composition on the device (the float32 bar of the project, 1e-4), two runs bit-identical, gradient finite."""
    dev = cuda_device
    batch = synthetic.make_batch(32, max_parts=20, num_points=1000, seed=1234, device=dev)
    posed = transform_pc(batch["part_trans"], batch["part_quat"], batch["part_pcs"], "quat").detach()
    v = batch["part_valids"]
    cd = L.repulsion_cd_loss(posed, v, 1.0, ret_cd=True)[1]
    pair = (v[:, :, None] * v[:, None, :]).bool() & ~torch.eye(20, dtype=torch.bool, device=dev)
    thre = float(cd[pair].median())  # about half of the valid pairs are hinged
    x = posed.clone().requires_grad_()
    got = L.repulsion_cd_loss(x, v, thre, fused=True)
    (g,) = torch.autograd.grad(got.sum(), x)
    y = posed.clone().requires_grad_()
    want = L.repulsion_cd_loss(y, v, thre)
    (gw,) = torch.autograd.grad(want.sum(), y)
    gw = gw * v[:, :, None, None]
    assert anchored.err(got, want.double()) <= anchored.CEIL and anchored.err(g, gw.double()) <= anchored.CEIL
    again = L.repulsion_cd_loss(x, v, thre, fused=True)
    (g2,) = torch.autograd.grad(again.sum(), x)
    assert torch.equal(again, got) and torch.equal(g2, g) and torch.isfinite(g).all()
