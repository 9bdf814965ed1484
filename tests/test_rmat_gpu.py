"""rot_type='rmat' on the MI355X: the conversion and transform kernels of csrc/rmat.hip, the 6D pose head, the matrix
form of the device-side part matching, and training steps of every model with the 6D rotation head."""
import warnings

import numpy as np
import pytest
import torch

from multi_part_assembly_amd import config, synthetic
from multi_part_assembly_amd import loss as L
from multi_part_assembly_amd.loss import geometric_assembly_loss
from multi_part_assembly_amd.matching import match_parts
from multi_part_assembly_amd.pn_transformer import build_model
from multi_part_assembly_amd.regressor import PoseRegressor
from multi_part_assembly_amd.rotation import Rotation3D, normalize_rot6d, quat_to_matrix, rot6d_to_matrix
from multi_part_assembly_amd.trainer import Trainer
from multi_part_assembly_amd.transforms import pose_apply_rmat, transform_pc

pytestmark = pytest.mark.gpu


def _unit_quats(n, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(n, 4, generator=g)
    return q / q.norm(dim=-1, keepdim=True)


def test_quat_to_rmat_bit_equal_to_definition(cuda_device):
    q = _unit_quats(1000, 1) * 1.3  # (no normalisation: a non-unit quaternion scales, as in pytorch3d)
    got = quat_to_matrix(q.to(cuda_device)).cpu()
    assert torch.equal(got, quat_to_matrix(q))


def test_rot6d_to_rmat_forward_and_backward(cuda_device):
    g = torch.Generator().manual_seed(2)
    a = torch.randn(777, 6, generator=g)
    a[0, :3] = 0.0  # |a1| below eps: F.normalize's clamp
    got = rot6d_to_matrix(a.to(cuda_device)).cpu()
    np.testing.assert_allclose(got.numpy(), rot6d_to_matrix(a).numpy(), atol=2e-6)
    a64 = a.double().requires_grad_()
    b = normalize_rot6d(a64)
    want = torch.stack((b[:, :3], b[:, 3:], torch.cross(b[:, :3], b[:, 3:], dim=-1)), dim=-2)
    w = torch.randn(777, 3, 3, generator=g, dtype=torch.float64)
    (want * w).sum().backward()
    ad = a.to(cuda_device).requires_grad_()
    (rot6d_to_matrix(ad) * w.float().to(cuda_device)).sum().backward()
    np.testing.assert_allclose(ad.grad.cpu().numpy()[1:], a64.grad.numpy()[1:], rtol=1e-4, atol=1e-5)


def test_pose_apply_rmat_bit_exact_and_gradients(cuda_device):
    g = torch.Generator().manual_seed(3)
    M, N = 37, 301
    pc = torch.randn(M, N, 3, generator=g)
    r = rot6d_to_matrix(torch.randn(M, 6, generator=g))
    t = torch.randn(M, 3, generator=g)
    mask = (torch.rand(M, generator=g) > 0.3).float()
    # the reference's `(r @ v[..., None])` evaluated left to right, then + t
    x, y, z = pc.unbind(-1)
    rows = [(r[:, i, 0, None] * x + r[:, i, 1, None] * y) + r[:, i, 2, None] * z for i in range(3)]
    want = torch.stack(rows, -1) + t[:, None]
    got = pose_apply_rmat(pc.to(cuda_device), r.to(cuda_device), t.to(cuda_device)).cpu()
    assert torch.equal(got, want)
    np.testing.assert_allclose(got.numpy(), (r[:, None] @ pc[..., None]).squeeze(-1).add(t[:, None]).numpy(), atol=1e-5)
    # masked parts: points replaced by the fill before the transform
    got = pose_apply_rmat(pc.to(cuda_device), r.to(cuda_device), t.to(cuda_device), mask=mask.to(cuda_device),
                          fill=1e3).cpu()
    filled = torch.where(mask[:, None, None] == 0, torch.full_like(pc, 1e3), pc)
    np.testing.assert_allclose(got.numpy(), ((r[:, None] @ filled[..., None]).squeeze(-1) + t[:, None]).numpy(),
                               rtol=1e-6, atol=1e-3)
    # backward vs float64 autograd of the definition
    w = torch.randn(M, N, 3, generator=g, dtype=torch.float64)
    p64, r64, t64 = (v.double().requires_grad_() for v in (pc, r, t))
    m64 = mask.double()[:, None, None]
    ((r64[:, None] @ p64[..., None]).squeeze(-1) + t64[:, None]).mul(w).sum().backward()
    pd, rd, td = (v.to(cuda_device).requires_grad_() for v in (pc, r, t))
    (pose_apply_rmat(pd, rd, td) * w.float().to(cuda_device)).sum().backward()
    np.testing.assert_allclose(rd.grad.cpu().numpy(), r64.grad.numpy(), rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(td.grad.cpu().numpy(), t64.grad.numpy(), rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(pd.grad.cpu().numpy(), p64.grad.numpy(), rtol=1e-4, atol=1e-5)
    pd.grad = None
    (pose_apply_rmat(pd, rd, td, mask=mask.to(cuda_device)) * w.float().to(cuda_device)).sum().backward()
    np.testing.assert_allclose(pd.grad.cpu().numpy(), (p64.grad * m64).numpy(), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("M,F", [(640, 256), (640, 135), (96, 137), (333, 160)])
def test_pose_head_6d_matches_float64_library(cuda_device, M, F):
    torch.manual_seed(M + F)
    head = PoseRegressor(F, rot_type="rmat").to(cuda_device)
    assert head.native and tuple(head.rot_head.weight.shape) == (6, 128)
    x = torch.randn(M, F, device=cuda_device, requires_grad=True)
    rot, trans = head(x)
    w_r = torch.randn(M, 6, device=cuda_device)
    w_t = torch.randn(M, 3, device=cuda_device)
    ((rot * w_r).sum() + (trans * w_t).sum()).backward()
    ref = {k: v.detach().cpu().double().requires_grad_() for k, v in head.state_dict().items()}
    x64 = x.detach().cpu().double().requires_grad_()
    lrelu = torch.nn.functional.leaky_relu
    h = lrelu(x64 @ ref["fc_layers.0.weight"].T + ref["fc_layers.0.bias"], 0.2)
    h = lrelu(h @ ref["fc_layers.2.weight"].T + ref["fc_layers.2.bias"], 0.2)
    rot64 = normalize_rot6d(h @ ref["rot_head.weight"].T + ref["rot_head.bias"])
    trans64 = h @ ref["trans_head.weight"].T + ref["trans_head.bias"]
    ((rot64 * w_r.cpu().double()).sum() + (trans64 * w_t.cpu().double()).sum()).backward()
    np.testing.assert_allclose(rot.detach().cpu().numpy(), rot64.detach().numpy(), atol=1e-4)
    np.testing.assert_allclose(trans.detach().cpu().numpy(), trans64.detach().numpy(), rtol=1e-3, atol=1e-4)
    rel = lambda a, b: np.abs(a - b).max() / (np.abs(b).max() + 1e-12)
    assert rel(x.grad.cpu().numpy(), x64.grad.numpy()) < 2e-3
    for k, p in head.named_parameters():
        assert rel(p.grad.cpu().numpy(), ref[k].grad.numpy()) < 2e-3, k


def test_match_parts_rmat_matches_quaternion_matching(cuda_device):
    """The same poses as quaternions and as matrices: the same assignment, and the matched GT rotations are the
    permuted GT matrices."""
    B, P, N, G, n = 4, 8, 300, 3, 100
    g = torch.Generator().manual_seed(9)
    pcs = torch.randn(B, P, N, 3, generator=g).to(cuda_device)
    tq = torch.randn(B, P, 3, generator=g).mul(0.1).to(cuda_device)
    tg = torch.randn(B, P, 3, generator=g).mul(0.1).to(cuda_device)
    q1, q2 = _unit_quats(B * P, 10).view(B, P, 4).to(cuda_device), _unit_quats(B * P, 11).view(B, P, 4).to(cuda_device)
    ids = torch.tensor([[1, 1, 1, 2, 2, 0, 3, 3]] * B, dtype=torch.int32, device=cuda_device)
    idx = torch.stack([torch.stack([torch.randperm(N, generator=g)[:n] for _ in range(G)]) for _ in range(B)])
    idx = idx.to(torch.int32).to(cuda_device)
    r1, r2 = quat_to_matrix(q1), quat_to_matrix(q2)
    _, _, perm_q, cost_q, _ = match_parts(pcs, tq, q1, tg, q2, ids, idx, ret_aux=True)
    new_t, new_r, perm_r, cost_r, _ = match_parts(pcs, tq, r1, tg, r2, ids, idx, ret_aux=True)
    for grp, c in enumerate((3, 2, 2)):  # (only the members' block of a group's cost matrix is written)
        np.testing.assert_allclose(cost_r[:, grp, :c, :c].cpu().numpy(), cost_q[:, grp, :c, :c].cpu().numpy(),
                                   rtol=1e-4, atol=1e-6)
    assert torch.equal(perm_r, perm_q)
    rows = perm_r.long() + torch.arange(B, device=cuda_device)[:, None] * P
    assert torch.equal(new_r, r2.reshape(-1, 3, 3)[rows.flatten()].view(B, P, 3, 3))
    assert torch.equal(new_t, tg.reshape(-1, 3)[rows.flatten()].view(B, P, 3))


def _no_dropout(model):
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0


def _small(name, rot_type="rmat"):
    cfg = getattr(config, name)()
    cfg.model.rot_type = rot_type
    cfg.data.max_num_part = 6 if cfg.data.dataset == "geometry" else 2
    if "transformer_layers" in cfg.model:
        cfg.model.transformer_layers = 2
    return cfg


def _batch(cfg, dev, B=4, N=256, seed=5):
    if cfg.data.dataset != "geometry":  # identical parts: the matching has a group to permute
        return synthetic.make_semantic_batch(B, cfg.data.max_num_part, N, seed=seed, device=dev,
                                             num_part_category=cfg.data.num_part_category)
    return synthetic.make_batch(B, max_parts=cfg.data.max_num_part, num_points=N, seed=seed, device=dev)


def test_rmat_loss_terms_equal_the_quaternion_terms(cuda_device):
    """The pose terms do not depend on how a rotation is written: a PNTransformer's rmat terms equal the fused
    quaternion loss evaluated on the same rotations converted to quaternions (rot_loss has its own definition)."""
    cfg = _small("pn_transformer_everyday")
    torch.manual_seed(0)
    model = build_model(cfg).to(cuda_device)
    _no_dropout(model)
    model.train()
    batch = _batch(cfg, cuda_device)
    out = model.forward_pass(batch, mode="train")
    with torch.no_grad():
        pred = model.forward(batch)
    q = pred["rot"].convert("quat")
    terms, _ = geometric_assembly_loss(batch["part_pcs"], pred["trans"], q, batch["part_trans"],
                                       Rotation3D(batch["part_quat"], "quat"), batch["part_valids"], training=True)
    for k in ("trans_loss", "rot_pt_cd_loss", "transform_pt_cd_loss", "rot_pt_l2_loss"):
        np.testing.assert_allclose(float(out[k].detach()), float(terms[k].mean()), rtol=2e-4, atol=1e-6, err_msg=k)


MODELS = ["pn_transformer_everyday", "pn_transformer_refine_everyday", "dgl_everyday", "rgl_net_everyday",
          "global_everyday", "global_partnet_chair", "lstm_everyday"]


@pytest.mark.parametrize("name", MODELS)
def test_every_model_takes_a_finite_rmat_step(cuda_device, name):
    cfg = _small(name)
    cfg.optimizer.lr_scheduler = ""
    torch.manual_seed(1)
    model = build_model(cfg).to(cuda_device)
    _no_dropout(model)
    model.train()
    batch = _batch(cfg, cuda_device)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        trainer = Trainer(model, cfg)
    before = trainer.flat.flat_param.clone()
    loss = trainer.train_step(batch)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()
    g = trainer.flat.flat_grad
    assert torch.isfinite(g).all().item() and float(g.abs().sum()) > 0
    assert not torch.equal(before, trainer.flat.flat_param)
    model.eval()
    with torch.no_grad():
        res = model.forward_pass(batch, mode="val")
    for k, v in res.items():
        if k != "batch_size":
            assert torch.isfinite(v).all().item(), k
    assert "part_acc" in res


def test_rmat_graph_replay_equals_eager(cuda_device):
    def fresh(**kw):
        cfg = _small("pn_transformer_everyday")
        cfg.optimizer.lr_scheduler = ""
        torch.manual_seed(2)
        model = build_model(cfg).to(cuda_device)
        _no_dropout(model)
        return Trainer(model, cfg, **kw)

    # (the fused matrix-form loss has no atomics: the replay walks the eager trajectory bit for bit)
    batch = _batch(_small("pn_transformer_everyday"), cuda_device, seed=8)
    eager, graph = fresh(), fresh(use_graph=True, graph_warmup=1)
    for _ in range(4):
        le = eager.train_step(batch)
        lg = graph.train_step(batch)
        assert float(lg) == float(le)
    assert graph._graph is not None  # steps 2.. were replays
    assert torch.equal(graph.flat.flat_param, eager.flat.flat_param)


def test_rmat_transform_pc_through_rotation3d(cuda_device):
    g = torch.Generator().manual_seed(4)
    d6 = torch.randn(2, 3, 6, generator=g).to(cuda_device)
    rot = Rotation3D(d6, "rmat")
    pc = torch.randn(2, 3, 50, 3, generator=g).to(cuda_device)
    t = torch.randn(2, 3, 3, generator=g).to(cuda_device)
    got = transform_pc(t, rot, pc)
    want = (rot.rot[:, :, None] @ pc[..., None]).squeeze(-1) + t[:, :, None]
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), atol=1e-5)


# ---- the fused five-term loss in matrix form (csrc/assembly_loss.hip, mpa_assembly_loss_*_rmat) --------------------------------
def _full_size_rmat(cuda_device):
    B, P, N = 32, 20, 1000
    batch = synthetic.make_batch(B, P, N, preset="everyday", seed=1234, device=cuda_device)
    g = torch.Generator().manual_seed(99)
    d6 = torch.randn(B, P, 6, generator=g).to(cuda_device)
    tp = (torch.randn(B, P, 3, generator=g) * 0.3).to(cuda_device)
    w = (torch.rand(5, B, generator=g) + 0.5).to(cuda_device)
    gt = Rotation3D(batch["part_quat"]).convert("rmat")
    return batch, d6, tp, w, gt


def _fused_rmat(batch, d6, tp, w, gt, fused=True):
    d = d6.clone().requires_grad_()
    t = tp.clone().requires_grad_()
    rot = Rotation3D(d, "rmat")
    pcs, v = batch["part_pcs"], batch["part_valids"]
    if fused:
        terms, _ = geometric_assembly_loss(pcs, t, rot, batch["part_trans"], gt, v, training=True)
    else:  # the per-function composition (pose_apply_rmat + the Chamfer operator + library reductions)
        terms = {"trans_loss": L.trans_l2_loss(t, batch["part_trans"], v),
                 "rot_pt_cd_loss": L.rot_points_cd_loss(pcs, rot, gt, v),
                 "transform_pt_cd_loss": L.shape_cd_loss(pcs, t, batch["part_trans"], rot, gt, v, training=True),
                 "rot_loss": L.rot_cosine_loss(rot, gt, v),
                 "rot_pt_l2_loss": L.rot_points_l2_loss(pcs, rot, gt, v)}
    sum((terms[k] * w[i]).sum() for i, k in enumerate(L.LOSS_TERMS)).backward()
    return torch.stack([terms[k].detach() for k in L.LOSS_TERMS]), d.grad, t.grad


def test_fused_rmat_loss_equals_composition_and_is_deterministic(cuda_device):
    """B = 32, P = 20, N = 1000: the five terms of the fused matrix-form loss equal the per-function composition, and so
    do the gradients (through the 6D conversion); two runs are bit-equal."""
    batch, d6, tp, w, gt = _full_size_rmat(cuda_device)
    lf, gdf, gtf = _fused_rmat(batch, d6, tp, w, gt)
    lc, gdc, gtc = _fused_rmat(batch, d6, tp, w, gt, fused=False)
    for i, k in enumerate(L.LOSS_TERMS):
        np.testing.assert_allclose(lf[i].cpu().numpy(), lc[i].cpu().numpy(), rtol=2e-5, atol=1e-8, err_msg=k)
    assert float((gdf - gdc).abs().max()) < 1e-4 * float(gdc.abs().max())
    assert float((gtf - gtc).abs().max()) < 1e-4 * float(gtc.abs().max())
    lf2, gdf2, gtf2 = _fused_rmat(batch, d6, tp, w, gt)
    assert torch.equal(lf, lf2) and torch.equal(gdf, gdf2) and torch.equal(gtf, gtf2)


def _raw_rmat_forward(batch, rp, tp, gt, mode, part, monkeypatch):
    import ctypes
    from multi_part_assembly_amd import _lib

    monkeypatch.setenv("MPA_SHAPE_SEARCH", mode)
    monkeypatch.setenv("MPA_PART_SEARCH", part)
    pcs, v = batch["part_pcs"], batch["part_valids"]
    B, P, N, _ = pcs.shape
    lib = _lib.lib()
    nf, ni = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(lib.mpa_assembly_loss_workspace(B, P, N, ctypes.byref(nf), ctypes.byref(ni)), "ws")
    fws = torch.full((nf.value,), float("nan"), device=pcs.device)  # poisoned: nothing may depend on old contents
    iws = torch.full((ni.value,), 0x7F7F7F7F, dtype=torch.int32, device=pcs.device)
    losses = torch.empty(5, B, device=pcs.device)
    tg = batch["part_trans"].contiguous()
    st = lib.mpa_assembly_loss_forward_rmat_ordered(_lib.ptr(pcs), _lib.ptr(v), _lib.ptr(rp), _lib.ptr(tp), _lib.ptr(gt),
                                                    _lib.ptr(tg), B, P, N, 1, 1, None, -1, _lib.ptr(fws), _lib.ptr(iws),
                                                    _lib.ptr(losses), None, _lib.current_stream(pcs.device))
    _lib.check(st, "mpa_assembly_loss_forward_rmat_ordered")
    torch.cuda.synchronize()
    pn, cloud = B * P * N, B * P * N * 3
    return losses, [iws[k * pn:(k + 1) * pn].view(B, P, N) for k in range(4)], fws[:4 * cloud].view(4, B, P, N, 3)


def test_fused_rmat_loss_argmins_equal_the_oracle_scan_under_every_route(cuda_device, monkeypatch):
    """The arg-mins of both Chamfer searches of the matrix-form loss are bit-equal to the C oracle's exhaustive scan run on
    the kernel's own transformed clouds, under every part-search route (gate, scan, leaves) and shape-search route
    (brute, grid, leaves, per-sample auto)."""
    from oracle import chamfer as oc

    batch, d6, tp, _, gt = _full_size_rmat(cuda_device)
    rp = rot6d_to_matrix(d6).contiguous()
    gtr = gt.rot.contiguous()
    valid = batch["part_valids"].bool()
    lb, ib, clouds = _raw_rmat_forward(batch, rp, tp.contiguous(), gtr, "brute", "scan", monkeypatch)
    for mode, part in (("brute", "gate"), ("grid", "gate"), ("grid", "scan"), ("leaf", "gate"), ("leaf", "scan"),
                       ("auto", "gate")):
        lm, im, _ = _raw_rmat_forward(batch, rp, tp.contiguous(), gtr, mode, part, monkeypatch)
        for k in range(4):
            assert torch.equal(ib[k][valid], im[k][valid]), (mode, part, k)
        np.testing.assert_allclose(lm.cpu().numpy(), lb.cpu().numpy(), rtol=2e-6, atol=1e-9, err_msg=f"{mode}/{part}")
    monkeypatch.delenv("MPA_PART_SEARCH", raising=False)
    monkeypatch.delenv("MPA_SHAPE_SEARCH", raising=False)
    B, P, N = valid.shape[0], valid.shape[1], clouds.shape[3]
    r1, r2, s1, s2 = (c.cpu() for c in clouds)
    vc = valid.cpu()
    # per-part Chamfer: each valid part against its own GT copy
    _, p1, _, p2 = oc.chamfer_forward(r1[vc].numpy(), r2[vc].numpy())
    assert torch.equal(ib[0].cpu()[vc].long(), torch.from_numpy(p1).long())
    assert torch.equal(ib[1].cpu()[vc].long(), torch.from_numpy(p2).long())
    # whole shapes (padded parts are the 1e3 fill, transformed)
    _, i1, _, i2 = oc.chamfer_forward(s1.flatten(1, 2).numpy(), s2.flatten(1, 2).numpy())
    assert torch.equal(ib[2].cpu()[vc].long(), torch.from_numpy(i1).view(B, P, N)[vc].long())
    assert torch.equal(ib[3].cpu()[vc].long(), torch.from_numpy(i2).view(B, P, N)[vc].long())
    # and the kernel's clouds are the library transform of the parts
    pcs = batch["part_pcs"]
    assert torch.equal(clouds[0][valid], pose_apply_rmat(pcs, rp)[valid])
    assert torch.equal(clouds[2][valid], pose_apply_rmat(pcs, rp, tp)[valid])


# ---- against records of the reference's own rmat path (tests/golden/make_golden_rmat.py) ---------------------------------------
def test_conversions_and_transform_match_the_reference_record(golden, cuda_device):
    z = golden("rmat_transforms")
    T = lambda k: torch.from_numpy(z[k].copy()).to(cuda_device)
    np.testing.assert_allclose(quat_to_matrix(T("quat")).cpu().numpy(), z["quat_rmat"], rtol=0, atol=1e-6)
    rot = Rotation3D(T("d6"), "rmat")
    np.testing.assert_allclose(rot.rot.cpu().numpy(), z["d6_rmat"], rtol=0, atol=1e-6)
    # the transform itself on the reference's own matrices: bit for bit
    got = pose_apply_rmat(T("pc"), T("d6_rmat"), T("trans")).cpu().numpy()
    assert np.array_equal(got, z["rmat_transform"])
    np.testing.assert_allclose(rot.to_euler().cpu().numpy(), z["to_euler"], atol=2e-3)


STEPS = {"pn_transformer_rmat_step": ("pn_transformer_everyday", 2e-3),
         "dgl_rmat_step": ("dgl_everyday", 5e-2),
         "global_rmat_semantic_step": ("global_partnet_chair", 2e-3)}


@pytest.mark.parametrize("name", sorted(STEPS))
def test_rmat_step_matches_the_reference(golden, cuda_device, name):
    """One training-mode forward_pass + backward against the reference's rmat step: every loss term to 1e-4, every
    parameter gradient within the bar of its model relative to the tensor's scale (the reference cannot evaluate its rmat
    path in float64, so the float32 record is the anchor; DGL's stacked BatchNorm MLPs leave float32 evaluations a few
    percent apart, see tests/test_callers_gpu.py)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import param_fill

    z = golden(name)
    preset, bar = STEPS[name]
    cfg = _small(preset)
    cfg.model.pc_feat_dim = int(z["cfg"][0])
    if preset == "pn_transformer_everyday":
        cfg.model.transformer_heads, cfg.model.transformer_feat_dim = int(z["cfg"][1]), int(z["cfg"][2])
        cfg.model.transformer_layers = int(z["cfg"][3])
    cfg.data.max_num_part = 5
    seed = int(z["seed"][0])
    torch.manual_seed(seed)
    model = build_model(cfg)
    assert sorted(model.state_dict().keys()) == [str(n) for n in z["names"]]
    param_fill.fill_parameters(model, seed)
    _no_dropout(model)
    model.to(cuda_device).train()
    data = {k[5:]: torch.from_numpy(z[k].copy()).to(cuda_device) for k in z if k.startswith("data.")}
    torch.manual_seed(seed + 1)
    res = model.forward_pass(data, mode="train")
    res["loss"].backward()
    for k in z:
        if k.startswith("loss."):
            np.testing.assert_allclose(float(res[k[5:]].detach()), float(z[k]), rtol=1e-4, atol=1e-6, err_msg=k)
    record = dict(z)
    for k, p in model.named_parameters():
        if ("grad." + k) in record or ("grad." + k + "#sample") in record:
            assert p.grad is not None, k
            # (floor: a bias in front of a BatchNorm has a gradient of rounding noise only)
            param_fill.compare(record, "grad.", k, p.grad.cpu().numpy(), rel=bar, floor=1e-3)
