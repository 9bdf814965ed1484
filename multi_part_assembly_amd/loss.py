"""Pose losses of the assembly training step — mirror of the reference's `utils/loss.py`
(multi_part_assembly/utils/loss.py:7-202), same names / arguments / [B] return shapes.

The heavy parts run on the HIP library: pose application (csrc/pose.hip) and the Chamfer searches
(csrc/chamfer.hip).  The O(B*P) reductions around them are a handful of torch ops on tiny tensors.
`rot1/rot2` are `Rotation3D` objects (quaternions or rotation matrices; the fused path takes quaternions).
"""
from __future__ import annotations

import torch

from . import _lib
from .chamfer import chamfer_distance
from .transforms import pose_apply, pose_apply_rmat, rot_pc

__all__ = ["geometric_assembly_loss", "part_order", "search_mode", "SEARCH_MODES", "LOSS_TERMS", "trans_l2_loss", "rot_l2_loss", "rot_cosine_loss", "rot_points_l2_loss",
           "rot_points_cd_loss", "shape_cd_loss", "repulsion_cd_loss", "repulsion_cd_search", "repulsion_supported"]

PAD_FILL = 1e3  # coordinate given to the points of padded parts in shape_cd_loss (loss.py:173-175)


def _valid_mean(loss_per_part, valids):
    """Mean over the valid parts of each sample: [B, P] x [B, P] -> [B]."""
    v = valids.float().detach()
    return (loss_per_part * v).sum(1) / v.sum(1)


def _quat(rot):
    if rot.rot_type != "quat":
        raise NotImplementedError(f"loss not supported for {rot.rot_type}")
    return rot.rot


def _pose_apply(pts, rot, trans, mask, fill):
    if rot.rot_type == "rmat":
        return pose_apply_rmat(pts, rot.rot, trans, mask=mask, fill=fill)
    return pose_apply(pts, _quat(rot), trans, mask=mask, fill=fill)


def trans_l2_loss(trans1, trans2, valids):
    """Squared L2 between translations, [B, P, 3] x2 -> [B]."""
    return _valid_mean((trans1 - trans2).square().sum(-1), valids)


def rot_l2_loss(rot1, rot2, valids):
    """min(|q1 - q2|^2, |q1 + q2|^2) since q and -q are the same rotation."""
    q1, q2 = _quat(rot1), _quat(rot2)
    per_part = torch.minimum((q1 - q2).square().sum(-1), (q1 + q2).square().sum(-1))
    return _valid_mean(per_part, valids)


def rot_cosine_loss(rot1, rot2, valids):
    """1 - |<q1, q2>| per part; for rotation matrices the mean of the squared entries of I - R1^T R2 (loss.py:76-82)."""
    if rot1.rot_type != rot2.rot_type:
        raise ValueError(f"rotation types differ: {rot1.rot_type} vs {rot2.rot_type}")
    if rot1.rot_type == "rmat":
        B = rot1.shape[0]
        r1, r2 = rot1.rot.reshape(-1, 3, 3), rot2.rot.reshape(-1, 3, 3)
        iden = torch.eye(3, dtype=r1.dtype, device=r1.device).unsqueeze(0)
        per_part = (iden - torch.bmm(r1.transpose(1, 2), r2)).pow(2).mean(dim=[-1, -2]).view(B, -1)
        return _valid_mean(per_part, valids)
    q1, q2 = _quat(rot1), _quat(rot2)
    return _valid_mean(1.0 - (q1 * q2).sum(-1).abs(), valids)


def rot_points_l2_loss(pts, rot1, rot2, valids, ret_pts=False):
    """Mean squared distance between the two rotated copies of each part's points."""
    pts1, pts2 = rot_pc(rot1, pts), rot_pc(rot2, pts)
    loss = _valid_mean((pts1 - pts2).square().sum(-1).mean(-1), valids)
    return (loss, pts1, pts2) if ret_pts else loss


def rot_points_cd_loss(pts, rot1, rot2, valids, ret_pts=False):
    """Per-part Chamfer distance between the two rotated copies: B*P searches of N x N."""
    B, P = pts.shape[:2]
    pts1, pts2 = rot_pc(rot1, pts), rot_pc(rot2, pts)
    dist1, dist2 = chamfer_distance(pts1.flatten(0, 1), pts2.flatten(0, 1))
    per_part = (dist1.mean(1) + dist2.mean(1)).view(B, P).type_as(pts)
    loss = _valid_mean(per_part, valids)
    return (loss, pts1, pts2) if ret_pts else loss


def shape_cd_loss(pts, trans1, trans2, rot1, rot2, valids, ret_pts=False, training=True):
    """Whole-shape Chamfer distance after applying both pose sets: B searches of (P*N) x (P*N).

    The points of padded parts are set to PAD_FILL before the transform so they never match a real
    point (done inside the pose kernel, no clone of `pts`); no gradient flows into `pts`.
    training=True divides by all P*N slots ("hard negative mining", reference loss.py:185-193),
    training=False averages per part and then over the valid parts (:194-198).
    """
    B, P, N, _ = pts.shape
    pts = pts.detach()
    pts1 = _pose_apply(pts, rot1, trans1, mask=valids, fill=PAD_FILL)
    pts2 = _pose_apply(pts, rot2, trans2, mask=valids, fill=PAD_FILL)
    dist1, dist2 = chamfer_distance(pts1.flatten(1, 2), pts2.flatten(1, 2))
    v = valids.float().detach()
    if training:
        slot = v[:, :, None].expand(B, P, N).reshape(B, P * N)
        loss = (dist1 * slot).mean(1) + (dist2 * slot).mean(1)
    else:
        loss = _valid_mean((dist1 + dist2).view(B, P, N).mean(-1), v)
    return (loss, pts1, pts2) if ret_pts else loss


def _repulsion_composed(part_pcs, valids, thre):
    """The reference's composition (loss.py:205-225): all P x P pairs through the Chamfer operator.  (loss [B], raw
    Chamfer distances [B, P, P]; the rows and columns of padded slots hold whatever their points give.)"""
    B, P, N, _ = part_pcs.shape
    a = part_pcs[:, :, None].expand(B, P, P, N, 3).reshape(-1, N, 3)
    b = part_pcs[:, None].expand(B, P, P, N, 3).reshape(-1, N, 3)
    dist1, dist2 = chamfer_distance(a.contiguous(), b.contiguous())
    raw = (dist1.mean(1) + dist2.mean(1)).view(B, P, P)
    cd = (thre - raw).clamp_min(0.0)
    pair = (valids[:, :, None] * valids[:, None, :]).type_as(cd)
    return (cd * pair).sum([1, 2]) / pair.sum([1, 2]), raw


def repulsion_supported(part_pcs):
    """The envelope of csrc/repulsion.hip (include/mpa_hip.h): float32 CUDA clouds [B, P, N, 3] with 1 <= N <= 2048,
    1 <= P <= 64 and B P P N < 2^31."""
    from . import repulsion_ref
    return (part_pcs.is_cuda and part_pcs.dtype == torch.float32 and part_pcs.dim() == 4 and part_pcs.shape[3] == 3
            and 1 <= part_pcs.shape[2] <= repulsion_ref.MAX_POINTS and 1 <= part_pcs.shape[1] <= repulsion_ref.MAX_PARTS
            and part_pcs.shape[0] * part_pcs.shape[1] ** 2 * part_pcs.shape[2] < 2 ** 31)


class _RepulsionCD(torch.autograd.Function):
    """The repulsion loss over the unordered pairs of valid parts: two launches forward, one backward (csrc/repulsion.hip).
    The workspace carries the pair flags and the 16-bit arg-min lists from the forward to the backward."""

    @staticmethod
    def forward(ctx, part_pcs, valids, thre, ret_cd):
        B, P, N, _ = part_pcs.shape
        dev = part_pcs.device
        nbytes = _lib.query("mpa_repulsion_cd_workspace", B, P, N)[0]
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        cd = torch.empty((B, P, P), dtype=torch.float32, device=dev) if ret_cd else None
        _lib.launch("mpa_repulsion_cd_forward", dev, part_pcs, valids, thre, B, P, N, ws, loss, cd, None,
                    timer=f"repulsion_cd_forward[{B}x{P}x{N}]")
        ctx.save_for_backward(part_pcs, valids, ws)
        ctx.set_materialize_grads(False)
        if cd is None:
            return loss, None
        ctx.mark_non_differentiable(cd)
        return loss, cd

    @staticmethod
    def backward(ctx, grad_loss, _grad_cd):
        if grad_loss is None:
            return None, None, None, None
        part_pcs, valids, ws = ctx.saved_tensors
        B, P, N, _ = part_pcs.shape
        grad = torch.empty_like(part_pcs)
        _lib.launch("mpa_repulsion_cd_backward", part_pcs.device, grad_loss.to(torch.float32).contiguous(), part_pcs, valids,
                    B, P, N, ws, grad, timer=f"repulsion_cd_backward[{B}x{P}x{N}]")
        return grad, None, None, None


@torch.no_grad()
def repulsion_cd_search(part_pcs, valids, thre, ret_cd=False, out=None):
    """What `mpa_repulsion_cd_forward` leaves behind, for tests and tools: a dict with loss [B], flag [B, P (P - 1) / 2]
    uint8 (0 not searched, 1 searched, 2 hinged), idx1 / idx2 [B, slots, N] int32 (-1 for none; rows of pairs that were not
    searched are unwritten), dist1 / dist2 [B, slots, N] and, with `ret_cd`, cd [B, P, P].  `out`: a dict of preallocated
    `loss`, `workspace`, `dists` (and `cd`) tensors to write into, as an earlier call returned them."""
    if not repulsion_supported(part_pcs):
        raise ValueError(f"repulsion_cd_search: {tuple(part_pcs.shape)} {part_pcs.dtype} {part_pcs.device.type} clouds are "
                         "outside csrc/repulsion.hip")
    import numpy as np
    B, P, N, _ = part_pcs.shape
    dev, slots = part_pcs.device, P * (P - 1) // 2
    nbytes, o_flag, o_idx1, o_idx2 = _lib.query("mpa_repulsion_cd_workspace", B, P, N)
    out = dict(out or {})
    ws = out.get("workspace")
    if ws is None:
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    loss = out.get("loss")
    if loss is None:
        loss = torch.empty(B, dtype=torch.float32, device=dev)
    dists = out.get("dists")
    if dists is None:
        dists = torch.empty((B, slots, 2, N), dtype=torch.float32, device=dev)
    cd = out.get("cd") if ret_cd else None
    if ret_cd and cd is None:
        cd = torch.empty((B, P, P), dtype=torch.float32, device=dev)
    _lib.launch("mpa_repulsion_cd_forward", dev, part_pcs.contiguous(), valids.to(torch.float32).contiguous(),
                float(np.float32(thre)), B, P, N, ws, loss, cd, dists)
    lists = lambda off: ws[off:off + 2 * B * slots * N].view(torch.int16).view(B, slots, N).to(torch.int32)
    res = {"loss": loss, "flag": ws[o_flag:o_flag + B * slots].view(B, slots), "idx1": lists(o_idx1), "idx2": lists(o_idx2),
           "dist1": dists[:, :, 0], "dist2": dists[:, :, 1], "workspace": ws, "dists": dists}
    if ret_cd:
        res["cd"] = cd
    return res


class _RepulsionHost(torch.autograd.Function):
    """The float32 restatement (repulsion_ref.py) for host tensors."""

    @staticmethod
    def forward(ctx, part_pcs, valids, thre, ret_cd):
        from . import repulsion_ref
        loss, cd, _ = repulsion_ref.repulsion_cd(part_pcs.detach().numpy(), valids.detach().numpy(), thre, prune=not ret_cd)
        ctx.save_for_backward(part_pcs, valids)
        ctx.thre, ctx.prune = thre, not ret_cd
        ctx.set_materialize_grads(False)
        if not ret_cd:
            return torch.from_numpy(loss), None
        cd = torch.from_numpy(cd)
        ctx.mark_non_differentiable(cd)
        return torch.from_numpy(loss), cd

    @staticmethod
    def backward(ctx, grad_loss, _grad_cd):
        if grad_loss is None:
            return None, None, None, None
        from . import repulsion_ref
        part_pcs, valids = ctx.saved_tensors
        grad = repulsion_ref.repulsion_cd_grad(part_pcs.detach().numpy(), valids.detach().numpy(), ctx.thre,
                                               grad_loss.detach().numpy(), prune=ctx.prune)
        return torch.from_numpy(grad), None, None, None


def repulsion_cd_loss(part_pcs, valids, thre, fused=False, ret_cd=False):
    """max(0, thre - CD(part_i, part_j)) averaged over the valid pairs of every sample, [B, P, N, 3] posed clouds -> [B]
    (reference loss.py:205-225): pushes apart parts that sit inside each other.

    fused=False is the reference's composition: the batch expanded to two [B P P, N, 3] tensors and one Chamfer call over
    all P x P pairs.  fused=True runs csrc/repulsion.hip: one block per unordered pair of valid parts, pairs whose bounding
    boxes are at least `thre` apart not searched, nothing expanded; the values are those of `repulsion_ref` (the same
    nearest neighbours as the composition, bit for bit; the sums in another order), the gradient flows to `part_pcs`.
    Float32 CUDA clouds with N <= 2048 and P <= 64; anything else leaves the kernel with one warning -- CUDA tensors for
    the composition, host tensors for the numpy restatement.  `ret_cd`: also the Chamfer distances [B, P, P] (no gradient);
    the fused path writes 0 on the diagonal and for pairs with a padded member, and then searches every valid pair."""
    if part_pcs.dim() != 4 or part_pcs.shape[-1] != 3 or tuple(valids.shape) != tuple(part_pcs.shape[:2]):
        raise ValueError(f"repulsion_cd_loss: part_pcs must be [B, P, N, 3] and valids [B, P], got "
                         f"{tuple(part_pcs.shape)} and {tuple(valids.shape)}")
    if fused and not repulsion_supported(part_pcs):
        from .eval_utils import _warn_once
        from . import repulsion_ref
        _warn_once("repulsion_cd_loss", f"{tuple(part_pcs.shape)} {part_pcs.dtype} {part_pcs.device.type} clouds are outside "
                   f"csrc/repulsion.hip (float32 CUDA, at most {repulsion_ref.MAX_POINTS} points per part and "
                   f"{repulsion_ref.MAX_PARTS} part slots)")
        if not part_pcs.is_cuda:
            import numpy as np
            loss, cd = _RepulsionHost.apply(part_pcs.float(), valids.detach().float(), float(np.float32(thre)), bool(ret_cd))
            return (loss, cd) if ret_cd else loss
        fused = False
    if fused:
        import numpy as np
        loss, cd = _RepulsionCD.apply(part_pcs.contiguous(), valids.detach().to(torch.float32).contiguous(),
                                      float(np.float32(thre)), bool(ret_cd))
        return (loss, cd) if ret_cd else loss
    loss, raw = _repulsion_composed(part_pcs, valids, thre)
    return (loss, raw.detach()) if ret_cd else loss


# ---- fused path ------------------------------------------------------------------------------------
LOSS_TERMS = ("trans_loss", "rot_pt_cd_loss", "transform_pt_cd_loss", "rot_loss", "rot_pt_l2_loss")


class LossTerms(dict):
    """{term name: [B]} that also carries the [K, B] tensor the terms are rows of (`stacked = (names, tensor)`):
    `BaseModel.loss_function` weights that tensor directly — selecting five rows and stacking them again costs
    ~15 small launches per step in autograd (five zero-filled [K, B] gradients, copies and adds)."""

    stacked = None


def sum_loss_rounds(per_round):
    """The terms of a model's rounds (GNN iterations, refinement steps), each a {name: [B]} with the same names -> the
    sums under `name`, then every round's own terms under `name_i`, round-major.  Where every round carries its terms as
    ONE [K, B] tensor (`LossTerms.stacked`, the fused loss) those are summed (rounds - 1 launches) and `loss_function`
    weights the [K (rounds + 1), B] concatenation directly — summing and re-stacking the terms one by one is ~100 small
    launches per step, forward and backward."""
    names = list(per_round[0])
    keys = names + [f"{k}_{i}" for i in range(len(per_round)) for k in names]
    stacks = [getattr(d, "stacked", None) for d in per_round]
    if all(st is not None and list(st[0]) == names for st in stacks):
        summed = stacks[0][1]
        for st in stacks[1:]:
            summed = summed + st[1]
        full = torch.cat([summed] + [st[1] for st in stacks], dim=0)
        total = LossTerms((k, full[j]) for j, k in enumerate(keys))
        total.stacked = (tuple(keys), full)
        return total
    total = {k: 0.0 for k in names}
    for i, loss_dict in enumerate(per_round):
        for k, v in loss_dict.items():
            total[k] = total[k] + v
            total[f"{k}_{i}"] = v
    return total


def part_order(part_pcs, valids):
    """The k-d order of a batch's parts that both Chamfer searches of the fused loss run on (csrc/leaf_nn.hip,
    `mpa_assembly_order`): a function of `part_pcs` and `valids` only — not of any pose — so ONE ordering serves every
    loss evaluation of a step (the GNN iterations of DGL / RGL-NET, the min-of-N samples, both directions).  Returns a
    float32 tensor to pass as `geometric_assembly_loss(..., order=...)`, or None where the loss keeps its grid search
    (N > 2048).  Only steers speed: the loss is bit-identical with or without it."""
    _lib.require_hip("part_order", part_pcs)
    B, P, N, _ = part_pcs.shape
    ne = _lib.query("mpa_assembly_order_elems", B, P, N)
    if ne == 0:
        return None
    pcs = part_pcs.detach().to(torch.float32).contiguous()
    v = valids.detach().to(torch.float32).contiguous()
    order = torch.empty(ne, dtype=torch.float32, device=pcs.device)
    _lib.launch("mpa_assembly_order", pcs.device, pcs, v, B, P, N, order)
    return order


class _AssemblyLoss(torch.autograd.Function):
    """All five geometric loss terms in 5 launches forward / 1 launch backward (csrc/assembly_loss.hip).  The rotations are
    quaternions [B,P,4] or rotation matrices [B,P,3,3] (the `_rmat` entry points)."""

    @staticmethod
    def forward(ctx, part_pcs, valids, quat_pred, trans_pred, quat_gt, trans_gt, training, fill_pads, order=None,
                search=-1):
        B, P, N, _ = part_pcs.shape
        dev = part_pcs.device
        nf, ni = _lib.query("mpa_assembly_loss_workspace", B, P, N)
        fws = torch.empty(nf, dtype=torch.float32, device=dev)
        iws = torch.empty(ni, dtype=torch.int32, device=dev)
        losses = torch.empty((5, B), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            # library-recorded events: [0..4] bound the four phases, [5] / [6] sit right around the grid search kernel
            tag = f"[{B}x{P}x{N}]"
            names = [k + tag for k in ("assembly_pose", "assembly_part_chamfer", "assembly_shape_chamfer",
                                       "assembly_finalize")]
            evs = _lib.KernelTimer.phase_events(names)
            gs = _lib.KernelTimer.phase_events(["shape_search_kernel" + tag])
            both = None
            if evs is not None or gs is not None:
                both = (evs if evs is not None else [None] * 5) + (gs if gs is not None else [None] * 2)
            _lib.launch(
                "mpa_assembly_loss_forward_rmat_ordered" if quat_pred.dim() == 4 else "mpa_assembly_loss_forward_ordered",
                dev, part_pcs, valids, quat_pred, trans_pred, quat_gt, trans_gt, B, P, N, training, fill_pads,
                order, int(search), fws, iws, losses, _lib.KernelTimer.handles(both))
            _lib.KernelTimer.add_phases(names, evs)
            _lib.KernelTimer.add_phases(["shape_search_kernel" + tag], gs)
        ctx.save_for_backward(part_pcs, valids, quat_pred, trans_pred, quat_gt, trans_gt, fws, iws)
        ctx.training = int(training)
        cloud = B * P * N * 3
        pts = fws[: 4 * cloud].view(4, B, P, N, 3)
        ctx.mark_non_differentiable(pts)
        ctx.set_materialize_grads(False)   # else every backward zero-fills a [4, B, P, N, 3] "gradient" for pts
        return losses, pts

    @staticmethod
    def backward(ctx, grad_losses, _grad_pts):
        if getattr(ctx, "consumed", False):
            raise RuntimeError("assembly loss: the backward pass reuses the forward's tile-sum area as scratch: a second "
                               "backward over the same forward (retain_graph=True) is not supported — run the forward again")
        if grad_losses is None:
            return (None,) * 10
        ctx.consumed = True
        part_pcs, valids, quat_pred, trans_pred, quat_gt, trans_gt, fws, iws = ctx.saved_tensors
        B, P, N, _ = part_pcs.shape
        dev = part_pcs.device
        gq = torch.empty_like(quat_pred)
        gt = torch.empty_like(trans_pred)
        grad_losses = grad_losses.contiguous()
        _lib.launch("mpa_assembly_loss_backward_rmat" if quat_pred.dim() == 4 else "mpa_assembly_loss_backward", dev,
                    grad_losses, part_pcs, valids, quat_pred, trans_pred, quat_gt, trans_gt, B, P, N, ctx.training,
                    fws, iws, gq, gt)
        return None, None, gq, gt, None, None, None, None, None, None


SEARCH_MODES = {"brute": 0, "grid": 1, "leaf": 2, "auto": 3}


class _LossReduce(torch.autograd.Function):
    """loss = sum_k w_k mean_b terms[k, b] and the per-term means, one launch each way (csrc/pose.hip
    mpa_loss_reduce_*; the reference: base_model.py:348-387 with one stochastic sample)."""

    @staticmethod
    def forward(ctx, terms, weights):
        terms = terms.contiguous()
        K, B = terms.shape
        means = torch.empty(K, dtype=torch.float32, device=terms.device)
        loss = torch.empty((), dtype=torch.float32, device=terms.device)
        _lib.launch("mpa_loss_reduce_forward", terms.device, terms, weights, K, B, means, loss)
        ctx.save_for_backward(weights)
        ctx.shape = (K, B)
        ctx.set_materialize_grads(False)
        return means, loss

    @staticmethod
    def backward(ctx, g_means, g_loss):
        if g_means is None and g_loss is None:
            return None, None
        (weights,) = ctx.saved_tensors
        K, B = ctx.shape
        g_terms = torch.empty((K, B), dtype=torch.float32, device=weights.device)
        gm = g_means.contiguous() if g_means is not None else None
        gl = g_loss.contiguous() if g_loss is not None else None
        _lib.launch("mpa_loss_reduce_backward", weights.device, gl, gm, weights, K, B, g_terms)
        return g_terms, None


def weighted_term_means(terms, weights):
    """terms [K, B], weights [K] (float32, same CUDA device) -> (means [K], loss scalar) through the library."""
    return _LossReduce.apply(terms, weights)


def search_mode(name=None):
    """The search behind the loss's two Chamfer terms as the C ABI's code: MPA_SHAPE_SEARCH if set (the override for tests
    and A/B runs), else `name` (a key of SEARCH_MODES; what a configuration asks for), else "grid".  Identical results all;
    "leaf" / "auto" pay where parts are many and small and need the batch's `part_order`."""
    import os
    name = os.environ.get("MPA_SHAPE_SEARCH") or name or "grid"
    if name not in SEARCH_MODES:
        raise ValueError(f"shape search must be one of {sorted(SEARCH_MODES)}, not {name!r}")
    return SEARCH_MODES[name]


def geometric_assembly_loss(part_pcs, pred_trans, pred_rot, gt_trans, gt_rot, valids, training=True,
                            ret_pts=False, order=None, search=None):
    """The loss terms of `BaseModel._calc_loss` for geometric data, fused (no GT re-matching).

    Returns ({name: [B]} for LOSS_TERMS, pts) where pts is None or, with ret_pts,
    (pred_trans_pts, gt_trans_pts) [B,P,N,3] as shape_cd_loss(..., ret_pts=True) returns them.
    Gradients flow to pred_trans and pred_rot only (the GT pose is detached, as in the reference).  `pred_rot` and
    `gt_rot` are quaternions or rotation matrices (both of the same type; rot_loss in the matching form, loss.py:59-84).
    `search`: "brute" | "grid" | "leaf" | "auto" (None: MPA_SHAPE_SEARCH, else "grid"): which exact searches run the two
    Chamfer terms — identical results.  `order`: `part_order(part_pcs, valids)` of this batch for "leaf" / "auto" when the
    caller evaluates the loss more than once per batch (computed by the call itself when None).
    """
    _lib.require_hip("geometric_assembly_loss", part_pcs)
    B, P, N, _ = part_pcs.shape
    f = lambda t: t.detach().to(torch.float32).contiguous()
    if pred_rot.rot_type != gt_rot.rot_type:
        raise ValueError(f"rotation types differ: {pred_rot.rot_type} vs {gt_rot.rot_type}")
    rot = (lambda r: r.rot) if pred_rot.rot_type == "rmat" else _quat
    losses, pts = _AssemblyLoss.apply(
        f(part_pcs), f(valids), rot(pred_rot).to(torch.float32).contiguous(),
        pred_trans.to(torch.float32).contiguous(), f(rot(gt_rot)), f(gt_trans), bool(training),
        bool(ret_pts), order, search_mode(search))
    terms = LossTerms((name, losses[i]) for i, name in enumerate(LOSS_TERMS))
    terms.stacked = (LOSS_TERMS, losses)
    return terms, ((pts[2], pts[3]) if ret_pts else None)
