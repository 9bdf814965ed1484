"""The five terms of the fused assembly loss (csrc/assembly_loss.hip) as a plain torch function with the nearest-neighbour
SELECTIONS PINNED: the yardstick of tests/test_loss_anchored_gpu.py and of the `lossgrad` family of tools/fuzz_parity.py
(a plain module, imported like tests/eval_ref.py and tests/anchored.py; the HIP path is driven by tests/assembly_loss_hip.py).

`pinned_loss` restates oracle/geometry.py (the reference's utils/loss.py:22-35,59-202) for quaternion poses and, for
rotation matrices, p' = R p + t with the rotation term mean((I - R1^T R2)^2) over the nine entries (utils/loss.py:59-86).
The two Chamfer terms do not search: they take the four arg-min arrays (ip1, ip2, is1, is2), each int [B, P, N], and
gather.  The arg-mins of the HIP path are proven bit-equal to the exhaustive scan elsewhere (tests/test_loss_gpu.py,
tests/test_rmat_gpu.py); given the selections the loss is a smooth function of the poses, so a float32-versus-float64
near-tie flip cannot turn a rounding difference into an O(1/N) gradient difference.  It is evaluated in the dtype of its
inputs and differentiated by autograd; tests/test_assembly_loss_ref.py holds it against `og.calc_loss_geometric` in
float64 (which does search, through the C oracle) and shows that the bars of tests/anchored.py reject its deliberately
wrong variants (`wrong=`) and accept a re-associated float32 evaluation.

Index conventions (those of the int workspace of mpa_assembly_loss_forward): ip1 / ip2 in 0..N-1 within the part, is1 / is2
in 0..P*N-1 within the sample; -1 = no candidate below 1e32: the distance is 1e32 and carries no gradient
(chamfer_kernel.cu:60,199-208).  Entries of padded parts are ignored (the loss multiplies their distances by zero).
"""
import numpy as np
import torch

from oracle import geometry as og

LOSS_TERMS = ("trans_loss", "rot_pt_cd_loss", "transform_pt_cd_loss", "rot_loss", "rot_pt_l2_loss")
PAD_FILL = 1e3   # utils/loss.py:173-175
NO_MATCH = 1e32  # chamfer_kernel.cu:60
WRONG = ("no_branch_c_for_pads", "eval_norm_in_training", "last_quarter_dropped", "sgn_plus_one")


# ---- rotations -------------------------------------------------------------------------------------------------------
def quat_to_rmat(q):
    """pytorch3d's quaternion_to_matrix in the dtype of q: [..., 4] real-first -> [..., 3, 3]."""
    r, i, j, k = q.unbind(-1)
    two_s = 2.0 / (((r * r + i * i) + j * j) + k * k)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def rot6d_to_rmat(d6):
    """pytorch3d's rotation_6d_to_matrix in the dtype of d6 (rows b1, b2, b1 x b2)."""
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = a1 / a1.norm(dim=-1, keepdim=True)
    b2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = b2 / b2.norm(dim=-1, keepdim=True)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2)


def rotate(rot, pts, rot_type):
    """rot [B, P, 4] or [B, P, 3, 3] applied to pts [B, P, N, 3]."""
    if rot_type == "quat":
        return og.rot_pc(rot, pts)
    assert rot_type == "rmat" and rot.shape[-2:] == (3, 3)
    return (rot[:, :, None, :, :] * pts[:, :, :, None, :]).sum(-1)


# ---- the loss ----------------------------------------------------------------------------------------------------------
def _pinned_sqdist(query, target, idx):
    """|query[i] - target[idx[i]]|^2 over the last-but-one axis; idx = -1: NO_MATCH, no gradient."""
    ok = idx >= 0
    j = idx.clamp_min(0)
    near = torch.gather(target, -2, j[..., None].expand(j.shape + (3,)))
    d = (query - near).pow(2).sum(-1)
    return torch.where(ok, d, torch.full_like(d, NO_MATCH))


def pinned_loss(pcs, valids, rot_pred, trans_pred, rot_gt, trans_gt, idx, rot_type="quat", training=True, wrong=None):
    """The five terms [5, B] in LOSS_TERMS order.  pcs [B, P, N, 3], valids [B, P], rot_* [B, P, 4] (already through the
    zero-quaternion rule) or [B, P, 3, 3], trans_* [B, P, 3], idx = (ip1, ip2, is1, is2).  `wrong`: one of WRONG, the
    deliberately wrong variants of tests/test_assembly_loss_ref.py."""
    assert wrong is None or wrong in WRONG
    B, P, N, _ = pcs.shape
    dt = pcs.dtype
    v = valids.to(dt).detach()
    vb = v > 0
    rot_gt, trans_gt, pcs = rot_gt.detach(), trans_gt.detach(), pcs.detach()
    # (what a padded part's entries hold is ignored: they are replaced by index 0 and weighted by zero below)
    ip1, ip2, is1, is2 = (torch.where(vb[..., None], torch.as_tensor(i).long(), 0) for i in idx)
    wn = torch.ones(N, dtype=dt)
    if wrong == "last_quarter_dropped":
        wn[N - max(N // 4, 1):] = 0.0
    mean_n = lambda d: (d * wn).sum(-1) / N                      # [B, P, N] -> [B, P]
    valid_mean = lambda per_part: (per_part * v).sum(1) / v.sum(1)

    trans = valid_mean((trans_pred - trans_gt).pow(2).sum(-1))                                    # utils/loss.py:22-35
    r1, r2 = rotate(rot_pred, pcs, rot_type), rotate(rot_gt, pcs, rot_type)
    part_cd = valid_mean(mean_n(_pinned_sqdist(r1, r2, ip1)) + mean_n(_pinned_sqdist(r2, r1, ip2)))  # :113-138
    pt_l2 = valid_mean(mean_n((r1 - r2).pow(2).sum(-1)))                                          # :89-110

    filled = pcs.masked_fill(~vb[..., None, None], PAD_FILL)                                      # :173-175
    s1 = rotate(rot_pred, filled, rot_type) + trans_pred[:, :, None]
    s2 = rotate(rot_gt, filled, rot_type) + trans_gt[:, :, None]
    s1_target = s1
    if wrong == "no_branch_c_for_pads":
        s1_target = torch.where(vb[..., None, None], s1, s1.detach())
    d1 = _pinned_sqdist(s1.flatten(1, 2), s2.flatten(1, 2), is1.flatten(1)).view(B, P, N)
    d2 = _pinned_sqdist(s2.flatten(1, 2), s1_target.flatten(1, 2), is2.flatten(1)).view(B, P, N)
    if training and wrong != "eval_norm_in_training":
        shape_cd = ((d1 * wn).sum(-1) * v).sum(1) / (P * N) + ((d2 * wn).sum(-1) * v).sum(1) / (P * N)  # :185-193
    else:
        shape_cd = valid_mean(mean_n(d1 + d2))                                                    # :194-198

    if rot_type == "quat":
        dot = (rot_pred * rot_gt).sum(-1)
        mag = dot.abs()
        if wrong == "sgn_plus_one":  # the value of |dot| with the derivative of dot
            mag = dot + (dot.abs() - dot).detach()
        rot = valid_mean(1.0 - mag)                                                                # :59-86, quaternions
    else:
        m = (rot_pred[..., :, :, None] * rot_gt[..., :, None, :]).sum(-3)  # (R1^T R2)_ij = sum_a R1[a][i] R2[a][j]
        rot = valid_mean((torch.eye(3, dtype=dt) - m).pow(2).mean(dim=(-1, -2)))                   # :76-82, matrices
    return torch.stack((trans, part_cd, shape_cd, rot, pt_l2))


def run(batch, idx, go, rot_type, training=True, dtype=torch.float64, wrong=None, samples=None):
    """One evaluation of `pinned_loss` and its autograd gradient of sum(go * losses), in `dtype` on the CPU, cast from the
    float32 values of `batch`.  `samples`: evaluate these samples only (a list of indices).  Returns (losses [5, B'],
    grad_rot, grad_trans) as float64 tensors."""
    pick = (lambda t: t) if samples is None else (lambda t: t[samples])
    c = lambda t: pick(t.detach().cpu()).to(dtype).clone()
    rp, tp = c(batch["rot_pred"]).requires_grad_(), c(batch["trans_pred"]).requires_grad_()
    idx = tuple(pick(torch.as_tensor(i).cpu()) for i in idx)
    go = go.detach().cpu().to(dtype)
    go = go if samples is None else go[:, samples]
    losses = pinned_loss(c(batch["pcs"]), c(batch["valids"]), rp, tp, c(batch["rot_gt"]), c(batch["trans_gt"]), idx,
                         rot_type, training, wrong)
    (losses * go).sum().backward()
    return losses.detach().double(), rp.grad.double(), tp.grad.double()


def tensors(losses, grad_rot, grad_trans, rows=(), samples=None, overflow=(), per_sample=()):
    """The per-sample tensors handed to anchored.check: `gq.b<k>`, `gt.b<k>` for every sample and the five loss terms.
    `rows`: (sample, part) pairs whose row is a tensor of its own (`gq.b<k>.p<p>`), the remaining rows of that sample
    then being `gq.b<k>.rest`.  `samples`: the names of the samples when the evaluation left some out.  `overflow`: (term,
    sample) entries of the losses that exceed float32's range by construction (`Case.overflow`) and are left out.
    `per_sample`: indices of the terms handed over as one tensor per sample (`loss.<name>.b<k>`), for a case in which one
    sample's value would dwarf the others' (`Case.per_sample`)."""
    B, P = grad_trans.shape[:2]
    names = list(range(B)) if samples is None else list(samples)
    out = {}
    for tag, g in (("gq", grad_rot), ("gt", grad_trans)):
        g = g.detach().cpu().double().reshape(B, P, -1)
        for k in range(B):
            own = [p for b, p in rows if b == names[k]]
            if not own:
                out[f"{tag}.b{names[k]}"] = g[k]
                continue
            for p in own:
                out[f"{tag}.b{names[k]}.p{p}"] = g[k, p]
            out[f"{tag}.b{names[k]}.rest"] = g[k][[p for p in range(P) if p not in own]]
    for i, name in enumerate(LOSS_TERMS):
        keep = [k for k in range(B) if (i, names[k]) not in overflow]
        term = losses[i].detach().cpu().double()
        if i in per_sample:
            out.update({f"loss.{name}.b{names[k]}": term[k:k + 1] for k in keep})
        else:
            out["loss." + name] = term[keep]
    return out


def permuted(batch, idx, perm):
    """The same batch with every part's points in the order `perm` (a permutation of 0..N-1) and the arg-min arrays
    mapped along: the same function with every sum over points in another order — forward and backward."""
    perm = torch.as_tensor(perm).long()
    N = perm.numel()
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(N)
    ip1, ip2, is1, is2 = (torch.as_tensor(i).long() for i in idx)
    part = lambda i: torch.where(i >= 0, inv[i.clamp_min(0)], i)[..., perm]
    shape = lambda i: torch.where(i >= 0, (i.clamp_min(0) // N) * N + inv[i.clamp_min(0) % N], i)[..., perm]
    out = dict(batch)
    out["pcs"] = batch["pcs"][:, :, perm].contiguous()
    return out, (part(ip1), part(ip2), shape(is1), shape(is2))


# ---- batches (built on the host) ----------------------------------------------------------------------------------------
def masks(B, P, kind, g):
    """valids [B, P] of kind
      "full"       all ones;
      "prefix"     the first c_b slots of sample b: c_0 = P, c_1 = 1, the others drawn in 1..P;
      "sparse"     about 63 % of the slots of every sample at random, never none;
      "nonprefix"  sample 0 full, sample 1 a single valid part (slot P // 2), the others about 60 % of the slots at
                   random, never none."""
    v = torch.ones(B, P)
    if kind == "full":
        return v
    if kind == "sparse":
        v = (torch.rand(B, P, generator=g) < 0.63).float()
        v[:, P - 1] = torch.where(v.sum(1) == 0, torch.ones(B), v[:, P - 1])
        return v
    for b in range(1, B):
        if kind == "prefix":
            c = 1 if b == 1 else int(torch.randint(1, P + 1, (1,), generator=g))
            v[b] = (torch.arange(P) < c).float()
        else:
            v[b] = (torch.rand(P, generator=g) < 0.6).float()
            if b == 1:
                v[b] = 0.0
                v[b, P // 2] = 1.0
            elif v[b].sum() == 0:
                v[b, P - 1] = 1.0
    return v


def make_batch(B, P, N, rot_type, seed, mask="nonprefix", valids=None):
    """float32 CPU tensors pcs, valids, rot_pred, trans_pred, rot_gt, trans_gt: every part a random box of points scaled
    per part, GT quaternions normalised, GT translations about 0.3, padded slots all zero (identity GT rotation);
    predicted poses random unit quaternions — for "rmat" the 6D -> matrix conversion of random vectors in float64, rounded
    once — and translations about 0.3."""
    g = torch.Generator().manual_seed(seed)
    v = masks(B, P, mask, g) if valids is None else torch.as_tensor(valids, dtype=torch.float32).reshape(B, P)
    box = 0.05 + 0.3 * torch.rand(B, P, 1, 3, generator=g)
    pcs = (torch.rand(B, P, N, 3, generator=g) - 0.5) * box
    qg = torch.nn.functional.normalize(torch.randn(B, P, 4, generator=g), dim=-1)
    tg = 0.3 * torch.randn(B, P, 3, generator=g)
    qp = torch.nn.functional.normalize(torch.randn(B, P, 4, generator=g), dim=-1)
    d6 = torch.randn(B, P, 6, generator=g, dtype=torch.float64)
    tp = 0.3 * torch.randn(B, P, 3, generator=g)
    pad = v == 0
    pcs[pad] = 0.0
    tg[pad] = 0.0
    qg[pad] = torch.tensor([1.0, 0.0, 0.0, 0.0])  # the all-zero quaternion after Rotation3D's rule
    if rot_type == "rmat":
        rot_gt, rot_pred = quat_to_rmat(qg.double()).float(), rot6d_to_rmat(d6).float()
    else:
        rot_gt, rot_pred = qg, qp
    return {"pcs": pcs.contiguous(), "valids": v, "rot_pred": rot_pred.contiguous(), "trans_pred": tp.contiguous(),
            "rot_gt": rot_gt.contiguous(), "trans_gt": tg}


def identity_rot(rot_type):
    return torch.tensor([1.0, 0.0, 0.0, 0.0]) if rot_type == "quat" else torch.eye(3)


def make_padded_nearest(batch, rot_type):
    """Case H, in place: in every sample one padded slot becomes somebody's nearest neighbour.  Its predicted rotation is the
    identity (the fill point (1e3, 1e3, 1e3) then stays exact; a generic rotation of it costs 1e-4 absolute in float32
    and makes the case ill-conditioned for any float32 code) and its predicted translation (a transformed GT point of a
    valid part + 0.004) - 1e3, computed in float32.  Returns the (sample, slot) pairs."""
    v = batch["valids"]
    with torch.no_grad():
        s2 = rotate(batch["rot_gt"], batch["pcs"], rot_type) + batch["trans_gt"][:, :, None]
    rows = []
    for b in range(v.shape[0]):
        pad = int((v[b] == 0).nonzero()[0])
        src = int((v[b] != 0).nonzero()[0])
        batch["rot_pred"][b, pad] = identity_rot(rot_type)
        batch["trans_pred"][b, pad] = (s2[b, src, 0] + np.float32(0.004)) - np.float32(PAD_FILL)
        rows.append((b, pad))
    return rows


def exhaustive_indices(batch, rot_type, dtype=torch.float64):
    """The four arg-min arrays of the exhaustive scan (oracle/chamfer_ref.c) over the clouds posed in `dtype` on the CPU."""
    from oracle import chamfer as oc
    c = lambda k: batch[k].detach().cpu().to(dtype)
    pcs, v = c("pcs"), batch["valids"].cpu() > 0
    B, P, N, _ = pcs.shape
    with torch.no_grad():
        r1, r2 = rotate(c("rot_pred"), pcs, rot_type), rotate(c("rot_gt"), pcs, rot_type)
        filled = pcs.masked_fill(~v[..., None, None], PAD_FILL)
        s1 = rotate(c("rot_pred"), filled, rot_type) + c("trans_pred")[:, :, None]
        s2 = rotate(c("rot_gt"), filled, rot_type) + c("trans_gt")[:, :, None]
    _, p1, _, p2 = oc.chamfer_forward(r1.flatten(0, 1).numpy(), r2.flatten(0, 1).numpy())
    _, i1, _, i2 = oc.chamfer_forward(s1.flatten(1, 2).numpy(), s2.flatten(1, 2).numpy())
    return tuple(torch.from_numpy(i).view(B, P, N) for i in (p1, p2, i1, i2))


def pin_disagreement(batch, idx, rot_type):
    """(differing, valid queries): the entries of the four arg-min arrays `idx`, on the valid parts, that differ from the
    float64 exhaustive scan."""
    v = batch["valids"].cpu() > 0
    ref = exhaustive_indices(batch, rot_type)
    diff = sum(int((torch.as_tensor(a).cpu().long()[v] != r[v]).sum()) for a, r in zip(idx, ref))
    return diff, 4 * int(v.sum()) * batch["pcs"].shape[2]


# ---- the cases of tests/test_loss_anchored_gpu.py (the CPU tests build the same batches) --------------------------------
class Case:
    """group: the letter of the case table; kind: "plain", "sign" (G), "padnear" (H), "far" (I), "empty" (J)."""

    def __init__(self, group, rot_type, shape, mask="nonprefix", training=True, kind="plain", valids=None):
        self.group, self.rot_type, self.shape, self.mask, self.training = group, rot_type, tuple(shape), mask, training
        self.kind, self.valids = kind, valids
        # (term, sample) entries of the losses above float32's range: the squared 1e20 translation of case I is 1e40, +inf in
        # any float32 evaluation; the gradient, 2e20 / nv, is representable and is compared
        self.overflow = ((0, 0),) if kind == "far" else ()
        # terms compared one sample at a time: in case I the N stored distances of 1e32 make transform_pt_cd_loss of sample 0
        # about 2.5e31, next to which the other samples' values would not be checked
        self.per_sample = (2,) if kind == "far" else ()
        B, P, N = shape
        self.seed = 100000 * (ord(group) - ord("A")) + 1000 * B + 100 * P + N + (7 if rot_type == "rmat" else 0)
        self.id = f"{group}-{rot_type}-{B}x{P}x{N}" + ("" if training else "-eval")

    def build(self):
        """(batch, go [5, B], rows): `rows` are the (sample, part) pairs compared as tensors of their own."""
        B, P, N = self.shape
        batch = make_batch(B, P, N, self.rot_type, self.seed, self.mask, self.valids)
        g = torch.Generator().manual_seed(self.seed + 1)
        go = torch.rand(5, B, generator=g) + 0.5
        rows = []
        if self.kind == "sign":  # (0, 0): dot < 0; (1, P // 2), the single valid part of sample 1: dot == 0; sample 2: zeroed weights
            qg = batch["rot_gt"]
            batch["rot_pred"][0, 0] = torch.nn.functional.normalize(-qg[0, 0] + 0.05 * torch.randn(4, generator=g), dim=-1)
            batch["rot_pred"][1, P // 2] = torch.tensor([1.0, 0.0, 0.0, 0.0])
            qg[1, P // 2] = torch.tensor([0.0, 1.0, 0.0, 0.0])
            go[3, 2] = go[4, 2] = 0.0
            assert float((batch["rot_pred"][0, 0] * qg[0, 0]).sum()) < -0.9
            assert float((batch["rot_pred"][1, P // 2] * qg[1, P // 2]).sum()) == 0.0 and batch["valids"][1, P // 2] == 1
        elif self.kind == "padnear":
            rows = make_padded_nearest(batch, self.rot_type)
        elif self.kind == "far":  # every distance of part (0, 1) is above 1e32: its stored indices are -1
            batch["trans_pred"][0, 1] = 1e20
            rows = [(0, 1)]
        elif self.kind == "empty":
            batch = make_batch(B, P, N, self.rot_type, self.seed, self.mask,
                               batch["valids"] * (torch.arange(B) != EMPTY_SAMPLE)[:, None])
        return batch, go, rows


EMPTY_SAMPLE = 2  # of case J
_PADNEAR = [[1, 0, 1], [1, 1, 0]]
CASES = (
    [Case("A", "quat", s) for s in ((3, 5, 1), (2, 3, 7), (3, 5, 33), (2, 7, 130))]
    + [Case("B", "quat", s, m) for s, m in (((2, 4, 896), "prefix"), ((2, 4, 897), "nonprefix"), ((1, 2, 1023), "prefix"),
                                            ((2, 3, 1025), "nonprefix"))]
    + [Case("C", "rmat", s, m) for s, m in (((2, 3, 896), "prefix"), ((2, 3, 899), "nonprefix"), ((2, 2, 1920), "prefix"),
                                            ((2, 2, 1923), "nonprefix"), ((1, 2, 2049), "prefix"))]
    + [Case("D", r, s, m) for r in ("quat", "rmat") for s, m in (((1, 1, 40), "full"), ((2, 2, 40), "nonprefix"),
                                                                 ((1, 63, 16), "sparse"), ((1, 64, 16), "sparse"))]
    + [Case("E", r, s, training=False) for r in ("quat", "rmat") for s in ((3, 6, 300), (2, 4, 1000))]
    + [Case("G", "quat", (3, 4, 64), kind="sign")]
    + [Case("H", r, s, kind="padnear", valids=_PADNEAR) for r in ("quat", "rmat") for s in ((2, 3, 16), (2, 3, 900))]
    + [Case("I", "quat", (3, 4, 200), kind="far")]
    + [Case("J", r, (4, 5, 100), kind="empty") for r in ("quat", "rmat")]
    + [Case("J", "quat", (4, 5, 100), kind="empty", training=False)]  # (the empty sample's terms differ between the two modes)
)
ROUTE_CASES = [Case("F", r, s) for r in ("quat", "rmat") for s in ((4, 20, 130), (2, 6, 1000))]
ROUTES = ("brute", "grid", "leaf", "auto")
PIN_SCAN_LIMIT = 20000  # B P N up to which the float64 exhaustive scan is run next to a case
PIN_SHARE = 1e-3        # at most this share of a case's valid queries may select differently from that scan
