"""Cost of computing a batch's contact table: the operator (csrc/contact_points.hip) against the same table composed on
library operators, B = 32, P = 20, N = 1000, part counts of `bench.representative_parts`.  One JSON line:

  ms_operator        ms per `contacts.contact_points` call returning the table alone (the bounding-box prune is active)
  ms_operator_full   ms per call that also returns `min_dist` and `index` (every real pair is searched)
  ms_cdist           ms for the yardstick, `cdist_table` below: the pose operator, then `torch.cdist` per block of pairs
                     i < j plus an arg-min over the flattened (a, c) axis and the gathers that fill the table.  It searches
                     all P (P - 1) / 2 pairs of every sample, padded ones too: which slots are padding is known on the
                     device only, and learning it first would be a host synchronisation.  `cdist` is not the pinned
                     arithmetic, so the arm is a yardstick for time, not for bits; `flags_differ` counts the table flags
                     on which it disagrees with the operator
  *_windows          all arms in ONE process, alternating windows after a warm-up; each figure is a host clock around a
                     window that ends in a device synchronise, divided by its calls; the median of the windows is reported
  real_pairs / contacts   pairs of real parts in the batch, and how many of them the table flags

GPU only:  python tools/contact_rate.py [--calls 10] [--windows 5] [--out profiles/r14_contact_rate.json]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_rig as rig  # noqa: E402  (puts the repository root on sys.path)
from multi_part_assembly_amd import contacts, synthetic  # noqa: E402
from multi_part_assembly_amd.rotation import Rotation3D  # noqa: E402
from multi_part_assembly_amd.transforms import transform_pc  # noqa: E402


def cdist_table(part_pcs, valids, rot, trans, thre=0.01, pairs_per_step=8):
    """The contact table on library operators: `pairs_per_step` pairs i < j of every sample per `torch.cdist` call."""
    B, P, N, _ = part_pcs.shape
    dev = part_pcs.device
    posed = transform_pc(trans, rot, part_pcs)
    real = valids == 1
    table = torch.zeros((B, P, P, 4), dtype=torch.float32, device=dev)
    I, J = torch.triu_indices(P, P, offset=1, device=dev)
    rows = torch.arange(B, device=dev)[:, None]
    for k0 in range(0, I.numel(), pairs_per_step):
        i, j = I[k0:k0 + pairs_per_step], J[k0:k0 + pairs_per_step]
        K = i.numel()
        d = torch.cdist(posed[:, i].reshape(B * K, N, 3), posed[:, j].reshape(B * K, N, 3)).reshape(B, K, N * N)
        dmin, flat = d.min(dim=2)
        touch = real[:, i] & real[:, j] & (dmin * dmin < thre)
        flag = touch.float()[..., None]
        table[:, i, j] = torch.cat([flag, part_pcs[rows, i[None], flat // N] * flag], dim=-1)
        table[:, j, i] = torch.cat([flag, part_pcs[rows, j[None], flat % N] * flag], dim=-1)
    return table


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--parts", type=int, default=20)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--thre", type=float, default=0.01)
    ap.add_argument("--out", default="")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    dev = torch.device("cuda:0")
    B, P, N = args.batch, args.parts, args.points
    result = {"B": B, "P": P, "N": N, "thre": args.thre, "calls_per_window": args.calls, "windows": args.windows}
    parts = rig.representative_parts(1234)
    parts = [min(P, parts[b % len(parts)]) for b in range(B)]
    batch = synthetic.make_batch(B, P, N, seed=1234, device=dev, num_parts=parts)
    part_pcs, valids, trans = batch["part_pcs"], batch["part_valids"], batch["part_trans"]
    rot = Rotation3D(batch["part_quat"], "quat")
    out1 = (torch.empty((B, P, P, 4), dtype=torch.float32, device=dev),)
    out3 = (torch.empty_like(out1[0]), torch.empty((B, P, P), dtype=torch.float32, device=dev),
            torch.empty((B, P, P), dtype=torch.int32, device=dev))
    arms = {
        "operator": lambda i: contacts.contact_points(part_pcs, valids, rot, trans, thre=args.thre, out=out1),
        "operator_full": lambda i: contacts.contact_points(part_pcs, valids, rot, trans, thre=args.thre, return_dist=True,
                                                           return_index=True, out=out3),
        "cdist": lambda i: cdist_table(part_pcs, valids, rot, trans, thre=args.thre),
    }
    table = arms["operator"](0).clone()
    full = arms["operator_full"](0)[0]
    yard = arms["cdist"](0)
    result["operator_arms_agree_bitwise"] = bool(torch.equal(table, full))
    result["flags_differ"] = int((table[..., 0] != yard[..., 0]).sum().item())
    result["real_pairs"] = int(sum(p * (p - 1) // 2 for p in parts))
    result["contacts"] = int(table[..., 0].sum().item()) // 2
    result["pair_evaluations_full"] = result["real_pairs"] * N * N
    calls = {k: args.calls if k != "cdist" else max(1, args.calls // 5) for k in arms}
    rig.report(result, rig.alternate(arms, calls, args.windows, 2), key="ms_{name}")
    rig.emit(result, args.out)


if __name__ == "__main__":
    main()
