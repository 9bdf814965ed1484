"""The PointNet++ SSG encoder of the fixture tests/golden/pointnet2_ssg.npz on the CPU with its ReLU decisions read out or
held fixed (a plain module, imported like tests/dgcnn_ref.py).

The first two set-abstraction levels put 3 to 13 million values in front of each ReLU: in float64 the smallest
pre-activation of each lies 8e-9 to 3e-7 from zero relative to its channel's largest — at float32 rounding.
A float32-grade evaluation in another summation order lands on the other side there; the value does not move, the
position's gradient appears or vanishes in every parameter gradient at and below the site, by about 1 / (positions of a
centre) of a tensor (1e-3).  The fixture's seed was chosen so that the float32 CPU pass takes the float64 decisions; a
device evaluation need not.  So the device's own decisions are read out, checked against the float64 pre-activations (a
decision may differ from the float64 sign only within FLIP_PREACT of zero) and held fixed in the float32 and float64 CPU
passes that the gradients are then compared with — what tests/test_dgcnn_anchored_gpu.py does for its maxima and slopes.
With the float64 decisions the pass reproduces the fixture's records (checked by the caller)."""
import sys

import torch

from conftest import GOLDEN
from multi_part_assembly_amd import pointnet2_utils as pu
from multi_part_assembly_amd.pointnet2 import PointNet2SSG

sys.path.insert(0, str(GOLDEN))
import param_fill  # noqa: E402


class _ReLU(torch.nn.Module):
    """ReLU that logs its input and, given a mask, passes exactly the masked positions."""

    def __init__(self, log, mask=None):
        super().__init__()
        self.log, self.mask = log, mask

    def forward(self, x):
        self.log.append(x.detach().cpu())
        return torch.relu(x) if self.mask is None else x * self.mask.to(x.dtype)


def relu_slots(enc):
    """(Sequential, index) of every ReLU of the encoder in execution order."""
    return [(sa.mlps[0], i) for sa in enc.SA_modules for i, m in enumerate(sa.mlps[0]) if isinstance(m, (torch.nn.ReLU, _ReLU))]


def build(fixture):
    enc = PointNet2SSG(int(fixture["w"].shape[1]))
    param_fill.fill_parameters(enc, int(fixture["seed"]))
    return enc.train()


def _gather64(features, idx):
    M, C, _ = features.shape
    flat = idx.long().reshape(M, 1, -1).expand(-1, C, -1)
    return features.gather(2, flat).reshape(M, C, *idx.shape[1:])


def cpu_pass(fixture, dtype, masks=None):
    """One training-mode forward + backward (loss = sum(out w)) on the CPU in `dtype`, ReLU decisions free (masks None) or
    held at `masks` (one bool tensor per ReLU, execution order).  Returns (`grad.<parameter>` in float64, the
    pre-activations of every ReLU)."""
    enc = build(fixture).to(dtype)
    log = []
    for k, (seq, i) in enumerate(relu_slots(enc)):
        seq[i] = _ReLU(log, None if masks is None else masks[k])
    saved = pu.grouping_operation, pu.gather_operation
    if dtype == torch.float64:  # (the operator module moves float32: the indices are found in float32 either way)
        pu.grouping_operation, pu.gather_operation = _gather64, _gather64
    try:
        out = enc(torch.from_numpy(fixture["points"]).to(dtype))
        (out * torch.from_numpy(fixture["w"]).to(dtype)).sum().backward()
    finally:
        pu.grouping_operation, pu.gather_operation = saved
    return {"grad." + k: p.grad.detach().double() for k, p in enc.named_parameters()}, log


def sites_off(masks, z64):
    """(number of decisions that differ from the float64 sign, the largest |z64| / channel maximum among them)."""
    n, worst = 0, 0.0
    for m, z in zip(masks, z64):
        off = m != (z > 0)
        if off.any():
            rel = z.abs() / z.abs().amax(dim=(0, 2, 3), keepdim=True)
            n, worst = n + int(off.sum()), max(worst, float(rel[off].max()))
    return n, worst
