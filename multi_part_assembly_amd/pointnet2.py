"""PointNet++ single-scale-grouping part encoder — mirror of the reference's `PointNet2SSG`
(multi_part_assembly/models/modules/encoder/pointnet2/pointnet2_ssg.py over pointnet2_ops/pointnet2_modules.py) with the
same constructor argument, forward contract ([n, N, 3] -> [n, feat_dim]) and state_dict keys
(`SA_modules.{i}.mlps.0.{0,1,3,4,6,7}.*`), so a reference checkpoint loads unchanged.

Sampling and grouping run on csrc/pointnet2_ops.hip through `pointnet2_utils`; the shared MLPs run on the module's own
Conv2d / BatchNorm2d / ReLU sub-modules — library operators, the reference's own op sequence.  In evaluation
(`eval()` under `no_grad`) `set_eval_mlp("fused")` routes the levels through csrc/pointnet2_sa_mlp.hip instead
(pointnet2_fused.py): gather, the three layers and the max in one kernel, no [n, C, S, K] tensor.  The training-mode
fused path (statistics passes and a backward) is the follow-up; `pointnet2_msg` is not built.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import pointnet2_utils


def build_shared_mlp(widths, bn=True):
    layers = []
    for i in range(1, len(widths)):
        layers.append(nn.Conv2d(widths[i - 1], widths[i], kernel_size=1, bias=not bn))
        if bn:
            layers.append(nn.BatchNorm2d(widths[i]))
        layers.append(nn.ReLU(True))
    return nn.Sequential(*layers)


class PointnetSAModule(nn.Module):
    """One set-abstraction level with a single scale: furthest point sampling of `npoint` centres, a ball query of
    `nsample` points within `radius` around each (or, with npoint None, one group of every point), the shared MLP on
    [xyz - centre ; features], a max over the samples.  `groupers` / `mlps` are lists of one, as upstream."""

    def __init__(self, mlp, npoint=None, radius=None, nsample=None, bn=True, use_xyz=True):
        super().__init__()
        self.npoint = npoint
        self.groupers = nn.ModuleList([pointnet2_utils.QueryAndGroup(radius, nsample, use_xyz=use_xyz)
                                       if npoint is not None else pointnet2_utils.GroupAll(use_xyz)])
        widths = list(mlp)
        if use_xyz:
            widths[0] += 3
        self.mlps = nn.ModuleList([build_shared_mlp(widths, bn)])

    def forward(self, xyz, features):
        """xyz [n, N, 3], features [n, C, N] | None -> new_xyz [n, npoint, 3] | None, new_features [n, C', npoint | 1]."""
        new_xyz = None
        if self.npoint is not None:
            centres = pointnet2_utils.furthest_point_sample(xyz, self.npoint)
            new_xyz = pointnet2_utils.gather_operation(xyz.transpose(1, 2).contiguous(), centres)
            new_xyz = new_xyz.transpose(1, 2).contiguous()
        out = []
        for grouper, mlp in zip(self.groupers, self.mlps):
            h = mlp(grouper(xyz, new_xyz, features))                       # [n, C', npoint, nsample]
            out.append(F.max_pool2d(h, kernel_size=[1, h.size(3)]).squeeze(-1))
        return new_xyz, torch.cat(out, dim=1)


class PointNet2SSG(nn.Module):
    """SA(512, 0.2, 64, 3-64-64-128) -> SA(128, 0.4, 64, 131-128-128-256) -> SA(all, 259-256-512-feat_dim).

    `forward_parts` is the entry of the assembly models: every part slot plus the validity mask.  BatchNorm must see the
    valid parts only, so the slots are compacted on the host first — one host synchronisation per forward, which the
    module advertises (`host_sync_per_forward`): `Trainer(use_graph=True)` keeps such a model on eager launches."""

    host_sync_per_forward = True
    # "library": the shared MLPs on Conv2d / BatchNorm2d / ReLU / max_pool2d, always.  "fused": in eval() mode without
    # gradients the levels run on csrc/pointnet2_sa_mlp.hip (pointnet2_fused.py); training and grad-enabled calls are the
    # library path either way.  Opt-in: `set_eval_mlp`, or cfg.model.pointnet2_eval through the models.
    EVAL_MLP_MODES = ("library", "fused")
    eval_mlp = "library"

    def __init__(self, feat_dim):
        super().__init__()
        self.feat_dim = feat_dim
        self.SA_modules = nn.ModuleList([
            PointnetSAModule(npoint=512, radius=0.2, nsample=64, mlp=[0, 64, 64, 128], use_xyz=True),
            PointnetSAModule(npoint=128, radius=0.4, nsample=64, mlp=[128, 128, 128, 256], use_xyz=True),
            PointnetSAModule(mlp=[256, 256, 512, feat_dim], use_xyz=True),
        ])

    def set_eval_mlp(self, mode):
        if mode not in self.EVAL_MLP_MODES:
            raise ValueError(f"PointNet2SSG.eval_mlp must be 'library' or 'fused', got {mode!r}")
        self.eval_mlp = mode
        return self

    def _forward_fused_eval(self, xyz, record):
        """The levels on pointnet2_fused.sa_level_eval, features point-major in between; a level outside the kernel's
        envelope runs its library chain (one warning per encoder)."""
        from . import pointnet2_fused
        from .encoder import _warn_library_path
        feats_pm = None                                                       # [n, N, C]
        for module in self.SA_modules:
            miss = pointnet2_fused.envelope_miss(module)
            if miss is None:
                xyz, feats_pm = pointnet2_fused.sa_level_eval(module, xyz, feats_pm)
                if record is not None:
                    record.append((xyz, feats_pm.transpose(1, 2).contiguous()))
            else:
                _warn_library_path(self, f"a set-abstraction level with {miss}")
                xyz, features = module(xyz, None if feats_pm is None else feats_pm.transpose(1, 2).contiguous())
                if record is not None:
                    record.append((xyz, features))
                feats_pm = features.transpose(1, 2).contiguous()
        return feats_pm.squeeze(1)

    def forward(self, pointcloud, record=None):
        """pointcloud [n, N, 3 + ...] -> [n, feat_dim]; `record`: a list that receives (new_xyz, features) of each level."""
        xyz, features = pointcloud[..., 0:3].contiguous(), None
        if self.eval_mlp == "fused" and not self.training and not torch.is_grad_enabled():
            return self._forward_fused_eval(xyz, record)
        for module in self.SA_modules:
            xyz, features = module(xyz, features)
            if record is not None:
                record.append((xyz, features))
        return features.squeeze(-1)

    def forward_parts(self, part_pcs, valids):
        """part_pcs [M, N, 3], valids [M] (1/0) -> [M, feat_dim]; rows of padded parts are zero, their points never read."""
        from .encoder import _run_valid_parts
        return _run_valid_parts(self.forward, part_pcs, valids, self.feat_dim, False)
