"""PointNet++ modules and part encoders — the counterpart of the reference's `pointnet2_ops/pointnet2_modules.py`
(`PointnetSAModuleMSG`, `PointnetSAModule`, `PointnetFPModule`) and of its encoders `PointNet2SSG` / `PointNet2MSG`
(multi_part_assembly/models/modules/encoder/pointnet2/pointnet2_ssg.py, pointnet2_msg.py) with the same constructor
arguments, forward contracts ([n, N, 3] -> [n, feat_dim]) and state_dict keys (`SA_modules.{i}.mlps.{j}.{0,1,3,4,6,7}.*`,
`mlp.{0,1,3,4,...}.*`), so a reference checkpoint loads unchanged.

Sampling, grouping and interpolation run on csrc/pointnet2_ops.hip and csrc/pointnet2_interp.hip through `pointnet2_utils`;
the shared MLPs run on the modules' own Conv2d / BatchNorm2d / ReLU sub-modules — library operators, the reference's own op
sequence.  In evaluation (`eval()` under `no_grad`) `set_eval_mlp("fused")` routes the single-scale levels inside the kernel's
envelope through csrc/pointnet2_sa_mlp.hip instead (pointnet2_fused.py): gather, the three layers and the max in one kernel,
no [n, C, S, K] tensor.  The training-mode fused path (statistics passes and a backward) is the follow-up.
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


class PointnetSAModuleMSG(nn.Module):
    """One set-abstraction level with multi-scale grouping: ONE furthest point sampling of `npoint` centres, then per
    scale a ball query of `nsamples[i]` points within `radii[i]` (with npoint None, one group of every point), the scale's
    shared MLP on [xyz - centre ; features] and a max over the samples; the scales' outputs are concatenated along the
    channels.  The width lists of `mlps` are copied, never changed (upstream adds 3 to the caller's first entry)."""

    def __init__(self, npoint, radii, nsamples, mlps, bn=True, use_xyz=True):
        super().__init__()
        if not len(radii) == len(nsamples) == len(mlps):
            raise ValueError(f"PointnetSAModuleMSG: {len(radii)} radii, {len(nsamples)} sample counts, {len(mlps)} MLPs")
        self.npoint = npoint
        self.groupers = nn.ModuleList()
        self.mlps = nn.ModuleList()
        for radius, nsample, mlp in zip(radii, nsamples, mlps):
            self.groupers.append(pointnet2_utils.QueryAndGroup(radius, nsample, use_xyz=use_xyz)
                                 if npoint is not None else pointnet2_utils.GroupAll(use_xyz))
            widths = list(mlp)
            if use_xyz:
                widths[0] += 3
            self.mlps.append(build_shared_mlp(widths, bn))

    def forward(self, xyz, features):
        """xyz [n, N, 3], features [n, C, N] | None -> new_xyz [n, npoint, 3] | None, new_features [n, sum C', npoint | 1]."""
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


class PointnetSAModule(PointnetSAModuleMSG):
    """One set-abstraction level with a single scale: furthest point sampling of `npoint` centres, a ball query of
    `nsample` points within `radius` around each (or, with npoint None, one group of every point), the shared MLP on
    [xyz - centre ; features], a max over the samples.  `groupers` / `mlps` are lists of one, as upstream."""

    def __init__(self, mlp, npoint=None, radius=None, nsample=None, bn=True, use_xyz=True):
        super().__init__(npoint=npoint, radii=[radius], nsamples=[nsample], mlps=[mlp], bn=bn, use_xyz=use_xyz)


class PointnetFPModule(nn.Module):
    """Feature propagation: the features of the `known` points are carried to the `unknown` points by inverse-distance
    interpolation over the three nearest known points (weights 1 / (dist + 1e-8), normalised), concatenated in front of
    the unknown points' own features, and run through the shared MLP `mlp` (widths, first entry C2 + C1)."""

    def __init__(self, mlp, bn=True):
        super().__init__()
        self.mlp = build_shared_mlp(list(mlp), bn=bn)

    def forward(self, unknown, known, unknow_feats, known_feats):
        """unknown [M, n, 3], known [M, m, 3] | None, unknow_feats [M, C1, n] | None, known_feats [M, C2, m] -> [M, mlp[-1], n].
        known None: `known_feats` [M, C2, 1] is repeated over the n points (upstream's branch adds a list to a torch.Size
        and cannot run; this is its evident meaning)."""
        if known is not None:
            dist, idx = pointnet2_utils.three_nn(unknown, known)
            dist_recip = 1.0 / (dist + 1e-8)
            norm = torch.sum(dist_recip, dim=2, keepdim=True)
            weight = dist_recip / norm
            interpolated = pointnet2_utils.three_interpolate(known_feats, idx, weight)
        else:
            interpolated = known_feats.expand(known_feats.size(0), known_feats.size(1), unknown.size(1))
        new_features = interpolated if unknow_feats is None else torch.cat([interpolated, unknow_feats], dim=1)
        return self.mlp(new_features.unsqueeze(-1)).squeeze(-1)


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
        self._build_model()

    def _build_model(self):
        self.SA_modules = nn.ModuleList([
            PointnetSAModule(npoint=512, radius=0.2, nsample=64, mlp=[0, 64, 64, 128], use_xyz=True),
            PointnetSAModule(npoint=128, radius=0.4, nsample=64, mlp=[128, 128, 128, 256], use_xyz=True),
            PointnetSAModule(mlp=[256, 256, 512, self.feat_dim], use_xyz=True),
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


class PointNet2MSG(PointNet2SSG):
    """The multi-scale-grouping encoder of the reference's pointnet2_msg.py:
    SA(512; 0.1 / 0.2 / 0.4; 16 / 32 / 128; 3-32-32-64, 3-64-64-128, 3-64-96-128) ->
    SA(128; 0.2 / 0.4 / 0.8; 32 / 64 / 128; 323-64-64-128, 323-128-128-256, 323-128-128-256) ->
    SA(all, 643-256-512-feat_dim).  `forward`, `forward_parts` and `host_sync_per_forward` are PointNet2SSG's.  With
    `set_eval_mlp("fused")` every level takes its library chain under the one-warning rule: the multi-scale levels have
    three scales and the last one 640 input features, both outside the fused kernel's envelope.

    The class is complete and importable; `encoder.build_encoder("pointnet2_msg", ...)` still raises NotImplementedError,
    because that line of the registry is pinned by tests/test_pointnet2_encoder.py."""

    def _build_model(self):
        self.SA_modules = nn.ModuleList([
            PointnetSAModuleMSG(npoint=512, radii=[0.1, 0.2, 0.4], nsamples=[16, 32, 128],
                                mlps=[[0, 32, 32, 64], [0, 64, 64, 128], [0, 64, 96, 128]], use_xyz=True),
            PointnetSAModuleMSG(npoint=128, radii=[0.2, 0.4, 0.8], nsamples=[32, 64, 128],
                                mlps=[[320, 64, 64, 128], [320, 128, 128, 256], [320, 128, 128, 256]], use_xyz=True),
            PointnetSAModule(mlp=[640, 256, 512, self.feat_dim], use_xyz=True),
        ])
