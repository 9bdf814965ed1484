"""PNTransformer — PointNet part encoder -> transformer over part tokens -> pose head; mirror of the
reference model (multi_part_assembly/models/pn_transformer/network.py:9-139), same sub-module names
(`encoder`, `corr_module`, `pose_predictor`) and therefore the same state_dict keys.

Valid-part compaction is done with fixed shapes: the encoder runs on the compacted [n, N, 3] valid
parts (BatchNorm statistics must only see valid parts, as upstream), but the gather/scatter index
is built on the device without the boolean-mask indexing of network.py:64-67.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .base_model import BaseModel
from .encoder import build_encoder
from .regressor import StocasticPoseRegressor
from .transformer import TransformerEncoder


class PNTransformer(BaseModel):
    BATCH_KEYS = ("part_pcs", "part_valids", "part_label", "instance_label")

    def __init__(self, cfg):
        super().__init__(cfg)
        m = cfg.model
        self.encoder = build_encoder(m.encoder, feat_dim=self.pc_feat_dim, global_feat=True,
                                     pointnet2_eval=self.pointnet2_eval)
        self.corr_module = self._init_corr_module()
        self.pose_predictor = self._init_pose_predictor()

    def _init_corr_module(self):
        m = self.cfg.model
        return TransformerEncoder(d_model=self.pc_feat_dim, num_heads=m.transformer_heads,
                                  ffn_dim=m.transformer_feat_dim, num_layers=m.transformer_layers,
                                  norm_first=m.transformer_pre_ln)

    def _init_pose_predictor(self):
        dim = self.pc_feat_dim
        if self.semantic:
            dim += self.max_num_part
        if self.use_part_label:
            dim += self.cfg.data.num_part_category
        return StocasticPoseRegressor(feat_dim=dim, noise_dim=self.cfg.loss.noise_dim, rot_type=self.rot_type)

    def forward(self, data_dict):
        feats = data_dict.get("pre_pose_feats", None)
        if feats is None:
            part_valids = data_dict["part_valids"]
            pc_feats = self._extract_part_feats(data_dict["part_pcs"], part_valids)
            corr = self.corr_module(pc_feats, part_valids)  # (real iff == 1: applied inside the attention kernels)
            feats = torch.cat([corr, data_dict["part_label"].type_as(corr),
                               data_dict["instance_label"].type_as(corr)], dim=-1)
        rot, trans = self.pose_predictor(feats)
        return {"rot": self._wrap_rotation(rot), "trans": trans, "pre_pose_feats": feats}

    def _loss_function(self, data_dict, out_dict={}, optimizer_idx=-1):
        """One MoN sample; the encoder/transformer features are cached in `pre_pose_feats` because only the pose head
        is stochastic (network.py:106-139)."""
        return self._sample_loss(data_dict, out_dict, self.BATCH_KEYS, ("pre_pose_feats",))


class PosEncoder(nn.Module):
    """MLP positional encoding of a pose vector (network_refine.py:11-25); `layers.{0,2,..}` as upstream."""

    def __init__(self, dims):
        super().__init__()
        layers = []
        for i in range(len(dims) - 2):
            layers += [nn.Linear(dims[i], dims[i + 1]), nn.ReLU()]
        layers.append(nn.Linear(dims[-2], dims[-1]))
        self.layers = nn.Sequential(*layers)

    def forward(self, x):
        return self.layers(x)


class PNTransformerRefine(PNTransformer):
    """PNTransformer with iterative refinement (pn_transformer/network_refine.py:28-175): `refine_steps` rounds of
    [pose -> positional encoding, added to the part tokens -> that round's transformer -> that round's pose head];
    the loss is summed over the rounds.  Same sub-module names (`corr_module.{i}`, `pose_predictor.{i}`,
    `corr_pos_enc.layers.*`).  Each round's transformer and every loss evaluation run on the HIP path; the pose
    heads' odd input widths (features + 7 or 9 pose values) use the library-op fallback of `PoseRegressor`."""

    def __init__(self, cfg):
        self.refine_steps = cfg.model.refine_steps
        self.pose_pc_feat = cfg.model.pose_pc_feat
        super().__init__(cfg)  # (BaseModel registers `zero_pose`, the identity pose of cfg.model.rot_type)
        self.corr_pos_enc = PosEncoder([self.pose_dim, *cfg.model.transformer_pos_enc])

    def _init_corr_module(self):
        m = self.cfg.model
        return nn.ModuleList(
            TransformerEncoder(d_model=self.pc_feat_dim, num_heads=m.transformer_heads, ffn_dim=m.transformer_feat_dim,
                               num_layers=m.transformer_layers, norm_first=m.transformer_pre_ln,
                               out_dim=self.pc_feat_dim) for _ in range(self.refine_steps))

    def _init_pose_predictor(self):
        dim = self.pc_feat_dim + self.pose_dim
        if self.semantic:
            dim += self.max_num_part
        if self.pose_pc_feat:
            dim += self.pc_feat_dim
        if self.use_part_label:
            dim += self.cfg.data.num_part_category
        return nn.ModuleList(
            StocasticPoseRegressor(feat_dim=dim, noise_dim=self.cfg.loss.noise_dim, rot_type=self.rot_type)
            for _ in range(self.refine_steps))

    def forward(self, data_dict):
        pc_feats = data_dict.get("pc_feats", None)
        part_valids = data_dict["part_valids"]
        if pc_feats is None:
            pc_feats = self._extract_part_feats(data_dict["part_pcs"], part_valids)
        part_label = data_dict["part_label"].type_as(pc_feats)
        inst_label = data_dict["instance_label"].type_as(pc_feats)
        B, P = inst_label.shape[:2]
        pose = self.zero_pose.to(pc_feats).expand(B, P, -1)
        valid_mask = part_valids  # (real iff == 1: applied inside the attention kernels)
        tokens, rots, transs = pc_feats, [], []
        for i in range(self.refine_steps):
            tokens = self.corr_module[i](tokens + self.corr_pos_enc(pose), valid_mask)
            feats = torch.cat([tokens, part_label, inst_label, pose], dim=-1)
            if self.pose_pc_feat:
                feats = torch.cat([pc_feats, feats], dim=-1)
            rot, trans = self.pose_predictor[i](feats)
            rots.append(rot)
            transs.append(trans)
            pose = torch.cat([rot, trans], dim=-1)
        if not self.training:
            return {"rot": self._wrap_rotation(rots[-1]), "trans": transs[-1], "pc_feats": pc_feats}
        # `_iters`: the per-round predictions as they were produced, for the loss (see DGLModel._forward)
        return {"rot": self._wrap_rotation(torch.stack(rots, dim=0)), "trans": torch.stack(transs, dim=0),
                "pc_feats": pc_feats, "_iters": [(self._wrap_rotation(r), t) for r, t in zip(rots, transs)]}

    def _loss_function(self, data_dict, out_dict={}, optimizer_idx=-1):
        """Loss of every round's prediction, summed (network_refine.py:131-175); `pc_feats` is reused across MoN samples."""
        if not self.training:
            return self._sample_loss(data_dict, out_dict, self.BATCH_KEYS, ("pc_feats",))
        pred = self.forward({k: data_dict[k] for k in self.BATCH_KEYS} | {"pc_feats": out_dict.get("pc_feats", None)})
        total, out = self._rounds_loss(pred["_iters"], data_dict)
        out["pc_feats"] = pred["pc_feats"]
        return total, out


def build_model(cfg):
    """Registry of reference models/__init__.py:10-26."""
    model = _build_model(cfg)
    TransformerEncoder.assign_dropout_salts(model)  # sibling encoders draw different masks, reproducibly
    return model


def _build_model(cfg):
    if cfg.model.name == "identity":
        from .identity import IdentityModel
        return IdentityModel(cfg)
    if cfg.model.name == "pn_transformer":
        return PNTransformer(cfg)
    if cfg.model.name == "pn_transformer_refine":
        return PNTransformerRefine(cfg)
    if cfg.model.name == "global":
        from .global_model import GlobalModel
        return GlobalModel(cfg)
    if cfg.model.name == "dgl":
        from .gnn import DGLModel
        return DGLModel(cfg)
    if cfg.model.name == "rgl_net":
        from .gnn import RGLNet
        return RGLNet(cfg)
    if cfg.model.name == "lstm":
        from .lstm import LSTMModel
        return LSTMModel(cfg)
    raise NotImplementedError(f"Model {cfg.model.name} not supported")
