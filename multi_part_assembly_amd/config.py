"""Configuration values of the shipped experiments, restated as plain attribute dictionaries.

The reference builds yacs CfgNodes from configs/**.py (utils/config_utils.py:6-19); the build ships
no yacs, so the values the hot path reads (`cfg.model.*`, `cfg.loss.*`, `cfg.data.*`,
`cfg.optimizer.*`, `cfg.exp.*`) are restated here, each citing its reference file.
"""
from __future__ import annotations


class Config(dict):
    """Attribute-style nested dict exposing the CfgNode calls the models use (`get`, `clone`)."""

    def __getattr__(self, key):
        try:
            return self[key]
        except KeyError as exc:
            raise AttributeError(key) from exc

    def __setattr__(self, key, value):
        self[key] = value

    def clone(self):
        return Config({k: (v.clone() if isinstance(v, Config) else v) for k, v in self.items()})


def geometric_loss():
    """configs/_base_/models/loss/geometric_loss.py:17-27."""
    return Config(noise_dim=0, trans_loss_w=1.0, rot_pt_cd_loss_w=10.0, transform_pt_cd_loss_w=10.0,
                  use_rot_loss=True, rot_loss_w=0.2, use_rot_pt_l2_loss=True, rot_pt_l2_loss_w=1.0)


def semantic_loss():
    """configs/_base_/models/loss/semantic_loss.py:12-23."""
    return Config(noise_dim=32, sample_iter=5, trans_loss_w=1.0, rot_pt_cd_loss_w=10.0,
                  transform_pt_cd_loss_w=10.0, use_rot_loss=False, use_rot_pt_l2_loss=False)


def part_palette(count=24):
    """RGB rows (0-255) that colour the parts of an exported assembly by their order (`cfg.data.colors`).  The project's
    own table: hues step by the golden angle, so neighbouring parts never look alike, at three alternating
    saturation / value levels; exact integers from integer arithmetic (HSV -> RGB in sixths of the hue circle)."""
    rows = []
    for k in range(count):
        hue = (k * 137) % 360                      # degrees
        sat, val = ((200, 230), (255, 180), (140, 255))[k % 3]
        c = val * sat // 255
        x = c * (60 - abs(hue % 120 - 60)) // 60
        m = val - c
        r, g, b = ((c, x, 0), (x, c, 0), (0, c, x), (0, x, c), (x, 0, c), (c, 0, x))[hue // 60]
        rows.append((r + m, g + m, b + m))
    return tuple(rows)


def breaking_bad_everyday():
    """configs/_base_/datasets/breaking_bad/everyday.py:5-16 (+ the colour table of exported assemblies)."""
    return Config(dataset="geometry", data_keys=("part_ids",), num_pc_points=1000, min_num_part=2,
                  max_num_part=20, colors=part_palette())


def adam_cosine():
    """configs/_base_/schedules/adam_cosine.py:5-11."""
    return Config(lr=1e-3, weight_decay=0.0, warmup_ratio=0.0, clip_grad=None, lr_scheduler="cosine",
                  lr_decay_factor=100.0)


def pn_transformer_model():
    """configs/_base_/models/pn_transformer/pn_transformer.py:5-15."""
    return Config(name="pn_transformer", rot_type="quat", pc_feat_dim=256, encoder="pointnet",
                  transformer_feat_dim=1024, transformer_heads=8, transformer_layers=4,
                  transformer_pre_ln=True)


def pn_transformer_everyday():
    """configs/pn_transformer/pn_transformer/pn_transformer-32x1-cosine_400e-everyday.py."""
    opt = adam_cosine()
    opt.warmup_ratio = 0.05
    return Config(exp=Config(batch_size=32, num_epochs=400, num_workers=8, gpus=[0]),
                  data=breaking_bad_everyday(), optimizer=opt, model=pn_transformer_model(),
                  loss=geometric_loss())


def partnet_chair():
    """configs/_base_/datasets/partnet/partnet_chair.py:5-16."""
    return Config(dataset="partnet", data_keys=("part_ids", "match_ids", "contact_points"), num_pc_points=1000,
                  num_part_category=57, min_num_part=2, max_num_part=20, colors=part_palette())


def dgl_model():
    """configs/_base_/models/dgl.py:5-18."""
    return Config(name="dgl", rot_type="quat", pc_feat_dim=128, encoder="pointnet", gnn_iter=3, merge_node=True)


def rgl_net_model():
    """configs/_base_/models/rgl_net.py:5-14."""
    return Config(name="rgl_net", rot_type="quat", pc_feat_dim=128, encoder="pointnet", gnn_iter=3, merge_node=True)


def global_model():
    """configs/_base_/models/global.py:5-11."""
    return Config(name="global", rot_type="quat", pc_feat_dim=128, encoder="pointnet")


def _exp(epochs):
    return Config(batch_size=32, num_epochs=epochs, num_workers=8, gpus=[0])


def dgl_everyday():
    """configs/dgl/dgl-32x1-cosine_200e-everyday.py: no equivalent parts in geometric data -> merge_node off."""
    model = dgl_model()
    model.merge_node = False
    data = breaking_bad_everyday()
    data.data_keys = ("part_ids", "valid_matrix")
    return Config(exp=_exp(200), data=data, optimizer=adam_cosine(), model=model, loss=geometric_loss())


def rgl_net_everyday():
    """configs/rgl_net/rgl_net-32x1-cosine_200e-everyday.py (merge_node stays on: the second relation net is used
    at odd iterations even though geometric data never merges nodes)."""
    model = rgl_net_model()
    data = breaking_bad_everyday()
    data.data_keys = ("part_ids", "valid_matrix")
    return Config(exp=_exp(200), data=data, optimizer=adam_cosine(), model=model, loss=geometric_loss())


def dgl_dgcnn_everyday():
    """BASELINE.json configs[2]: DGL with the DGCNN part encoder (`cfg.model.encoder = 'dgcnn'`, allowed by
    models/modules/encoder/__init__.py:6-21; no shipped config file sets it)."""
    cfg = dgl_everyday()
    cfg.model.encoder = "dgcnn"
    return cfg


def rgl_net_dgcnn_artifact():
    """BASELINE.json configs[4]: RGL-NET with the DGCNN part encoder on the Breaking-Bad artifact subset
    (configs/_base_/datasets/breaking_bad/artifact.py: same keys as everyday, other data list)."""
    cfg = rgl_net_everyday()
    cfg.model.encoder = "dgcnn"
    # many small parts per shape: both Chamfer terms of the loss on per-part k-d leaves (csrc/leaf_nn.hip; identical
    # results; the step: 21.64 ms with the grid, 21.15 with the per-sample route "auto", 20.90 with "leaf" on one box)
    cfg.loss.shape_search = "leaf"
    return cfg


def global_everyday():
    """configs/global/global-32x1-cosine_200e-everyday.py."""
    return Config(exp=_exp(200), data=breaking_bad_everyday(), optimizer=adam_cosine(), model=global_model(),
                  loss=geometric_loss())


def global_partnet_chair():
    """configs/global/global-32x1-cosine_200e-partnet_chair.py (semantic data: matching + min-of-N)."""
    return Config(exp=_exp(200), data=partnet_chair(), optimizer=adam_cosine(), model=global_model(),
                  loss=semantic_loss())


def _partnet_chair_graph_data():
    """The data block of configs/{dgl,rgl_net}/*-partnet_chair.py: the graph networks also read the valid matrix."""
    data = partnet_chair()
    data.data_keys = ("part_ids", "match_ids", "contact_points", "valid_matrix")
    return data


def dgl_partnet_chair():
    """configs/dgl/dgl-32x1-cosine_300e-partnet_chair.py (semantic data: matching + min-of-N, equivalent parts merged at
    odd GNN iterations; 300 epochs)."""
    return Config(exp=_exp(300), data=_partnet_chair_graph_data(), optimizer=adam_cosine(), model=dgl_model(),
                  loss=semantic_loss())


def rgl_net_partnet_chair():
    """configs/rgl_net/rgl_net-32x1-cosine_300e-partnet_chair.py (as DGL's; the parts are shuffled to avoid part-label
    leakage from their order)."""
    data = _partnet_chair_graph_data()
    data.shuffle_parts = True
    return Config(exp=_exp(300), data=data, optimizer=adam_cosine(), model=rgl_net_model(), loss=semantic_loss())


def pn_transformer_partnet_chair():
    """configs/pn_transformer/pn_transformer/pn_transformer-32x1-cosine_400e-partnet_chair.py."""
    opt = adam_cosine()
    opt.warmup_ratio = 0.05
    return Config(exp=_exp(400), data=partnet_chair(), optimizer=opt, model=pn_transformer_model(), loss=semantic_loss())


def pn_transformer_refine_model():
    """configs/_base_/models/pn_transformer/pn_transformer_refine.py:5-19."""
    return Config(name="pn_transformer_refine", rot_type="quat", pc_feat_dim=128, encoder="pointnet",
                  transformer_pos_enc=(128, 128), transformer_feat_dim=512, transformer_heads=8,
                  transformer_layers=2, transformer_pre_ln=True, pose_pc_feat=True, refine_steps=3)


def pn_transformer_refine_everyday():
    """configs/pn_transformer/pn_transformer_refine/pn_transformer_refine-32x1-cosine_400e-everyday.py."""
    opt = adam_cosine()
    opt.warmup_ratio = 0.05
    return Config(exp=_exp(400), data=breaking_bad_everyday(), optimizer=opt, model=pn_transformer_refine_model(),
                  loss=geometric_loss())


def lstm_model():
    """configs/_base_/models/lstm.py:5-13."""
    return Config(name="lstm", rot_type="quat", pc_feat_dim=128, encoder="pointnet", lstm_hidden_size=256)


def breaking_bad_artifact():
    """configs/_base_/datasets/breaking_bad/artifact.py: the keys and sizes of everyday, another data list."""
    return breaking_bad_everyday()


def lstm_everyday():
    """configs/lstm/lstm-32x1-cosine_200e-everyday.py."""
    return Config(exp=_exp(200), data=breaking_bad_everyday(), optimizer=adam_cosine(), model=lstm_model(),
                  loss=geometric_loss())


def lstm_artifact():
    """configs/lstm/lstm-32x1-cosine_200e-artifact.py."""
    return Config(exp=_exp(200), data=breaking_bad_artifact(), optimizer=adam_cosine(), model=lstm_model(),
                  loss=geometric_loss())


def lstm_partnet_chair():
    """configs/lstm/lstm-32x1-cosine_200e-partnet_chair.py (semantic data: matching + min-of-N; the parts are shuffled
    to avoid part-label leakage from their order)."""
    data = partnet_chair()
    data.shuffle_parts = True
    return Config(exp=_exp(200), data=data, optimizer=adam_cosine(), model=lstm_model(), loss=semantic_loss())


def identity_model():
    """configs/_base_/models/identity.py:5-8."""
    return Config(name="identity", rot_type="quat", pc_feat_dim=128)


def identity_everyday():
    """configs/identity/identity-32x1-cosine_200e-everyday.py (the shipped file pairs geometric data with the semantic
    loss settings: five identical samples, no cosine / L2 rotation terms)."""
    return Config(exp=_exp(200), data=breaking_bad_everyday(), optimizer=adam_cosine(), model=identity_model(),
                  loss=semantic_loss())


def identity_artifact():
    """configs/identity/identity-32x1-cosine_200e-artifact.py."""
    return Config(exp=_exp(200), data=breaking_bad_artifact(), optimizer=adam_cosine(), model=identity_model(),
                  loss=semantic_loss())


def identity_partnet_chair():
    """configs/identity/identity-32x1-cosine_200e-partnet_chair.py."""
    return Config(exp=_exp(200), data=partnet_chair(), optimizer=adam_cosine(), model=identity_model(),
                  loss=semantic_loss())


# the category lists scripts/test.py loops over with `--category all` (configs/_base_/datasets/breaking_bad/*.py)
EVERYDAY_CATEGORIES = ("BeerBottle", "Bowl", "Cup", "DrinkingUtensil", "Mug", "Plate", "Spoon", "Teacup", "ToyFigure",
                       "WineBottle", "Bottle", "Cookie", "DrinkBottle", "Mirror", "PillBottle", "Ring", "Statue", "Teapot",
                       "Vase", "WineGlass")
