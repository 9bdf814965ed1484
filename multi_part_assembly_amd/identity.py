"""`IdentityModel` — the trivial baseline that predicts the identity rotation and a zero translation for every part
(reference: multi_part_assembly/models/b_identity/network.py:4-60).  No parameters; `load_state_dict` accepts anything
and does nothing, so the test entry point needs no weight file for it (scripts/test.py:93-94)."""
from __future__ import annotations

from .base_model import BaseModel


class IdentityModel(BaseModel):
    def forward(self, data_dict):
        part_pcs = data_dict["part_pcs"]
        B, P = part_pcs.shape[:2]
        zero_pose = self.zero_pose.repeat(B, P, 1).type_as(part_pcs)
        return {"rot": self._wrap_rotation(zero_pose[..., :-3]), "trans": zero_pose[..., -3:], "pre_pose_feats": None}

    def _loss_function(self, data_dict, out_dict={}, optimizer_idx=-1):
        return self._calc_loss(self.forward({"part_pcs": data_dict["part_pcs"]}), data_dict)

    def load_state_dict(self, *args, **kwargs):
        pass
