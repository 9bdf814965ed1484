"""`Rotation3D` — mirror of the reference's rotation value type for quaternions and rotation matrices
(reference: multi_part_assembly/utils/rotation.py:91-309).

Two representations are carried, as a model can predict either (`cfg.model.rot_type`):
  * 'quat': [..., 4], real part first.  Semantics kept from the reference constructor (rotation.py:115-147): the
    tensor is cast to fp32 and quaternions whose norm is <= 0.5 (the all-zero rows of padded parts) are replaced by
    the identity (1, 0, 0, 0); nothing is normalised.
  * 'rmat': [..., 3, 3] row-major matrices.  The constructor also takes the 6D form of Zhou et al. (CVPR'19),
    [..., 6] or [..., 2, 3], and turns it into a matrix with pytorch3d's rotation_6d_to_matrix (rotation.py:150-165).
'axis' (axis-angle) is not provided: no model can predict it (the reference's regressor cannot build it either).
On CUDA tensors the quaternion -> matrix and 6D -> matrix conversions run in csrc/rmat.hip; matrix -> quaternion
(evaluation only, `to_euler`) runs on library operators.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

_TENSOR_METHODS = ("reshape", "view", "squeeze", "unsqueeze", "flatten", "unflatten", "transpose",
                   "permute", "contiguous", "to", "cuda", "type", "type_as", "detach", "clone")


_IDENT = {}


def _identity_quat(device):
    """(1, 0, 0, 0) on `device`, created once (the constructor runs several times per training step)."""
    key = (device.type, device.index)
    if key not in _IDENT:
        _IDENT[key] = torch.tensor([1.0, 0.0, 0.0, 0.0], device=device)
    return _IDENT[key]


class _SanitizeFn(torch.autograd.Function):
    """Quaternions with norm <= 0.5 -> identity (the constructor rule); the gradient passes where the input was kept."""

    @staticmethod
    def forward(ctx, rot):
        from . import _lib
        q = rot.contiguous()
        out = torch.empty_like(q)
        keep = torch.empty(q.shape[:-1] + (1,), dtype=torch.float32, device=q.device)
        _lib.launch("mpa_quat_sanitize", q.device, q, q.numel() // 4, out, keep)
        ctx.save_for_backward(keep)
        return out

    @staticmethod
    def backward(ctx, grad):
        (keep,) = ctx.saved_tensors
        return grad * keep


# ---- conversions ------------------------------------------------------------------------------------------------
def normalize_rot6d(rot):
    """The reference's `normalize_rot6d` (models/modules/regressor.py:6-27) on library operators: [..., 6] or
    [..., 2, 3] -> same shape, the two 3-vectors normalised and made orthogonal (Gram-Schmidt)."""
    unflatten = rot.shape[-1] == 3
    if unflatten:
        rot = rot.flatten(-2, -1)
    a1, a2 = rot[..., :3], rot[..., 3:]
    b1 = F.normalize(a1, p=2, dim=-1)
    b2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = F.normalize(b2, p=2, dim=-1)
    rot = torch.cat([b1, b2], dim=-1)
    return rot.unflatten(-1, (2, 3)) if unflatten else rot


class _Rot6dFn(torch.autograd.Function):
    """[M, 6] -> [M, 3, 3] (csrc/rmat.hip), differentiable."""

    @staticmethod
    def forward(ctx, d6):
        from . import _lib
        M = d6.shape[0]
        out = torch.empty((M, 3, 3), dtype=torch.float32, device=d6.device)
        _lib.launch("mpa_rot6d_to_rmat_forward", d6.device, d6, M, out)
        ctx.save_for_backward(d6)
        return out

    @staticmethod
    def backward(ctx, grad):
        from . import _lib
        (d6,) = ctx.saved_tensors
        gd6 = torch.empty_like(d6)
        grad = grad.contiguous()
        _lib.launch("mpa_rot6d_to_rmat_backward", d6.device, d6, grad, d6.shape[0], gd6)
        return gd6


def rot6d_to_matrix(d6):
    """pytorch3d's rotation_6d_to_matrix: [..., 6] -> [..., 3, 3], rows b1, b2 (normalize_rot6d) and b3 = b1 x b2."""
    d6 = d6.float()
    lead = d6.shape[:-1]
    if d6.is_cuda:
        return _Rot6dFn.apply(d6.reshape(-1, 6).contiguous()).reshape(*lead, 3, 3)
    b = normalize_rot6d(d6)
    b1, b2 = b[..., :3], b[..., 3:]
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2)


def quat_to_matrix(quat):
    """pytorch3d's quaternion_to_matrix: [..., 4] (real part first) -> [..., 3, 3]; |q|^2 is summed left to right on both
    paths.  The device conversion carries no gradient (it converts ground-truth poses)."""
    quat = quat.float()
    lead = quat.shape[:-1]
    if quat.is_cuda:
        from . import _lib
        if quat.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("quat_to_matrix: the device conversion has no backward (it converts ground-truth poses)")
        q = quat.reshape(-1, 4).contiguous()
        out = torch.empty((q.shape[0], 3, 3), dtype=torch.float32, device=q.device)
        _lib.launch("mpa_quat_to_rmat", q.device, q, q.shape[0], out)
        return out.reshape(*lead, 3, 3)
    r, i, j, k = quat.unbind(-1)
    two_s = 2.0 / (((r * r + i * i) + j * j) + k * k)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(*lead, 3, 3)


def matrix_to_quaternion(matrix):
    """pytorch3d's matrix_to_quaternion on library operators: [..., 3, 3] -> [..., 4] (real part first, made
    non-negative).  The best-conditioned candidate is gathered on the device (no host copy)."""
    lead = matrix.shape[:-2]
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = matrix.reshape(*lead, 9).unbind(-1)
    s = torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], -1)
    q_abs = torch.sqrt(s.clamp_min(0.0))  # _sqrt_positive_part
    cand = torch.stack([
        torch.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], dim=-1),
        torch.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], dim=-1),
        torch.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], dim=-1),
        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], dim=-1),
    ], dim=-2)
    cand = cand / (2.0 * q_abs[..., None].clamp_min(0.1))
    best = q_abs.argmax(dim=-1)
    out = cand.gather(-2, best[..., None, None].expand(*lead, 1, 4)).squeeze(-2)
    return torch.where(out[..., 0:1] < 0, -out, out)


def _as_matrix(rot):
    """The 'rmat' constructor rule (reference rotation.py:150-165): [..., 3, 3] kept, [..., 6] / [..., 2, 3] -> matrix."""
    if rot.shape[-1] == 3 and rot.dim() >= 2:
        if rot.shape[-2] == 3:
            return rot
        if rot.shape[-2] == 2:
            return rot6d_to_matrix(rot.flatten(-2, -1))
        raise ValueError("wrong rotation matrix shape")
    if rot.shape[-1] == 6:
        return rot6d_to_matrix(rot)
    raise NotImplementedError("wrong rotation matrix shape")


class Rotation3D:
    ROT_TYPE = ["quat", "rmat"]

    def __init__(self, rot, rot_type="quat", _sanitized=False):
        """`_sanitized` (internal): `rot` is the float32 tensor of another Rotation3D passed through an operation that keeps
        every rotation as it is (detach, clone, a change of device) — the constructor rule is idempotent, so applying it
        again would be one more launch for the same values."""
        if _sanitized and rot.dtype == torch.float32 and (
                (rot_type == "quat" and rot.shape[-1] == 4) or (rot_type == "rmat" and rot.shape[-2:] == (3, 3))):
            self._rot, self._rot_type = rot, rot_type
            return
        if rot_type not in self.ROT_TYPE:
            raise NotImplementedError(f"rotation {rot_type!r}: only 'quat' and 'rmat' are supported")
        assert isinstance(rot, torch.Tensor), "rotation must be a tensor"
        if rot_type == "rmat":
            self._rot, self._rot_type = _as_matrix(rot.float()), rot_type
            return
        assert rot.shape[-1] == 4, "wrong quaternion shape"
        rot = rot.float()
        if rot.is_cuda:  # one HIP launch (csrc/pose.hip) instead of norm + compare + where
            self._rot = _SanitizeFn.apply(rot)
        else:
            with torch.no_grad():
                keep = rot.norm(p=2, dim=-1, keepdim=True) > 0.5
            self._rot = torch.where(keep, rot, _identity_quat(rot.device))  # [4] broadcasts over the batch
        self._rot_type = rot_type

    # --- value access -----------------------------------------------------------------------
    @property
    def rot(self):
        return self._rot

    @rot.setter
    def rot(self, value):
        self.__init__(value, self._rot_type)

    @property
    def rot_type(self):
        return self._rot_type

    def convert(self, rot_type):
        if rot_type not in self.ROT_TYPE:
            raise NotImplementedError(f"conversion to {rot_type!r} is not supported")
        if rot_type == self._rot_type:
            return self.clone()
        if rot_type == "rmat":
            return Rotation3D(quat_to_matrix(self._rot), "rmat", _sanitized=True)
        return Rotation3D(matrix_to_quaternion(self._rot), "quat")

    def to_quat(self):
        return self.convert("quat").rot

    def to_rmat(self):
        return self.convert("rmat").rot

    def to_euler(self, order="zyx", to_degree=True):
        """Euler angles [..., 3] (reference rotation.py:201-204; only its default convention is provided)."""
        if order != "zyx" or not to_degree:
            raise NotImplementedError("only the 'zyx' / degree convention of the evaluation metrics is provided")
        from .eval_utils import quat_to_euler_zyx_deg
        return quat_to_euler_zyx_deg(self.to_quat())

    # --- tensor-like surface ------------------------------------------------------------------
    shape = property(lambda self: self._rot.shape)
    device = property(lambda self: self._rot.device)
    dtype = property(lambda self: self._rot.dtype)

    def __len__(self):
        return self._rot.shape[0]

    def __getitem__(self, key):
        return Rotation3D(self._rot[key], self._rot_type)

    @staticmethod
    def _combine(op, rot_lst, dim):
        assert isinstance(rot_lst, (list, tuple)) and all(isinstance(r, Rotation3D) for r in rot_lst)
        assert all(r.rot_type == rot_lst[0].rot_type for r in rot_lst), "cannot combine different rotation types"
        return Rotation3D(op([r.rot for r in rot_lst], dim=dim), rot_lst[0].rot_type)

    @staticmethod
    def cat(rot_lst, dim=0):
        return Rotation3D._combine(torch.cat, rot_lst, dim)

    @staticmethod
    def stack(rot_lst, dim=0):
        return Rotation3D._combine(torch.stack, rot_lst, dim)


_VALUE_PRESERVING = ("detach", "clone", "contiguous", "cuda", "cpu")  # every rotation of the result is one of the input


def _delegate(name):
    def method(self, *args, **kwargs):
        return Rotation3D(getattr(self._rot, name)(*args, **kwargs), self._rot_type, _sanitized=name in _VALUE_PRESERVING)

    method.__name__ = name
    method.__doc__ = f"torch.Tensor.{name} applied to the wrapped rotation tensor."
    return method


for _name in _TENSOR_METHODS:
    setattr(Rotation3D, _name, _delegate(_name))
