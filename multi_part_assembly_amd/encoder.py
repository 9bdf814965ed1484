"""Per-part point-cloud encoders — mirrors of the reference's PointNet and DGCNN
(multi_part_assembly/models/modules/encoder/pointnet.py:6-41, dgcnn.py:8-109) with identical
constructor arguments, forward contract ([n, N, 3] -> [n, feat_dim]) and state_dict keys, so a
reference checkpoint loads unchanged (DGCNN registers every BatchNorm under two names, `bnK` and
`convK.1`, exactly as upstream).
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .gradsink import DeferredBackward, GradSink


class _PointNetFn(torch.autograd.Function):
    """PointNet forward/backward on the HIP library (csrc/pointnet.hip).  The bf16 performance variant
    (csrc/pointnet_bf16.hip, `_PointNetBF16Fn`) differs in the entry points' suffix and in its workspace only."""

    SUFFIX, LABEL = "", "PointNet"

    @staticmethod
    def _workspace(M, N, F_, dev):
        nf, ni = _lib.query("mpa_pointnet_workspace", M, N, F_)
        return (torch.empty(nf, dtype=torch.float32, device=dev), torch.empty(ni, dtype=torch.int32, device=dev))

    @classmethod
    def forward(cls, ctx, points, valids, training, momentum, eps, running, *params):
        conv_w, bn_w, bn_b = params[0:5], params[5:10], params[10:15]
        run_mean, run_var = running
        M, N, _ = points.shape
        F_ = conv_w[4].shape[0]
        dev = points.device
        ws = cls._workspace(M, N, F_, dev)
        feat = torch.empty((M, F_), dtype=torch.float32, device=dev)
        _lib.launch("mpa_pointnet_forward" + cls.SUFFIX, dev, points, valids, conv_w, bn_w, bn_b, run_mean, run_var,
                    training, float(momentum), float(eps), M, N, F_, *ws, feat,
                    timer=f"pointnet_forward{cls.SUFFIX}[{M}x{N}x{F_}]")
        ctx.training = bool(training)
        GradSink.register(ctx, params)
        ctx.save_for_backward(points, valids, *ws)
        return feat

    @classmethod
    def backward(cls, ctx, grad_feat):
        if not ctx.training:
            raise RuntimeError(f"{cls.LABEL}: backward is implemented for training-mode BatchNorm only")
        if DeferredBackward.active is not None:  # graph-mode data parallelism: run later, behind the first all-reduce
            saved = ctx.saved_tensors  # (autograd releases them when its own pass is over)
            DeferredBackward.park(lambda g: cls._run_backward(ctx, g, saved).accumulate(), grad_feat, ctx.params)
            return (None,) * len(ctx.needs_input_grad)
        grads = cls._run_backward(ctx, grad_feat, ctx.saved_tensors)
        return (None, None, None, None, None, None, *grads.handed_back())

    @classmethod
    def _run_backward(cls, ctx, grad_feat, saved):
        """The launch -> the parameter gradients it wrote (`gradsink.ParamGrads`)."""
        points, valids, *ws = saved
        params = ctx.params
        conv_w, bn_w = params[0:5], params[5:10]
        M, N, _ = points.shape
        F_ = conv_w[4].shape[0]
        grads = GradSink.outputs(params)
        g = grads.buffers
        _lib.launch("mpa_pointnet_backward" + cls.SUFFIX, points.device, grad_feat.contiguous(), points, valids, conv_w,
                    bn_w, M, N, F_, *ws, g[0:5], g[5:10], g[10:15],
                    timer=f"pointnet_backward{cls.SUFFIX}[{M}x{N}x{F_}]")
        return grads


class _PointNetBF16Fn(_PointNetFn):
    SUFFIX, LABEL = "_bf16", "PointNet (bf16)"

    @staticmethod
    def _workspace(M, N, F_, dev):
        return (torch.empty(_lib.query("mpa_pointnet_workspace_bf16", M, N, F_), dtype=torch.uint8, device=dev),)


# ---- configurations outside the HIP kernels' instantiation ------------------------------------------------------------------
# ONE policy for every module of the package (encoders here, TransformerEncoder in transformer.py): a configuration the
# hand-written kernels are not instantiated for — which the reference accepts (encoder/pointnet.py:6-41, dgcnn.py:41-109:
# any feat_dim, per-point features, any number of points) — runs on PyTorch-ROCm library operators through the module's
# own Conv / BatchNorm / Linear sub-modules, said aloud ONCE per module with a warning.  It is a slow path (the
# reference's own op sequence: edge tensors, one launch per op, a host sync to compact the valid parts), it is never taken
# by a shipped configuration, and it is still device-only: CPU tensors are rejected as everywhere else.
def _warn_library_path(module, what):
    if not getattr(module, "_warned_library", False):
        import warnings
        warnings.warn(f"{type(module).__name__}: {what} is outside the HIP kernels' instantiation; running this module on "
                      "library operators (slow path)")
        module._warned_library = True


def _run_valid_parts(fn, part_pcs, valids, feat_dim, per_point):
    """fn on the valid parts only, zeros elsewhere (the reference's `_extract_part_feats`: boolean-mask compaction — a
    host sync, accepted on the slow path)."""
    M, N, _ = part_pcs.shape
    keep = valids.reshape(-1) != 0
    out = part_pcs.new_zeros((M, N, feat_dim) if per_point else (M, feat_dim))
    if bool(keep.any()):
        out[keep] = fn(part_pcs[keep].float())
    return out


class PointNet(nn.Module):
    """Shared MLP 3-64-64-64-128-F (1x1 conv, no bias, BN, ReLU except after the last) + max over N.

    The Conv1d / BatchNorm1d sub-modules only hold the parameters and buffers (so state_dict keys and
    shapes equal the reference's); the computation runs on csrc/pointnet.hip.  `forward_parts` is the
    sync-free entry the assembly models use: all B*P part slots plus the validity mask.
    feat_dim outside {64, 128, 256} or per-point features (`global_feat=False`): library operators, see above."""

    WIDTHS = (3, 64, 64, 64, 128)

    def __init__(self, feat_dim, global_feat=True):
        super().__init__()
        self.feat_dim = feat_dim
        dims = (*self.WIDTHS, feat_dim)
        for i in range(5):
            setattr(self, f"conv{i + 1}", nn.Conv1d(dims[i], dims[i + 1], kernel_size=1, bias=False))
        for i in range(5):
            setattr(self, f"bn{i + 1}", nn.BatchNorm1d(dims[i + 1]))
        self.global_feat = global_feat
        # "fp32": the parity path (csrc/pointnet.hip).  "bf16": the separately named performance variant
        # (csrc/pointnet_bf16.hip, bench.py --dtype bf16) — bf16 activations and matrix-core GEMMs, fp32 statistics.
        self.precision = "fp32"

    def forward_parts(self, part_pcs, valids):
        """part_pcs [M, N, 3], valids [M] (1/0) -> [M, feat_dim]; rows of padded parts are zero."""
        _lib.require_hip("PointNet", part_pcs)
        if not self._fused_ok():
            _warn_library_path(self, f"feat_dim = {self.feat_dim}, global_feat = {self.global_feat}")
            return _run_valid_parts(self._library_forward, part_pcs, valids, self.feat_dim, not self.global_feat)
        convs = [getattr(self, f"conv{i}") for i in range(1, 6)]
        bns = [getattr(self, f"bn{i}") for i in range(1, 6)]
        if self.training:
            with torch.no_grad():  # one multi-tensor launch for the five counters
                torch._foreach_add_([bn.num_batches_tracked for bn in bns], 1)
        running = ([bn.running_mean for bn in bns], [bn.running_var for bn in bns])
        if self.precision not in ("fp32", "bf16"):
            raise ValueError(f"PointNet.precision must be 'fp32' or 'bf16', not {self.precision!r}")
        fn = _PointNetFn if self.precision == "fp32" else _PointNetBF16Fn
        return fn.apply(
            part_pcs.detach().float().contiguous(), valids.detach().float().contiguous(), self.training,
            bns[0].momentum, bns[0].eps, running, *[c.weight for c in convs], *[b.weight for b in bns],
            *[b.bias for b in bns])

    def _fused_ok(self):
        return self.global_feat and self.feat_dim in (64, 128, 256) and not getattr(self, "force_library", False)

    def _library_forward(self, x):
        """[n, N, 3] -> [n, feat_dim] | [n, N, feat_dim] on library operators (pointnet.py:29-41)."""
        h = x.transpose(1, 2)
        for i in range(1, 6):
            h = getattr(self, f"bn{i}")(getattr(self, f"conv{i}")(h))
            if i < 5:
                h = F.relu(h)
        return h.amax(dim=-1) if self.global_feat else h.transpose(1, 2).contiguous()

    def forward(self, x):
        """x [n, N, 3] (every part valid) -> [n, feat_dim] ([n, N, feat_dim] per point); the reference's signature."""
        return self.forward_parts(x, torch.ones(x.shape[0], device=x.device))


def knn_exact(x, n, N, C=None):
    """Index-exact kNN graph (mpa_knn_exact, csrc/dg_knn.h): x [n*N, ld] row-major (C = 3: ld = 4, zero pad column)
    -> int32 [n*N, 20], best first, (score descending, index ascending)."""
    R, ld = x.shape
    C = (3 if ld == 4 else ld) if C is None else C
    idx = torch.empty((R, 20), dtype=torch.int32, device=x.device)
    ws = torch.empty(_lib.query("mpa_knn_exact_workspace", n, N), dtype=torch.uint8, device=x.device)
    _lib.launch("mpa_knn_exact", x.device, x, ld, n, N, C, ws, idx)
    return idx


class _DGCNNFn(torch.autograd.Function):
    """Whole DGCNN encoder forward/backward on the HIP library (csrc/dgcnn_enc.hip)."""

    @staticmethod
    def forward(ctx, points, valids, training, momentum, eps, running, want_point_grad, hooks, *params):
        conv_w, bn_w, bn_b, fc_w, fc_b = params[0:5], params[5:10], params[10:15], params[15], params[16]
        run_mean, run_var = running
        M, N, _ = points.shape
        F_ = fc_w.shape[0]
        dev = points.device
        ws = torch.empty(_lib.query("mpa_dgcnn_workspace", M, N, F_), dtype=torch.uint8, device=dev)
        feat = torch.empty((M, F_), dtype=torch.float32, device=dev)
        pts = points.detach()
        with torch.cuda.device(dev):
            # library-recorded events [2l] / [2l + 1] right around the kNN kernels of stage l
            knn_names = [f"dgcnn_knn[{M}x{N} stage {l + 1} C={C}]" for l, C in enumerate((3, 64, 64, 128))]
            pairs = [_lib.KernelTimer.phase_events([n]) for n in knn_names]
            flat = None
            if any(p is not None for p in pairs):
                flat = [e for p in pairs for e in (p if p is not None else [None, None])]
            graphs = hooks.get("graphs") if hooks else None
            if graphs is not None:  # parity tests: hold some stages' kNN graphs fixed (mpa_dgcnn_forward_graphs)
                graphs = [None if g is None else g.to(device=dev, dtype=torch.int32).contiguous() for g in graphs]
                # a hole (None) is a stage whose graph the forward builds itself, so the array is made here
                gp = (ctypes.c_void_p * 4)(*[None if g is None else g.data_ptr() for g in graphs])
                name, last = "mpa_dgcnn_forward_graphs", gp
            else:
                name, last = "mpa_dgcnn_forward", _lib.KernelTimer.handles(flat)
            _lib.launch(name, dev, pts, valids, conv_w, bn_w, bn_b, run_mean, run_var, fc_w, fc_b, training,
                        float(momentum), float(eps), M, N, F_, ws, feat, last, timer=f"dgcnn_forward[{M}x{N}x{F_}]")
            if hooks is not None and hooks.get("export"):
                out = []
                for l in range(4):
                    g = torch.empty((M * N, 20), dtype=torch.int32, device=dev)
                    _lib.launch("mpa_dgcnn_export_graph", dev, ws, M, N, F_, l, g)
                    out.append(g)
                hooks["exported"] = out
            if hooks is not None and hooks.get("export_selection"):
                out = []
                for l, width in enumerate((64, 64, 128, 256, F_)):
                    t = torch.empty((M * N, width) if l < 4 else (M, F_), dtype=torch.int32, device=dev)
                    _lib.launch("mpa_dgcnn_export_selection", dev, ws, M, N, F_, l, t)
                    out.append(t)
                hooks["selection"] = out
                out = []
                for l, width in enumerate((64, 64, 128, 256, F_)):
                    t = torch.empty((M * N, width), dtype=torch.int32, device=dev)
                    _lib.launch("mpa_dgcnn_export_branch", dev, ws, M, N, F_, l, t)
                    out.append(t)
                hooks["branch"] = out
            for n, p in zip(knn_names, pairs):
                _lib.KernelTimer.add_phases([n], p)
        ctx.training = bool(training)
        ctx.want_point_grad = bool(want_point_grad)
        GradSink.register(ctx, params)
        ctx.save_for_backward(pts, ws)
        return feat

    @staticmethod
    def backward(ctx, grad_feat):
        if not ctx.training:
            raise RuntimeError("DGCNN: backward is implemented for training-mode BatchNorm only")
        if DeferredBackward.active is not None and not ctx.want_point_grad:
            saved = ctx.saved_tensors
            DeferredBackward.park(lambda g: _DGCNNFn._run_backward(ctx, g, saved)[1].accumulate(), grad_feat, ctx.params)
            return (None,) * len(ctx.needs_input_grad)
        gpts, grads = _DGCNNFn._run_backward(ctx, grad_feat, ctx.saved_tensors)
        return (gpts, None, None, None, None, None, None, None, *grads.handed_back())

    @staticmethod
    def _run_backward(ctx, grad_feat, saved):
        if getattr(ctx, "consumed", False):
            raise RuntimeError("DGCNN: the backward pass overwrites its saved workspace (y5 becomes dY5, dhcat is "
                               "accumulated in place): a second backward over the same forward is not supported — "
                               "run the forward again")
        ctx.consumed = True
        pts, ws = saved
        params = ctx.params
        conv_w, bn_w, fc_w = params[0:5], params[5:10], params[15]
        M, N, _ = pts.shape
        F_ = fc_w.shape[0]
        dev = pts.device
        # with a GradSink the kernels write the parameter gradients straight into the flat gradient buffer (every output
        # is overwritten in full) instead of 17 AccumulateGrad `add_` launches
        grads = GradSink.outputs(params)
        g = grads.buffers
        gpts = torch.empty_like(pts) if ctx.want_point_grad else None
        _lib.launch("mpa_dgcnn_backward", dev, grad_feat.contiguous(), conv_w, bn_w, fc_w, M, N, F_, ws, g[0:5],
                    g[5:10], g[10:15], g[15], g[16], gpts, timer=f"dgcnn_backward[{M}x{N}x{F_}]")
        return gpts, grads


class DGCNN(nn.Module):
    """4 EdgeConv stages (k=20, widths 64-64-128-256, LeakyReLU 0.2, max over k), concat 512 ->
    1x1 conv -> [max ; mean] over N -> Linear.

    The sub-modules hold the parameters under the reference's names (state_dict keys as upstream, every BatchNorm
    under `bnK` and `convK.1`); the computation is ONE library call forward and one backward (csrc/dgcnn_enc.hip:
    index-exact kNN on the matrix cores, one exact-fp32 MFMA GEMM per point instead of per edge, LDS-resident
    gather / BatchNorm2d / LeakyReLU / max, HIP tail).  `forward_parts` is the sync-free entry of the assembly
    models: all part slots plus the validity mask, zeros out for padded parts.

    Outside the kernels' instantiation (per-point features, more than 1024 points per cloud, feat_dim not in
    {64, 128, 256}) the module runs on library operators (the policy stated above PointNet; every shipped
    configuration — 1000 points per part, global feature — is inside).  Fewer than 20 points per cloud fail as they do
    upstream: a 20-nearest-neighbour graph does not exist."""

    MAX_POINTS = 1024

    def __init__(self, feat_dim, global_feat=True):
        super().__init__()
        self.bn1, self.bn2 = nn.BatchNorm2d(64), nn.BatchNorm2d(64)
        self.bn3, self.bn4 = nn.BatchNorm2d(128), nn.BatchNorm2d(256)
        self.bn5 = nn.BatchNorm1d(feat_dim)
        act = lambda: nn.LeakyReLU(negative_slope=0.2)
        self.conv1 = nn.Sequential(nn.Conv2d(6, 64, kernel_size=1, bias=False), self.bn1, act())
        self.conv2 = nn.Sequential(nn.Conv2d(128, 64, kernel_size=1, bias=False), self.bn2, act())
        self.conv3 = nn.Sequential(nn.Conv2d(128, 128, kernel_size=1, bias=False), self.bn3, act())
        self.conv4 = nn.Sequential(nn.Conv2d(256, 256, kernel_size=1, bias=False), self.bn4, act())
        self.conv5 = nn.Sequential(nn.Conv1d(512, feat_dim, kernel_size=1, bias=False), self.bn5, act())
        self.global_feat = global_feat
        self.feat_dim = feat_dim
        if global_feat:
            self.out_fc = nn.Linear(feat_dim * 2, feat_dim)
        # parity-test hooks (None in production): {"graphs": [4 x (None | int32 [nv*N, 20])]} holds stages' kNN graphs
        # fixed; {"export": True} leaves the graphs the forward built under "exported" ([M*N, 20] int32 per stage);
        # {"export_selection": True} leaves the maxima it took under "selection" (the neighbour slot, [M*N, CO] int32 per
        # stage, and the pooled point, [M, F]) and the LeakyReLU slopes its backward will take under "branch"
        # ([M*N, CO] per stage and [M*N, F] for the tail, 1 = unit slope); rows past the valid parts are -1
        self.graph_hooks = None

    def _fused_ok(self, N):
        return (self.global_feat and self.feat_dim in (64, 128, 256) and 20 <= N <= self.MAX_POINTS
                and not getattr(self, "force_library", False))

    @staticmethod
    def _edge_tensor(h, k=20):
        """h [n, C, N] -> [n, 2C, N, k]: (neighbour - centre ; centre) over the k best of 2 x.y - |x|^2 - |y|^2
        (dgcnn.py:8-38)."""
        rows = h.transpose(1, 2)                                     # [n, N, C]
        sq = (rows * rows).sum(dim=-1)                               # [n, N]
        score = 2.0 * torch.matmul(rows, h) - sq[:, :, None] - sq[:, None, :]
        idx = score.topk(k, dim=-1).indices                         # [n, N, k] (the centre itself included)
        n, N, C = rows.shape
        nb = torch.gather(rows[:, None].expand(n, N, N, C), 2, idx[..., None].expand(n, N, k, C))
        centre = rows[:, :, None].expand(n, N, k, C)
        return torch.cat([nb - centre, centre], dim=-1).permute(0, 3, 1, 2)

    def _library_forward(self, x):
        """[n, N, 3] -> [n, feat_dim] | [n, N, feat_dim] on library operators (dgcnn.py:73-109)."""
        if x.shape[1] < 20:
            raise RuntimeError(f"DGCNN: a 20-nearest-neighbour graph needs at least 20 points per cloud, got {x.shape[1]}")
        h = x.transpose(1, 2)
        stages = []
        for conv in (self.conv1, self.conv2, self.conv3, self.conv4):
            h = conv(self._edge_tensor(h)).amax(dim=-1)
            stages.append(h)
        h = self.conv5(torch.cat(stages, dim=1))
        if not self.global_feat:
            return h.transpose(1, 2).contiguous()
        return self.out_fc(torch.cat([h.amax(dim=-1), h.mean(dim=-1)], dim=1))

    def forward_parts(self, part_pcs, valids):
        """part_pcs [M, N, 3], valids [M] (1/0) -> [M, feat_dim]; rows of padded parts are zero."""
        _lib.require_hip("DGCNN", part_pcs)
        M, N, _ = part_pcs.shape
        if not self._fused_ok(N):
            _warn_library_path(self, f"N = {N}, feat_dim = {self.feat_dim}, global_feat = {self.global_feat}")
            return _run_valid_parts(self._library_forward, part_pcs, valids, self.feat_dim, not self.global_feat)
        bns = [self.bn1, self.bn2, self.bn3, self.bn4, self.bn5]
        convs = [self.conv1[0], self.conv2[0], self.conv3[0], self.conv4[0], self.conv5[0]]
        if self.training:
            with torch.no_grad():
                torch._foreach_add_([bn.num_batches_tracked for bn in bns], 1)
        running = ([bn.running_mean for bn in bns], [bn.running_var for bn in bns])
        return _DGCNNFn.apply(
            part_pcs.float().contiguous(), valids.detach().float().contiguous(), self.training, bns[0].momentum,
            bns[0].eps, running, part_pcs.requires_grad, self.graph_hooks, *[c.weight for c in convs], *[b.weight for b in bns],
            *[b.bias for b in bns], self.out_fc.weight, self.out_fc.bias)

    def forward(self, x):
        """x [n, N, 3] -> [n, feat_dim] (global feature) or [n, N, feat_dim]; the reference's signature."""
        _lib.require_hip("DGCNN", x)
        return self.forward_parts(x, torch.ones(x.shape[0], device=x.device))


def build_encoder(arch, feat_dim, global_feat=True, **kwargs):
    """Registry of reference encoder/__init__.py:6-21: `pointnet` and `dgcnn` (whole encoders on HIP kernels) and
    `pointnet2_ssg` (pointnet2.py: HIP sampling and grouping, the shared MLPs on library operators; global feature
    only, as upstream; `pointnet2_eval` = cfg.model.pointnet2_eval picks its evaluation path, other encoders ignore it).
    `pointnet2_msg`, the multi-scale variant, is not in the registry yet: the class exists (pointnet2.PointNet2MSG), the
    refusal below is what tests/test_pointnet2_encoder.py pins."""
    if arch == "pointnet":
        return PointNet(feat_dim, global_feat=global_feat)
    if arch == "dgcnn":
        return DGCNN(feat_dim, global_feat=global_feat)
    if arch == "pointnet2_ssg":
        if not global_feat:
            raise ValueError("pointnet2_ssg gives a global feature only (global_feat=True), as in the reference")
        from .pointnet2 import PointNet2SSG
        return PointNet2SSG(feat_dim).set_eval_mlp(kwargs.get("pointnet2_eval", "library"))
    if arch == "pointnet2_msg":
        raise NotImplementedError("pointnet2_msg is not supported: the multi-scale-grouping PointNet++ encoder (MSG) is not "
                                  "built; use pointnet2_ssg")
    raise NotImplementedError(f"{arch} is not supported")
