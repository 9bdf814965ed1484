"""Float64-anchored bars for the HIP-vs-oracle tests (a plain module, imported like tests/eval_ref.py).

Every compared tensor — an output, a running statistic, an input or parameter gradient — is measured against the float64
evaluation of the CPU oracle (oracle/nets.py, oracle/geometry.py evaluate in float64 when their inputs are float64), and
the bar comes from the FLOAT32 CPU oracle's own distance to that anchor on the same inputs, never from the HIP path:

    err(a, r64) = max|a - r64| / max|r64|                                     (per tensor, in float64)
    e32_k       = err(float32 oracle, float64 oracle) of tensor k
    bar_k       = min(CEIL, MULT * max(e32_k, median of e32 over the tensors of the call))

CEIL = 1e-4 is the project's parity bar (the loss terms of tests/test_callers_gpu.py) and is never raised.  MULT = 8: the HIP
path is float32-grade arithmetic in another summation order (the split-bf16 products drop terms at the 2^-24 level), and two
float32-grade evaluations of a max-norm error differ by a small factor, not by orders of magnitude.  The median term keeps a
tensor on which the CPU float32 run happens to be nearly exact (a bias gradient summed over a few terms) from getting a bar
below rounding.  A gradient that is structurally zero (a bias in front of a normalisation: float64 gradient below 1e-9 of
its layer's weight-gradient scale) is held to the absolute rule of tests/test_callers_gpu.py: 1e-5 of that scale.

tests/test_anchored.py shows on the CPU that these bars accept a re-associated float32 evaluation and reject a weight that
lost the third term of its bf16 split, a wrong epsilon and one gradient tensor off by 2e-5; for the single layers of
csrc/gru.hip and csrc/mlp.hip (the cases at the end of this file, whose only ReLU is pinned by `_pin_relu`) a GRU with b_hn
outside the reset product, a running variance from the biased variance and swapped weight halves of the pair layer.
"""
import math
import statistics

import torch

from oracle import nets as on

CEIL = 1e-4
MULT = 8.0
ZERO_REL = 1e-9   # float64 gradient below this fraction of its layer's weight-gradient scale: structurally zero
ZERO_ABS = 1e-5   # ... and then the compared gradient must stay below this fraction of that scale


def _f64(t):
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    return t.detach().cpu().double()


def err(a, r64):
    """max|a - r64| / max|r64| in float64 (0 for two all-zero tensors)."""
    a, r = _f64(a), _f64(r64)
    assert a.shape == r.shape, (tuple(a.shape), tuple(r.shape))
    if r.numel() == 0:
        return 0.0
    d, s = float((a - r).abs().max()), float(r.abs().max())
    if math.isnan(d):
        return math.inf
    return 0.0 if d == 0.0 else (d / s if s > 0.0 else math.inf)


def oracle_run(fn, sd, inputs, wrt=(), dtype=torch.float64):
    """One evaluation of `fn(sd, inputs) -> (outs: dict of tensors, scalar loss)` — a callable over oracle.nets — on the
    CPU in `dtype`, cast from the given (float32) values.  Floating-point entries of `sd` other than BatchNorm's running
    statistics are parameters; `wrt` names the entries of `inputs` to differentiate.  Returns a dict of float64 CPU
    tensors: `out.<name>`, `gin.<input>` and `grad.<parameter>`."""
    cast = lambda v: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()).clone()
    sdc = {k: cast(v) for k, v in sd.items()}
    params = {k: v.requires_grad_() for k, v in sdc.items() if v.is_floating_point() and "running_" not in k}
    inp = {k: (cast(v) if torch.is_tensor(v) else v) for k, v in inputs.items()}
    for k in wrt:
        inp[k].requires_grad_()
    outs, loss = fn(sdc, inp)
    loss.backward()
    r = {"out." + k: _f64(v) for k, v in outs.items()}
    r.update({"gin." + k: _f64(inp[k].grad) for k in wrt})
    r.update({"grad." + k: _f64(p.grad) for k, p in params.items() if p.grad is not None})
    return r


def oracle_pair(fn, sd, inputs, wrt=()):
    """(r32, r64): `oracle_run` in float32 and in float64; the float64 copies are made from the same float32 values."""
    return oracle_run(fn, sd, inputs, wrt, torch.float32), oracle_run(fn, sd, inputs, wrt, torch.float64)


def _zero_scale(k, r64):
    """Weight-gradient scale of the layer if `k` is a bias gradient that is structurally zero in float64, else None."""
    if not (k.startswith("grad.") and k.endswith(".bias")):
        return None
    wk = k[:-len("bias")] + "weight"
    if wk not in r64:
        return None
    ws = float(_f64(r64[wk]).abs().max())
    return ws if ws > 0.0 and float(_f64(r64[k]).abs().max()) < ZERO_REL * ws else None


def bars(r32, r64, keys=None):
    """(e32, bar, median of e32) over the tensors of one call — `keys`, the compared ones; by default every tensor that
    r32 and r64 share; structurally zero gradients take no part."""
    keys = [k for k in (r64 if keys is None else keys) if k in r32 and k in r64 and _zero_scale(k, r64) is None]
    e32 = {k: err(r32[k], r64[k]) for k in keys}
    med = statistics.median(e32.values()) if e32 else 0.0
    return e32, {k: min(CEIL, MULT * max(e32[k], med)) for k in keys}, med


def check(got, r32, r64):
    """Compare every tensor of `got` with the float64 anchor.  Returns (rows, failures): rows = (err, e32, bar, name) of
    the tensors under the relative bar, failures = the descriptions of everything that missed its bar.  The median term
    of the bars is taken over the tensors of `got` only, however much more r32 and r64 hold."""
    e32, bar, med = bars(r32, r64, list(got))
    rows, bad = [], []
    for k, a in got.items():
        assert k in r64 and k in r32, f"{k}: no float64 anchor or no float32 reference"
        ws = _zero_scale(k, r64)
        if ws is not None:
            top = float(_f64(a).abs().max())
            if not top <= ZERO_ABS * ws:
                bad.append(f"{k}: structurally zero, |g| {top:.2e} > {ZERO_ABS:g} x {ws:.2e}")
            continue
        e = err(a, r64[k])
        rows.append((e, e32[k], bar[k], k))
        if not e <= bar[k]:
            bad.append(f"{k}: {e:.2e} > bar {bar[k]:.2e} (e32 {e32[k]:.2e}, median e32 {med:.2e})")
    return rows, bad


def summary(label, rows, r32, r64):
    e32, _, med32 = bars(r32, r64, [r[3] for r in rows])
    worst, w32 = max(rows), max(e32, key=e32.get)
    med = statistics.median(r[0] for r in rows)
    ratio, at = max((r[0] / max(r[1], med32, 1e-300), r[3]) for r in rows)
    return (f"{label}: {len(rows)} tensors vs float64: worst {worst[0]:.2e} ({worst[3]}; e32 there {worst[1]:.2e}, bar "
            f"{worst[2]:.2e}), median {med:.2e}; float32 oracle: worst e32 {e32[w32]:.2e} ({w32}), median {med32:.2e}; "
            f"largest hip / max(e32, median e32) {ratio:.2f} of {MULT:g} ({at})")


def assert_anchored(got, r32, r64, label="", capsys=None):
    """Assert that every tensor of `got` is within its bar of the float64 anchor `r64`; `r32` is the float32 reference
    the bar is derived from (the float32 CPU oracle, or a fixture's recorded float32 reference).  Prints one line (through
    `capsys.disabled()` when given) before it asserts, and names every tensor that missed."""
    rows, bad = check(got, r32, r64)
    line = summary(label, rows, r32, r64) if rows else f"{label}: no tensor under a relative bar"
    if capsys is not None:
        with capsys.disabled():
            print("\n  " + line, end="")
    assert not bad, line + "\n  " + "\n  ".join(bad)
    return rows


def assert_bit_equal(a, b):
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: two runs differ"


# ---- the cases: shared by the GPU tests and by the CPU tests of these bars (tests/test_anchored.py) --------------------

# (M, N, F), valids (None = all): the smallest shapes that reach each structural edge of the launch plan of
# csrc/pointnet.hip (mpa_pointnet_forward / mpa_pointnet_backward); see tests/test_pointnet_anchored_gpu.py
POINTNET_CASES = [
    ((33, 1, 64), None),
    ((5, 31, 128), None),
    ((1, 33, 64), None),
    ((6, 64, 256), None),
    ((7, 65, 64), (1, 0, 1, 1, 0, 0, 1)),
    ((3, 97, 128), None),
    ((40, 224, 256), None),
    ((40, 460, 64), tuple(0 if i % 10 == 3 else 1 for i in range(40))),
    ((260, 33, 64), None),
    ((3, 513, 128), None),
]

# (B, P, D, H, FF, L): the dispatch of csrc/transformer.hip; see tests/test_transformer_anchored_gpu.py
TRANSFORMER_CASES = [
    (1, 1, 256, 8, 1024, 2), (2, 32, 256, 8, 1024, 2), (33, 7, 256, 8, 1024, 2), (40, 20, 256, 8, 1024, 2),
    (9, 2, 256, 8, 1024, 2),
    (3, 32, 128, 4, 512, 2),
    (3, 17, 256, 4, 1024, 2), (2, 32, 64, 1, 64, 1),
    (2, 33, 256, 8, 1024, 2), (2, 64, 256, 8, 1024, 1),
    (3, 20, 64, 8, 256, 2), (2, 64, 128, 8, 192, 2),
    (2, 5, 256, 8, 64, 1),
    (2, 5, 64, 4, 64, 16),
]

POSE_HEAD_CASES = [(rows, width) for width in (64, 256, 180, 263) for rows in (1, 35, 641)]


def pointnet_case(shape, valids=None, seed=0):
    """A PointNet (on the CPU, training mode) whose bn5.weight has negative and zero entries and whose bn4.weight has
    negative entries (the max over points then is a min / a constant of the never-stored pre-BatchNorm values), points,
    the validity vector and the weights of the scalar loss."""
    from multi_part_assembly_amd.encoder import build_encoder
    M, N, F = shape
    torch.manual_seed(1000 * M + N + F + seed)
    enc = build_encoder("pointnet", F).train()
    g = torch.Generator().manual_seed(7 * M + 3 * N + F + seed)
    with torch.no_grad():
        enc.bn5.weight[::3] *= -1.0
        enc.bn5.weight[1::7] = 0.0
        enc.bn5.bias.copy_(torch.randn(F, generator=g))
        enc.bn4.weight[::5] *= -0.5
        for i in range(1, 5):  # non-trivial affine parameters and running statistics everywhere
            bn = getattr(enc, f"bn{i}")
            bn.weight.mul_(1.0 + 0.3 * torch.rand(bn.weight.shape, generator=g))
            bn.bias.copy_(0.1 * torch.randn(bn.bias.shape, generator=g))
        for i in range(1, 6):
            bn = getattr(enc, f"bn{i}")
            bn.running_mean.copy_(0.1 * torch.randn(bn.running_mean.shape, generator=g))
            bn.running_var.copy_(0.5 + torch.rand(bn.running_var.shape, generator=g))
    pts = torch.randn(M, N, 3, generator=g) * 0.3
    v = torch.ones(M) if valids is None else torch.tensor(valids, dtype=torch.float32)
    assert v.shape == (M,)
    w = torch.randn(M, F, generator=g)
    return enc, pts, v, w


def pointnet_fn(training=True):
    """oracle.nets.pointnet on the valid parts: features and (training) the updated running statistics; loss = sum(feat w)."""
    def fn(sd, inp):
        stats = {} if training else None
        feat = on.pointnet(inp["pts"], sd, training=training, stats_out=stats)
        outs = {"feat": feat}
        if training:
            outs.update({"stat." + k: v for k, v in stats.items()})
        return outs, (feat * inp["w"]).sum()
    return fn


def transformer_case(dims, seed=0):
    """A TransformerEncoder (on the CPU) with perturbed one-dimensional parameters, tokens, the validity matrix (valid
    counts drawn per sample; the first sample has a single valid token, the last one all P) and the loss weights.  The
    samples' token scales differ (0.05, 1, 0.3, ...): LayerNorm's epsilon only shows where the variance is small."""
    from multi_part_assembly_amd.transformer import TransformerEncoder
    B, P, D, H, FF, L = dims
    torch.manual_seed(sum(dims) + seed)
    enc = TransformerEncoder(D, H, FF, L, norm_first=True, dropout=0.1).train()
    g = torch.Generator().manual_seed(B + 7 * P + D + seed)
    with torch.no_grad():
        for p in enc.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    num = torch.randint(1, P + 1, (B,), generator=g)
    num[0] = 1
    num[-1] = P
    valid = torch.arange(P)[None] < num[:, None]
    scale = torch.tensor([0.05, 1.0, 0.3])[torch.arange(B) % 3]
    tok = torch.randn(B, P, D, generator=g) * scale[:, None, None] * valid[..., None]
    w = torch.randn(B, P, D, generator=g) * valid[..., None]
    return enc, tok, valid, w


def transformer_fn(dims, dropout_p=0.0, seed=0):
    """oracle.nets.transformer_encoder with the HIP kernels' counter-based masks; loss = sum(out w), w zero on padded tokens."""
    B, P, D, H, FF, L = dims

    def fn(sd, inp):
        out = on.transformer_encoder(inp["tok"], inp["valid"], sd, "", L, H, dropout_p=dropout_p, seed=seed)
        return {"out": out}, (out * inp["w"]).sum()
    return fn


def pose_head_case(rows, width, seed=0):
    from multi_part_assembly_amd.regressor import StocasticPoseRegressor
    torch.manual_seed(rows + width + seed)
    head = StocasticPoseRegressor(feat_dim=width, noise_dim=0).train()
    g = torch.Generator().manual_seed(3 * rows + width + seed)
    with torch.no_grad():
        for p in head.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    x = torch.randn(rows, width, generator=g)
    return head, x, torch.randn(rows, 4, generator=g), torch.randn(rows, 3, generator=g)


def pose_head_fn(sd, inp):
    rot, trans = on.pose_head(inp["x"], sd, "")
    return {"rot": rot, "trans": trans}, (rot * inp["w_rot"]).sum() + (trans * inp["w_trans"]).sum()


def valid_rows(t, valid):
    """Rows of the valid tokens of a [B, P, ...] tensor."""
    return t.detach().cpu()[valid.cpu()]


# ---- the graph networks' workhorses: csrc/gru.hip and csrc/mlp.hip -------------------------------------------------------

FLIP_PREACT = 5e-6  # the constant of tests/test_callers_gpu.py (tests/test_anchored.py holds the two equal)
PIN_SHARE = 1e-3    # at most this share of a case's output entries may be taken out of the loss by the ReLU pinning

# (D, B, T, H): the smallest shapes that reach each edge of csrc/gru.hip; see tests/test_gru_anchored_gpu.py
GRU_CASES = [(2, 1, 1, 128), (1, 1, 2, 256), (1, 32, 4, 128), (2, 32, 3, 256), (2, 33, 3, 256), (2, 64, 2, 128),
             (2, 64, 5, 256), (2, 7, 33, 128)]
GRU_WRAPPER_CASES = [(33, 6, 256), (64, 4, 128)]  # (B, T, H) of the masked bidirectional wrapper

# (R, K, N, mode) of one layer of csrc/mlp.hip; see tests/test_mlp_anchored_gpu.py.  Modes: "bn" Linear + bias ->
# BatchNorm -> ReLU, "bn-norelu" the same without the ReLU; without BatchNorm "bias-relu", "bias", "nobias" (ReLU, no
# bias) and "data" (bias + ReLU, x takes no gradient).
MLP_SMALL_CASES = [(5, 64, 64, "bn"), (31, 192, 320, "bn"), (33, 384, 192, "bn"), (257, 768, 64, "bn"),
                   (2048, 1024, 128, "bn"), (257, 128, 768, "bn"), (2048, 384, 192, "bn"), (33, 128, 768, "bn"),
                   (257, 192, 320, "bn-norelu")]
MLP_BIG_CASES = [(2049, 64, 64, "bn"), (2177, 192, 320, "bn"), (2049, 320, 192, "bn"), (2177, 128, 128, "bn"),
                 (2177, 64, 64, "bn"), (2049, 128, 128, "bn"), (2177, 192, 320, "bn-norelu")]
MLP_NOBN_MODES = ("bias-relu", "bias", "nobias", "data")
MLP_NOBN_CASES = [(R, K, N, mode) for R in (1, 33, 2049) for K, N in ((256, 512), (192, 64)) for mode in MLP_NOBN_MODES]
MLP_LAYER_CASES = MLP_SMALL_CASES + MLP_BIG_CASES + MLP_NOBN_CASES

# (B, P, F, N, mode) of the pair layer; modes: "distinct" a and b, "same" one tensor in both roles, "data" b takes no gradient
PAIR_MODES = ("distinct", "same", "data")
PAIR_LAYER_CASES = [(B, P, F, N, mode) for B, P, F, N in ((1, 2, 64, 64), (3, 5, 192, 192), (2, 7, 64, 320), (2, 46, 64, 128),
                                                         (5, 13, 128, 512)) for mode in PAIR_MODES]


def case_id(case):
    return "x".join(str(c) for c in case)


def gru_case(dims, seed=0):
    """(sd, inputs) of the recurrence: gi ~ N(0,1), h0 ~ N(0,1), whh ~ N(0,1)/sqrt(H), bhh ~ 0.1 N(0,1), loss weights w."""
    D, B, T, H = dims
    g = torch.Generator().manual_seed(1000 * D + 100 * B + 10 * T + H + seed)
    sd = {"whh": torch.randn(D, 3 * H, H, generator=g) / H ** 0.5, "bhh": 0.1 * torch.randn(D, 3 * H, generator=g)}
    inputs = {"gi": torch.randn(D, B, T, 3 * H, generator=g), "h0": torch.randn(D, B, H, generator=g),
              "w": torch.randn(D, B, T, H, generator=g)}
    return sd, inputs


def gru_fn(sd, inp):
    """oracle.callers.gru_recurrent; loss = sum(h w)."""
    from oracle import callers as oc
    h = oc.gru_recurrent(inp["gi"], inp["h0"], sd["whh"], sd["bhh"])
    return {"h": h}, (h * inp["w"]).sum()


GRU_WRT = ("gi",)


def gru_wrapper_case(dims, seed=0):
    """A _MaskedBiGRU (on the CPU) over nn.GRU(H, H, bidirectional), x [B, T, H], a non-zero initial state [2, B, H], the
    validity matrix (valid lengths drawn in 1..T; the first sample has length 1, the last one T) and the loss weights."""
    from multi_part_assembly_amd.gnn import _MaskedBiGRU
    B, T, H = dims
    torch.manual_seed(B + 10 * T + H + seed)
    mod = _MaskedBiGRU(torch.nn.GRU(input_size=H, hidden_size=H, num_layers=1, batch_first=True, bidirectional=True))
    g = torch.Generator().manual_seed(7 * B + 3 * T + H + seed)
    lengths = torch.randint(1, T + 1, (B,), generator=g)
    lengths[0], lengths[-1] = 1, T
    valids = (torch.arange(T)[None] < lengths[:, None]).float()
    inputs = {"x": torch.randn(B, T, H, generator=g), "hidden": torch.randn(2, B, H, generator=g), "valids": valids,
              "w": torch.randn(B, T, 2 * H, generator=g)}
    return mod, inputs


def gru_wrapper_fn(sd, inp):
    """oracle.callers.packed_bigru (pack_padded_sequence -> GRU -> pad_packed_sequence); loss = sum(out w)."""
    from oracle import callers as oc
    out = oc.packed_bigru(inp["x"], inp["hidden"], inp["valids"], sd, "", True)
    return {"y": out}, (out * inp["w"]).sum()


def _layer_sd(K, N, bn, bias, g):
    """lin.* (+ bn.*) of one layer: gamma in 0.5..1.5 with a few negative entries and one exact zero, beta ~ 0.1 N,
    non-trivial running statistics."""
    sd = {"lin.weight": torch.randn(N, K, generator=g) / K ** 0.5}
    if bias:
        sd["lin.bias"] = 0.1 * torch.randn(N, generator=g)
    if bn:
        gamma = 0.5 + torch.rand(N, generator=g)
        gamma[::9] *= -1.0
        gamma[5] = 0.0
        sd.update({"bn.weight": gamma, "bn.bias": 0.1 * torch.randn(N, generator=g),
                   "bn.running_mean": 0.1 * torch.randn(N, generator=g), "bn.running_var": 0.5 + torch.rand(N, generator=g)})
    return sd


def _pin_relu(fn, sd, inputs):
    """The ReLU pinning of a single layer: evaluate `fn` in float64, find the output entries whose pre-activation lies
    within FLIP_PREACT of zero relative to its channel's largest |pre-activation| — a float32-grade evaluation may land
    on the other side of the ReLU there — and zero the loss weight `w` at them (in place).  Their gradient contribution
    is then zero on either side of the flip and their output within any bar of zero.  Returns their share."""
    cast = lambda v: v.double() if torch.is_tensor(v) and v.is_floating_point() else v
    with torch.no_grad():
        outs, _ = fn({k: cast(v) for k, v in sd.items()}, {k: cast(v) for k, v in inputs.items()})
    pre = outs["pre"]
    near = pre.abs() < FLIP_PREACT * pre.abs().amax(dim=0, keepdim=True)
    inputs["w"][near] = 0.0
    return float(near.double().mean())


def mlp_layer_case(case, seed=0):
    """(sd, inputs, wrt, share) of one MLP-layer case: x ~ N(0,1) [R, K], weight ~ N(0,1)/sqrt(K), bias ~ 0.1 N, the
    BatchNorm parameters of `_layer_sd`, the loss weights w [R, N] with the ReLU pinning applied (share: the entries it
    zeroed; 0 without a ReLU)."""
    R, K, N, mode = case
    modes = ("bn", "bn-norelu") + MLP_NOBN_MODES
    g = torch.Generator().manual_seed(100000 * modes.index(mode) + 1000 * R + 10 * K + N + seed)
    sd = _layer_sd(K, N, mode.startswith("bn"), mode != "nobias", g)
    inputs = {"x": torch.randn(R, K, generator=g), "w": torch.randn(R, N, generator=g)}
    relu = mode in ("bn", "bias-relu", "nobias", "data")
    share = _pin_relu(mlp_layer_fn(case, preact=True), sd, inputs) if relu else 0.0
    return sd, inputs, (() if mode == "data" else ("x",)), share


def mlp_layer_fn(case, training=True, preact=False):
    """oracle.callers.mlp_layer: the output and (training-mode BatchNorm) the updated running statistics; loss = sum(y w).
    `preact`: also the value in front of the ReLU (as `pre`; for `_pin_relu`, not a compared tensor)."""
    R, K, N, mode = case
    bn, relu = mode.startswith("bn"), mode in ("bn", "bias-relu", "nobias", "data")

    def fn(sd, inp):
        from oracle import callers as oc
        stats = {} if bn and training else None
        y, pre = oc.mlp_layer(inp["x"], sd, "", bn, relu, training, stats, return_preact=True)
        outs = {"y": y}
        if stats:
            outs.update({"stat." + k: v for k, v in stats.items()})
        if preact:
            outs["pre"] = pre
        return outs, (y * inp["w"]).sum()
    return fn


def pair_layer_case(case, seed=0):
    """(sd, inputs, wrt, share) of one pair-layer case: a, b ~ N(0,1) [B, P, F] ("same": a alone, in both roles), the
    layer's parameters over the 2F-wide pair rows, the loss weights w [B P P, N] with the ReLU pinning applied."""
    B, P, F, N, mode = case
    g = torch.Generator().manual_seed(100000 * PAIR_MODES.index(mode) + 1000 * B + 100 * P + 10 * F + N + seed)
    sd = _layer_sd(2 * F, N, True, True, g)
    inputs = {"a": torch.randn(B, P, F, generator=g), "w": torch.randn(B * P * P, N, generator=g)}
    if mode != "same":
        inputs["b"] = torch.randn(B, P, F, generator=g)
    share = _pin_relu(pair_layer_fn(case, preact=True), sd, inputs)
    return sd, inputs, (("a", "b") if mode == "distinct" else ("a",)), share


def pair_layer_fn(case, preact=False):
    """oracle.callers.mlp_layer over the materialised pair rows cat([a_i ; b_j]) (oracle.callers.pair_rows)."""
    def fn(sd, inp):
        from oracle import callers as oc
        stats = {}
        rows = oc.pair_rows(inp["a"], inp.get("b", inp["a"]))
        y, pre = oc.mlp_layer(rows, sd, "", True, True, True, stats, return_preact=True)
        outs = {"y": y, **{"stat." + k: v for k, v in stats.items()}}
        if preact:
            outs["pre"] = pre
        return outs, (y * inp["w"]).sum()
    return fn
