"""The reference's DGCNN (multi_part_assembly/models/modules/encoder/dgcnn.py:8-109) restated with torch ops on
materialised edge tensors, with the kNN graphs GIVEN and the maxima optionally PINNED (a plain module, imported like
tests/eval_ref.py; checked on the CPU by tests/test_dgcnn_ref.py).

The encoder takes a max over the 20 neighbours at every (point, channel) of four stages and one over the N points at
every (part, channel) of the tail.  Two float32-grade evaluations in different summation orders may resolve a near-tie
differently, and one flipped site moves a whole weight-gradient row: a comparison of gradients means something only
once the selections are held fixed.  With `selection` every max becomes a gather at the given site, so the value and the
gradient follow that site whatever the arithmetic's rounding says; whether the given sites ARE maxima is a separate
question, answered on the float64 values by `selection_regret`.

Evaluated in the dtype of its inputs; parameters under the reference's state_dict keys (convK.0.weight, bnK.*, out_fc.*).
"""
import torch
import torch.nn.functional as F

K = 20
WIDTHS = (64, 64, 128, 256)
BN_EPS, BN_MOMENTUM, SLOPE = 1e-5, 0.1, 0.2


def _bn(e, sd, name, training, stats_out):
    """BatchNorm over every axis but the last (channels).  Training: batch statistics (biased variance), and the running
    statistics after the update (momentum 0.1, unbiased variance) go to `stats_out`."""
    rm, rv = sd[name + ".running_mean"], sd[name + ".running_var"]
    if training:
        flat = e.reshape(-1, e.shape[-1])
        mean = flat.mean(dim=0)
        var = ((flat - mean) ** 2).mean(dim=0)
        if stats_out is not None:
            cnt = flat.shape[0]
            with torch.no_grad():
                stats_out[name + ".running_mean"] = (1 - BN_MOMENTUM) * rm + BN_MOMENTUM * mean
                stats_out[name + ".running_var"] = (1 - BN_MOMENTUM) * rv + BN_MOMENTUM * var * (cnt / max(cnt - 1, 1))
    else:
        mean, var = rm, rv
    return (e - mean) / torch.sqrt(var + BN_EPS) * sd[name + ".weight"] + sd[name + ".bias"]


def _act(y, branch):
    """LeakyReLU(0.2); with `branch` (1 = unit slope) the slope is GIVEN instead of read off the sign of y."""
    return F.leaky_relu(y, SLOPE) if branch is None else torch.where(branch.bool(), y, SLOPE * y)


def dgcnn_ref(x, sd, graphs, selection=None, training=True, stats_out=None, branch=None):
    """x [n, N, 3]; graphs: 4 x [n, N, 20] indices inside each cloud; selection: None, or 4 x [n, N, CO] neighbour SLOTS
    (0..19) and one [n, F] point index of the tail's max-pooling; branch: None, or the LeakyReLU slopes of the activations
    a gradient passes through (1 = unit slope): 4 x [n, N, CO] for the stages' selected values, [n, N, F] for the tail.
    Returns (features [n, F], z): z[0..3] the post-activation edge values [n, N, 20, CO] of the stages, z[4] the tail's
    post-activation rows [n, N, F] (always the true LeakyReLU: these are what a selection is judged on).
    BatchNorm statistics are over all 20 edges whatever is selected.  Without a selection the maxima are torch's `max`,
    taken as a gather at its own index (the site its gradient goes to), so that both modes run the same operators.

    The slope is the encoder's third discrete choice: a pre-activation within rounding of zero takes the slope 1 in one
    float32-grade evaluation and 0.2 in another, the VALUE moves by nothing and the gradient of that row by a factor of
    five — with R rows that is 1 / R of a whole gradient tensor, above 1e-4 up to R = 8000, and among some millions of
    activations a few always sit that close to zero."""
    n, N, _ = x.shape
    h, stages, z = x, [], []
    base = (torch.arange(n) * N).view(n, 1, 1)
    for l in range(4):
        C = h.shape[-1]
        flat = (graphs[l].long() + base).reshape(-1)
        nbr = h.reshape(n * N, C).index_select(0, flat).view(n, N, K, C)     # dgcnn.py:26-33 (a serial, repeatable backward)
        ctr = h.view(n, N, 1, C).expand(n, N, K, C)
        edge = torch.cat((nbr - ctr, ctr), dim=3)                            # [x_j - x_i ; x_i]
        e = edge @ sd[f"conv{l + 1}.0.weight"].reshape(WIDTHS[l], 2 * C).t()    # the 1 x 1 convolution
        y = _bn(e, sd, f"bn{l + 1}", training, stats_out)
        a = F.leaky_relu(y.detach(), SLOPE)
        z.append(a)
        at = a.max(dim=2)[1] if selection is None else selection[l].long()
        # (LeakyReLU is increasing: the activation of the selected value is the selected activation)
        h = _act(y.gather(2, at.view(n, N, 1, WIDTHS[l])).squeeze(2), None if branch is None else branch[l])
        stages.append(h)
    y = _bn(torch.cat(stages, dim=2) @ sd["conv5.0.weight"].reshape(-1, sum(WIDTHS)).t(), sd, "bn5", training, stats_out)
    z.append(F.leaky_relu(y.detach(), SLOPE))
    a = _act(y, None if branch is None else branch[4])
    at = z[4].max(dim=1)[1] if selection is None else selection[4].long()
    top = a.gather(1, at.view(n, 1, -1)).squeeze(1)
    pooled = torch.cat((top, a.mean(dim=1)), dim=1)
    return pooled @ sd["out_fc.weight"].t() + sd["out_fc.bias"], z


def argmax_selection(z):
    """The selection `dgcnn_ref(..., selection=None)` itself took (torch's max: the index its gradient goes to)."""
    return [t.max(dim=2)[1] for t in z[:4]] + [z[4].max(dim=1)[1]]


def own_branch(z, selection):
    """The slopes `dgcnn_ref(..., branch=None)` itself took at the activations a gradient passes through."""
    return [t.gather(2, s.long().unsqueeze(2)).squeeze(2) > 0 for t, s in zip(z[:4], selection[:4])] + [z[4] > 0]


def selection_regret(z, selection):
    """Per stage (0..3) and for the tail (4): (regret [channels], scale [channels], sites that differ from the arg-max).
    regret = the largest `max_t z - z[selected]` over the sites of a channel, scale = max|z| of the channel: a selection
    is as good as the maximum where regret <= tol * scale."""
    out = []
    for l, t in enumerate(z):
        dim = 2 if l < 4 else 1
        sel = selection[l].long()
        got = t.gather(dim, sel.unsqueeze(dim)).squeeze(dim)
        top, at = t.max(dim=dim)
        C = t.shape[-1]
        regret = (top - got).reshape(-1, C).max(dim=0)[0]
        scale = t.abs().reshape(-1, C).max(dim=0)[0]
        out.append((regret, scale, int((at != sel).sum())))
    return out


# ---- graphs with a known in-degree (imported through graph_hooks["graphs"]) ---------------------------------------------

def hub_ring_graph(N, hub, listers):
    """[N, 20] int64: point i lists the ring i, i + 1, ... (mod N, the hub skipped) and, if i < listers, the hub at slot
    i % 20 — 20 distinct indices per list, in-degree of the hub exactly `listers`, of every other point 19 to 21."""
    rows = []
    for i in range(N):
        want = K - 1 if i < listers else K
        ring, j = [], i
        while len(ring) < want:
            if j % N != hub:
                ring.append(j % N)
            j += 1
        if i < listers:
            ring.insert(i % K, hub)
        rows.append(ring)
    return torch.tensor(rows, dtype=torch.int64)


def constant_graph(N):
    """[N, 20]: every list = 0..19 (what a part of coinciding points resolves to): twenty points of in-degree N."""
    return torch.arange(K, dtype=torch.int64).repeat(N, 1)


def in_degrees(graph, N):
    """graph [n, N, 20] -> [n, N] in-degrees; asserts that every list holds 20 distinct indices below N."""
    import numpy as np
    g = graph.cpu().numpy().astype(np.int64)
    assert g.ndim == 3 and g.shape[1:] == (N, K), g.shape
    assert g.min() >= 0 and g.max() < N
    s = np.sort(g, axis=2)
    assert (s[..., 1:] != s[..., :-1]).all(), "a neighbour list repeats an index"
    return np.stack([np.bincount(p.reshape(-1), minlength=N) for p in g])
