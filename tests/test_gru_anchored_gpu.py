"""The GRU recurrence of csrc/gru.hip (all steps of both directions in one launch each way, the blocks of a direction
handing each other the hidden state as tagged words) against oracle.callers.gru_recurrent — a plain loop over t —
evaluated in FLOAT64 on the CPU, under the bars of tests/anchored.py: the hidden states of every step and the gradients of
the input projections, W_hh and b_hh, with a non-zero initial state; two runs bit-equal.  And the masked bidirectional
wrapper of RGL-NET (gnn._MaskedBiGRU: input projections, reversed valid prefixes, zeros on padded steps) against
oracle.callers.packed_bigru — pack_padded_sequence -> GRU -> pad_packed_sequence — the same way, every parameter
gradient included.

The shapes (D, B, T, H) are the smallest that reach each edge of the kernels.  A block owns 8 hidden units; its 256 threads
take the (sample, unit) pairs e = thread, thread + 256 (the forward's loop is unrolled twice, the backward's loops step
by 256), and the forward reads the other blocks' hidden state 8192 words per trip:

  (2, 1, 1, 128)   one sample, one step: no exchange at all; 8 working threads per block
  (1, 1, 2, 256)   one direction; each step parity of the exchange used once
  (1, 32, 4, 128)  B * 8 = 256: the last batch size with one trip of the gate loops
  (2, 32, 3, 256)  B * H = 8192: exactly one trip of the exchange read
  (2, 33, 3, 256)  the second trip of the gate loops (8 pairs) and of the exchange read (256 words), of the backward's
                   loops too — one of them polls the other blocks' partial sums
  (2, 64, 2, 128)  the batch limit at H = 128: B * H = 8192, the exact fit of one exchange trip, two full gate trips
  (2, 64, 5, 256)  the batch limit at H = 256: two full trips of everything, both parities used more than once
  (2, 7, 33, 128)  many steps, an odd batch; H = 128: two row groups per column in the backward
"""
import pytest
import torch

import anchored as A

pytestmark = pytest.mark.gpu


def _recurrence(dev, sd, inputs):
    """One forward + backward of gru.gru_recurrent; (results, data pointer of the launch's workspace)."""
    from multi_part_assembly_amd import gru as G
    gi = inputs["gi"].to(dev).requires_grad_()
    whh, bhh = sd["whh"].to(dev).requires_grad_(), sd["bhh"].to(dev).requires_grad_()
    out = G.gru_recurrent(gi, inputs["h0"].to(dev), whh, bhh)
    G.raise_if_failed(dev, synchronize=True)
    ws = out.grad_fn.saved_tensors[3].data_ptr()
    grads = torch.autograd.grad((out * inputs["w"].to(dev)).sum(), [gi, whh, bhh])
    G.raise_if_failed(dev, synchronize=True)
    res = {"out.h": out, "gin.gi": grads[0], "grad.whh": grads[1], "grad.bhh": grads[2]}
    return {k: v.detach().cpu() for k, v in res.items()}, ws


@pytest.mark.parametrize("dims", A.GRU_CASES, ids=A.case_id)
def test_gru_recurrence_against_the_float64_oracle(cuda_device, capsys, dims):
    from multi_part_assembly_amd import gru as G
    D, B, T, H = dims
    if not G.supported(H, B, D):
        pytest.skip("device cannot hold the GRU grid")
    sd, inputs = A.gru_case(dims)
    r32, r64 = A.oracle_pair(A.gru_fn, sd, inputs, A.GRU_WRT)
    first, ws = _recurrence(cuda_device, sd, inputs)
    assert set(first) == set(r64), sorted(set(first) ^ set(r64))
    A.assert_anchored(first, r32, r64, f"GRU recurrence {dims}", capsys)
    # the same bits again, and again on a workspace that an earlier launch has used (its exchange words carry that launch's
    # tags: the clear in front of every launch is load-bearing)
    seen, reused = {ws}, False
    for _ in range(4):
        again, ws = _recurrence(cuda_device, sd, inputs)
        A.assert_bit_equal(first, again)
        reused = reused or ws in seen
        seen.add(ws)
        if reused:
            break
    assert reused, "no launch ran on a workspace that an earlier one had used"


def test_gru_recurrent_refuses_an_initial_state_that_needs_a_gradient(cuda_device):
    from multi_part_assembly_amd import gru as G
    sd, inputs = A.gru_case((1, 1, 2, 256))
    h0 = inputs["h0"].to(cuda_device).requires_grad_()
    with pytest.raises(RuntimeError, match="initial state"):
        G.gru_recurrent(inputs["gi"].to(cuda_device), h0, sd["whh"].to(cuda_device), sd["bhh"].to(cuda_device))
    G.gru_recurrent(inputs["gi"].to(cuda_device), h0.detach(), sd["whh"].to(cuda_device), sd["bhh"].to(cuda_device))
    G.raise_if_failed(cuda_device, synchronize=True)


@pytest.mark.parametrize("dims", A.GRU_WRAPPER_CASES, ids=A.case_id)
def test_masked_bigru_against_the_float64_packed_gru(cuda_device, capsys, dims):
    import multi_part_assembly_amd.gnn as gnn
    from multi_part_assembly_amd import gru as G
    B, T, H = dims
    if not G.supported(H, B, 2):
        pytest.skip("device cannot hold the GRU grid")
    mod, inputs = A.gru_wrapper_case(dims)
    lengths = inputs["valids"].sum(dim=1)
    assert int(lengths.min()) == 1 and int(lengths.max()) == T and int(lengths[0]) == 1 and int(lengths[-1]) == T
    sd = {k: t.detach().clone() for k, t in mod.state_dict().items()}
    r32, r64 = A.oracle_pair(A.gru_wrapper_fn, sd, inputs, ("x",))

    mod.to(cuda_device).train()
    calls = []
    keep = gnn.gru_recurrent
    gnn.gru_recurrent = lambda *a: calls.append(1) or keep(*a)  # the wrapper must take csrc/gru.hip, not the library GRU
    try:
        x = inputs["x"].to(cuda_device).requires_grad_()
        out, _ = mod(x, inputs["hidden"].to(cuda_device), valids=inputs["valids"].to(cuda_device))
    finally:
        gnn.gru_recurrent = keep
    assert calls == [1]
    G.raise_if_failed(cuda_device, synchronize=True)
    (out * inputs["w"].to(cuda_device)).sum().backward()
    G.raise_if_failed(cuda_device, synchronize=True)
    got = {"out.y": out.detach().cpu(), "gin.x": x.grad.cpu()}
    got.update({"grad." + k: p.grad.cpu() for k, p in mod.named_parameters()})
    assert set(got) == set(r64) and len(got) == 10, sorted(set(got) ^ set(r64))
    pad = inputs["valids"] == 0
    assert float(got["out.y"][pad].abs().max()) == 0.0 and float(got["gin.x"][pad].abs().max()) == 0.0  # padded steps: exactly zero
    A.assert_anchored(got, r32, r64, f"masked bidirectional GRU {dims}", capsys)
