"""The part transformer and the pose head on csrc/transformer.hip against oracle.nets.transformer_encoder / pose_head
evaluated in FLOAT64, under the bars of tests/anchored.py: output on the valid tokens, token gradient, every parameter
gradient — at dropout 0 and at dropout 0.1 with the oracle regenerating the kernels' counter-based masks (on the scalar
attention path the mask is indexed by element of the probability tensor: that the oracle's masks line up there too is one
of the things these cases establish).

The transformer cases follow the dispatch of mpa_transformer_forward / mpa_transformer_backward, (B, P, D, H, FF, L):

  (1,1,256,8,1024,2) (2,32,256,8,1024,2) (33,7,256,8,1024,2) (40,20,256,8,1024,2)
                         fused LayerNorm + qkv + attention forward, fused d o / attention backward
  (9,2,256,8,1024,2)     more samples than LayerNorm-backward blocks: the fused backward is refused, the forward stays fused
  (3,32,128,4,512,2)     attn_fwd_mfma_kernel<1> without the LayerNorm fusion (D != 256)
  (3,17,256,4,1024,2) (2,32,64,1,64,1)
                         attn_fwd_mfma_kernel<2> (head dim 64)
  (2,33,256,8,1024,2) (2,64,256,8,1024,1)
                         the scalar attention kernels (P > 32), more than one 32-row tile per sample, LayerNorm fusion on
  (3,20,64,8,256,2) (2,64,128,8,192,2)
                         the scalar attention kernels at head dim 8 and 16, FF != 4 D
  (2,5,256,8,64,1)       FF = 64, below D
  (2,5,64,4,64,16)       16 layers, the envelope's maximum

Valid counts are drawn per sample; the first sample has a single valid token, the last one all P."""
import pytest
import torch

import anchored as A
from multi_part_assembly_amd.transformer import _TransformerFn

pytestmark = pytest.mark.gpu

SEED = 0xA5EED0123457


@pytest.mark.parametrize("p_drop", [0.0, 0.1], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("dims", A.TRANSFORMER_CASES, ids=["x".join(map(str, d)) for d in A.TRANSFORMER_CASES])
def test_transformer_against_the_float64_oracle(cuda_device, capsys, dims, p_drop):
    B, P, D, H, FF, L = dims
    enc, tok0, valid, w = A.transformer_case(dims)
    sd0 = {k: t.detach().clone() for k, t in enc.state_dict().items()}
    fn = A.transformer_fn(dims, p_drop, SEED)
    r32, r64 = A.oracle_pair(fn, sd0, {"tok": tok0, "valid": valid, "w": w}, ("tok",))
    if p_drop > 0.0:  # the masks bite
        clean = A.oracle_run(A.transformer_fn(dims), sd0, {"tok": tok0, "valid": valid, "w": w}, ("tok",))
        assert A.err(clean["out.out"][valid], r64["out.out"][valid]) > 1e-3
    for r in (r32, r64):  # padded tokens carry no output and no gradient that anything reads
        r["out.out"], r["gin.tok"] = r["out.out"][valid], r["gin.tok"][valid]

    assert enc.native
    enc.to(cuda_device).train()
    tok = tok0.to(cuda_device).requires_grad_()
    out = _TransformerFn.apply(tok, valid.reshape(-1).float().to(cuda_device), H, p_drop, SEED, None, *enc._params())
    (out * w.to(cuda_device)).sum().backward()
    torch.cuda.synchronize()
    got = {"out.out": A.valid_rows(out, valid), "gin.tok": A.valid_rows(tok.grad, valid)}
    got.update({"grad." + k: p.grad.detach().cpu() for k, p in enc.named_parameters()})
    assert set(got) == set(r64), sorted(set(got) ^ set(r64))
    A.assert_anchored(got, r32, r64, f"transformer {dims}, dropout {p_drop:g}, {int(valid.sum())} valid tokens", capsys)


@pytest.mark.parametrize("rows,width", A.POSE_HEAD_CASES, ids=["%dx%d" % c for c in A.POSE_HEAD_CASES])
def test_pose_head_against_the_float64_oracle(cuda_device, capsys, rows, width):
    """StocasticPoseRegressor(noise_dim=0) on the HIP head: input widths that are and are not multiples of the 64-column
    GEMM panels, one row, a ragged tile, many tiles — rot, trans, input gradient and parameter gradients."""
    head, x0, w_r, w_t = A.pose_head_case(rows, width)
    sd0 = {k: t.detach().clone() for k, t in head.state_dict().items()}
    r32, r64 = A.oracle_pair(A.pose_head_fn, sd0, {"x": x0, "w_rot": w_r, "w_trans": w_t}, ("x",))
    assert head.native
    head.to(cuda_device).train()
    x = x0.to(cuda_device).requires_grad_()
    rot, trans = head(x)
    ((rot * w_r.to(cuda_device)).sum() + (trans * w_t.to(cuda_device)).sum()).backward()
    torch.cuda.synchronize()
    got = {"out.rot": rot.detach().cpu(), "out.trans": trans.detach().cpu(), "gin.x": x.grad.cpu()}
    got.update({"grad." + k: p.grad.detach().cpu() for k, p in head.named_parameters()})
    assert set(got) == set(r64), sorted(set(got) ^ set(r64))
    A.assert_anchored(got, r32, r64, f"pose head {rows} rows x {width}", capsys)
