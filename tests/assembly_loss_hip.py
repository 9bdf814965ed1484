"""The driver of the code under test for tests/test_loss_anchored_gpu.py and the `lossgrad` family of tools/fuzz_parity.py:
forward and backward of the fused assembly loss through the C ABI (a plain module; the yardstick, tests/assembly_loss_ref.py,
does not import the library's loader)."""
import torch


def hip_run(batch, go, rot_type, training=True, search="grid", device=None):
    """mpa_assembly_loss_forward[_rmat]_ordered and mpa_assembly_loss_backward[_rmat] on the same, poisoned workspaces
    (NaN floats, 0x7F7F7F7F ints).  Returns CPU tensors: losses [5, B], grad_rot, grad_trans, the four arg-min arrays from
    the head of the int workspace and the four posed clouds [4, B, P, N, 3] from the head of the float workspace."""
    from multi_part_assembly_amd import _lib
    from multi_part_assembly_amd.loss import SEARCH_MODES
    dev = torch.device("cuda:0") if device is None else device
    d = lambda k: batch[k].detach().to(dev, torch.float32).contiguous()
    pcs, v, rp, tp, rg, tg = (d(k) for k in ("pcs", "valids", "rot_pred", "trans_pred", "rot_gt", "trans_gt"))
    B, P, N, _ = pcs.shape
    assert rp.shape[2:] == ((3, 3) if rot_type == "rmat" else (4,)) and rg.shape == rp.shape
    lib, p, sfx = _lib.lib(), _lib.ptr, ("_rmat" if rot_type == "rmat" else "")
    nf, ni = _lib.query("mpa_assembly_loss_workspace", B, P, N)
    fws = torch.full((nf,), float("nan"), device=dev)
    iws = torch.full((ni,), 0x7F7F7F7F, dtype=torch.int32, device=dev)
    losses = torch.full((5, B), float("nan"), device=dev)
    gq, gt = torch.full_like(rp, float("nan")), torch.full_like(tp, float("nan"))
    gol = go.detach().to(dev, torch.float32).contiguous()
    with torch.cuda.device(dev):
        stream = _lib.current_stream(dev)
        fwd = getattr(lib, f"mpa_assembly_loss_forward{sfx}_ordered")
        _lib.check(fwd(p(pcs), p(v), p(rp), p(tp), p(rg), p(tg), B, P, N, int(training), 0, None, SEARCH_MODES[search],
                       p(fws), p(iws), p(losses), None, stream), "assembly_loss_forward")
        torch.cuda.synchronize(dev)
        pn = B * P * N
        idx = tuple(iws[k * pn:(k + 1) * pn].view(B, P, N).cpu() for k in range(4))
        clouds = fws[:12 * pn].view(4, B, P, N, 3).cpu()
        bwd = getattr(lib, f"mpa_assembly_loss_backward{sfx}")
        _lib.check(bwd(p(gol), p(pcs), p(v), p(rp), p(tp), p(rg), p(tg), B, P, N, int(training), p(fws), p(iws), p(gq),
                       p(gt), stream), "assembly_loss_backward")
        torch.cuda.synchronize(dev)
    return {"losses": losses.cpu(), "grad_rot": gq.cpu(), "grad_trans": gt.cpu(), "idx": idx, "clouds": clouds}
