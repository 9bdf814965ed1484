"""`mpa_epoch_order` (csrc/epoch_order.hip) on the device against its numpy restatement
(multi_part_assembly_amd/sampler_ref.py, checked on its own in tests/test_epoch_sampler.py), bit for bit: the sizes around
the kernel's block (256 threads) and key tile (1024 keys), every rank of small worlds, epochs with a high word, seeds with
a high word; the epoch read from a device word, eagerly and under a captured launch; and `EpochSampler` on top."""
import numpy as np
import pytest
import torch

from multi_part_assembly_amd import _lib, sampler_ref
from multi_part_assembly_amd.sampler import EpochSampler

pytestmark = pytest.mark.gpu

SENTINEL = -7
SEEDS = (3, (0x9E3779B9 << 32) | 12345)
EPOCHS = (0, 1, (1 << 32) + 5)


def run(dev, S, world=1, rank=0, seed=0, epoch=0, epoch_dev=None, extra=5, workspace=None, out=None):
    """One call into a sentinel-filled buffer `extra` entries longer than the shard; returns the whole buffer."""
    shard = -(-S // world)
    if out is None:
        out = torch.full((shard + extra,), SENTINEL, dtype=torch.int64, device=dev)
    if workspace is None:
        workspace = torch.empty(_lib.query("mpa_epoch_order_workspace", S) // 8, dtype=torch.int64, device=dev)
    _lib.launch("mpa_epoch_order", dev, S, world, rank, seed, epoch, epoch_dev, workspace, out)
    return out


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025, 2049, 4097])
def test_order_equals_the_restatement(cuda_device, S):
    for seed in SEEDS:
        for epoch in EPOCHS:
            perm = sampler_ref.epoch_permutation(S, seed, epoch)
            for world in (1, 2, 3):
                shard = -(-S // world)
                for rank in range(world):
                    got = run(cuda_device, S, world, rank, seed, epoch).cpu().numpy()
                    want = sampler_ref.shard(perm, world, rank)
                    assert np.array_equal(got[:shard], want), (S, seed, epoch, world, rank)
                    assert (got[shard:] == SENTINEL).all()  # exactly total / world entries are written


def test_two_runs_are_bit_identical(cuda_device):
    a = run(cuda_device, 4097, 3, 1, SEEDS[1], 9)
    b = run(cuda_device, 4097, 3, 1, SEEDS[1], 9)
    assert torch.equal(a, b) and not torch.equal(a, run(cuda_device, 4097, 3, 1, SEEDS[1], 10))


def test_epoch_from_a_device_word_equals_the_epoch_by_value(cuda_device):
    for epoch in EPOCHS:
        word = torch.tensor([epoch], dtype=torch.int64, device=cuda_device)
        got = run(cuda_device, 1000, 2, 1, SEEDS[0], epoch=123456, epoch_dev=word)  # the value is ignored beside the word
        assert torch.equal(got, run(cuda_device, 1000, 2, 1, SEEDS[0], epoch))


def test_captured_launch_draws_the_next_epoch_after_the_word_is_rewritten(cuda_device):
    S, world, rank, seed = 1000, 2, 0, SEEDS[1]
    word = torch.tensor([4], dtype=torch.int64, device=cuda_device)
    out = torch.full((S // world + 5,), SENTINEL, dtype=torch.int64, device=cuda_device)
    ws = torch.empty(S, dtype=torch.int64, device=cuda_device)
    run(cuda_device, S, world, rank, seed, epoch_dev=word, workspace=ws, out=out)  # (loads the code object before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        run(cuda_device, S, world, rank, seed, epoch_dev=word, workspace=ws, out=out)
    for epoch in (4, 5, (1 << 32) + 5):
        word.fill_(epoch)
        out.fill_(SENTINEL)
        graph.replay()
        got = out.cpu().numpy()
        assert np.array_equal(got[:S // world], sampler_ref.epoch_order(S, seed, epoch, world, rank)), epoch
        assert (got[S // world:] == SENTINEL).all()


def test_more_ranks_than_shapes_wrap_around_more_than_once(cuda_device):
    for rank in range(5):
        got = run(cuda_device, 2, 5, rank, 1, 0).cpu().numpy()
        assert np.array_equal(got[:1], sampler_ref.epoch_order(2, 1, 0, 5, rank)) and (got[1:] == SENTINEL).all()


def test_sampler_yields_device_views_of_the_documented_order(cuda_device):
    s = EpochSampler(1000, 32, seed=SEEDS[1], world=3, rank=2, device=cuda_device)
    assert len(s) == 334 // 32
    for epoch in (0, 7):
        s.set_epoch(epoch)
        batches = list(s)
        assert len(batches) == len(s) and all(b.is_cuda and b.dtype == torch.int64 and b.is_contiguous() for b in batches)
        assert batches[1].data_ptr() == s.order.data_ptr() + 32 * 8  # views into the epoch's vector
        want = sampler_ref.epoch_order(1000, SEEDS[1], epoch, 3, 2)
        assert np.array_equal(torch.cat(batches).cpu().numpy(), want[:32 * len(s)])
    plain = EpochSampler(10, 4, world=3, rank=1, shuffle=False, drop_last=False, device=cuda_device)
    plain.set_epoch(0)
    assert [b.tolist() for b in plain] == [[1, 4, 7, 0]]
    # mid-epoch state on the device sampler
    s.set_epoch(3)
    it = iter(s)
    next(it), next(it)
    t = EpochSampler(1000, 32, seed=0, world=3, rank=2, device=cuda_device)
    t.load_state_dict(s.state_dict())
    assert torch.equal(next(iter(t)), s.batch_indices(2))
