"""`DeviceGeometryProducer.batch` with a device index vector: the slot table built by `mpa_mesh_slot_table`
(csrc/mesh_sample.hip) gives the bits of the host-index path for the same (seed, batch_counter, indices); bad indices are
reported through the status word without being dereferenced."""
import numpy as np
import pytest
import torch

from multi_part_assembly_amd import synthetic
from multi_part_assembly_amd.datasets import DeviceGeometryProducer, MeshStore

pytestmark = pytest.mark.gpu

B, P, N = 3, 4, 64
COUNTS = [2, 4, 3, 2, 4, 3, 4]


@pytest.fixture(scope="module")
def store():
    return MeshStore.from_arrays(synthetic.make_fracture_meshes(11, len(COUNTS), COUNTS, 24), 2, P)


def producer(store, dev, **kw):
    return DeviceGeometryProducer(store, num_points=N, min_num_part=2, max_num_part=P, seed=(5 << 32) | 77,
                                  data_keys=("part_ids", "valid_matrix"), device=dev, **kw)


def assert_same(got, want, rows=None):
    assert list(got) == list(want)
    for key in want:
        if key == "data_id":
            continue
        g, w = got[key], want[key]
        assert g.dtype == w.dtype and g.shape == w.shape and g.device == w.device, key
        if rows is not None and g.numel():
            g, w = g[rows], w[rows]
        assert torch.equal(g, w), key


@pytest.mark.parametrize("indices,counter", [([0, 1, 2], 0), ([6, 3, 1], 5), ([4, 4, 0], (1 << 40) + 3)])
def test_device_indices_give_the_bits_of_host_indices(cuda_device, store, indices, counter):
    prod = producer(store, cuda_device)
    want, want_raw = prod.batch(indices, batch_counter=counter, return_raw=True)
    d_idx = torch.tensor(indices, dtype=torch.int64, device=cuda_device)
    got, got_raw = prod.batch(d_idx, batch_counter=counter, return_raw=True)
    assert_same(got, want)
    assert torch.equal(got_raw, want_raw)
    assert got["data_id"] is d_idx and want["data_id"].tolist() == indices
    assert got["part_valids"].sum().item() == sum(COUNTS[i] for i in indices)
    prod.check()


def test_default_counter_advances_like_the_host_path(cuda_device, store):
    a, b = producer(store, cuda_device), producer(store, cuda_device)
    d_idx = torch.tensor([2, 5, 6], dtype=torch.int64, device=cuda_device)
    for _ in range(3):
        assert_same(a.batch(d_idx), b.batch([2, 5, 6]))
    assert a.batch_counter == b.batch_counter == 3


@pytest.mark.parametrize("bad", [len(COUNTS), -1])
def test_bad_index_sets_the_status_and_reads_nothing(cuda_device, store, bad):
    prod = producer(store, cuda_device)
    clean = prod.batch(torch.tensor([3, 0, 5], dtype=torch.int64, device=cuda_device), batch_counter=2)
    prod.check()
    got = prod.batch(torch.tensor([3, bad, 5], dtype=torch.int64, device=cuda_device), batch_counter=2)
    with pytest.raises(RuntimeError, match="outside the store"):
        prod.check()
    prod.check()  # reported once, the word is clear again
    assert got["part_valids"][1].sum().item() == 0 and got["part_ids"][1].abs().sum().item() == 0
    assert got["part_pcs"][1].abs().sum().item() == 0 and got["part_trans"][1].abs().sum().item() == 0
    assert_same(got, clean, rows=[0, 2])  # the other shapes: the streams depend on the slot, not on the neighbours


def test_part_count_outside_the_limits_is_reported(cuda_device, store):
    prod = DeviceGeometryProducer(store, num_points=N, min_num_part=3, max_num_part=P, device=cuda_device)
    got = prod.batch(torch.tensor([1, 0, 2], dtype=torch.int64, device=cuda_device), batch_counter=0)  # shape 0: 2 parts
    with pytest.raises(RuntimeError, match="part count"):
        prod.check()
    assert got["part_valids"].sum(1).tolist() == [4.0, 0.0, 3.0]
    with pytest.raises(ValueError, match="part count"):
        prod.batch([1, 0, 2])  # the host path refuses the same batch up front


def test_what_the_device_path_refuses(cuda_device, store):
    d_idx = torch.tensor([0, 1, 2], dtype=torch.int64, device=cuda_device)
    with pytest.raises(ValueError, match="shuffle_parts"):
        producer(store, cuda_device, shuffle_parts=True).batch(d_idx)
    prod = producer(store, cuda_device)
    with pytest.raises(ValueError, match="contiguous int64"):
        prod.batch(d_idx.int())
    with pytest.raises(ValueError, match="contiguous int64"):
        prod.batch(torch.arange(6, device=cuda_device)[::2])
    with pytest.raises(ValueError, match="contiguous int64"):
        prod.batch(d_idx.view(3, 1))
    assert np.array_equal(store.device_shape_part_off(cuda_device).cpu().numpy(), store.shape_part_off)
    assert store.device_shape_part_off(cuda_device) is store.device_shape_part_off(cuda_device)  # uploaded once
