"""PartNet batches gathered from a device-resident store (csrc/partnet_gather.hip) on the GPU: `DevicePartNetProducer`
against `PartNetBatchProducer` — the producer tests/test_datasets.py pins to the reference's `PartNetPartDataset` — bit
for bit, at the edges of the kernel's envelope, with replayed and device-drawn part orders, device-side indices under a
captured graph, the run-time bounds check, and as the feed of one captured training step."""
from pathlib import Path

import numpy as np
import pytest
import torch

from multi_part_assembly_amd import config, datasets, synthetic
from multi_part_assembly_amd.datasets import DevicePartNetProducer, PartNetBatchProducer, PartNetStore
from test_partnet_store import KEYS, part_orders, shape_dict
from test_semantic_device_gpu import pinned_noise  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

MINI = Path(__file__).resolve().parent / "golden" / "partnet_mini"
ALL_KEYS = ("part_pcs", "part_trans", "part_quat", "part_valids", "instance_label", "part_label", "part_ids", "match_ids",
            "contact_points", "sym", "valid_matrix", "shape_id", "data_id")


def numpy_batch(store, indices, P, C, keys, perm=None):
    """The host side of a batch from a store: padding plus `datasets.instance_labels` / `datasets.match_ids`, with the
    expressions of `PartNetBatchProducer.item`; `perm[b, :p]` reorders the parts (never the contact block)."""
    out = {k: [] for k in ("part_pcs", "part_trans", "part_quat", "part_valids", "shape_id", "instance_label",
                           "part_label") + tuple(k for k in keys if k != "part_label")}

    def pad(a):
        z = np.zeros((P,) + a.shape[1:], dtype=np.float32)
        z[: len(a)] = a
        return z

    for b, s in enumerate(indices):
        a, e = store.shape_part_off[s], store.shape_part_off[s + 1]
        p = e - a
        order = np.arange(p) if perm is None else np.asarray(perm[b][:p])
        geo, pose = store.geo_ids[a:e][order].astype(np.int64), pad(store.poses[a:e][order])
        valids = pad(np.ones(p, dtype=np.float32))
        one_hot = np.zeros((p, C), dtype=np.float32)
        if "part_label" in keys:
            one_hot[np.arange(p), store.sem_ids[a:e][order] - 1] = 1.0
        item = {"part_pcs": pad(store.pcs[a:e][order]), "part_trans": pose[:, :3], "part_quat": pose[:, 3:],
                "part_valids": valids, "shape_id": store.shape_ids[s], "instance_label": datasets.instance_labels(geo, P),
                "part_label": pad(one_hot), "part_ids": pad(geo), "match_ids": datasets.match_ids(geo, P),
                "sym": pad(store.sym[a:e][order]), "valid_matrix": valids[:, None] * valids[None, :]}
        if "contact_points" in keys:
            c = np.zeros((P, P, 4), dtype=np.float32)
            c[:p, :p] = store.contacts[store.contact_off[s]:store.contact_off[s + 1]].reshape(p, p, 4)
            item["contact_points"] = c
        for k in out:
            out[k].append(item[k])
    out = {k: np.stack(v) for k, v in out.items()}
    out["data_id"] = np.asarray(indices, dtype=np.int64)
    return out


def assert_batch_equal(got, want, keys=None):
    assert list(got) == list(want) if keys is None else set(keys) <= set(got)
    for k in (want if keys is None else keys):
        w = want[k].cpu().numpy() if isinstance(want[k], torch.Tensor) else np.asarray(want[k])
        g = got[k].cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=k)


def contacts_for(shapes, seed=1):
    rng = np.random.RandomState(seed)
    return [rng.standard_normal((len(d["geo_part_ids"]),) * 2 + (4,)).astype(np.float32) for d in shapes]


@pytest.fixture(scope="module")
def mini():
    store = PartNetStore.from_folder(str(MINI), "Chair.train.npy", min_num_part=2, max_num_part=8)
    host = {keys: PartNetBatchProducer(str(MINI), "Chair.train.npy", keys, num_part_category=5, max_num_part=8, device="cpu")
            for keys in (KEYS, KEYS[1:])}
    return store, host


# ---- 1. the reference's files, every key ----------------------------------------------------------------------------------
@pytest.mark.parametrize("indices", [[0, 2, 3, 1], [1]])
@pytest.mark.parametrize("keys", [KEYS, KEYS[1:]], ids=["part_label", "no_part_label"])
def test_partnet_mini_every_key_equals_the_host_producer(cuda_device, mini, indices, keys):
    store, host = mini
    want = host[keys].batch(indices)
    prod = DevicePartNetProducer(store, keys, num_part_category=5, max_num_part=8, device=cuda_device)
    got = prod.batch(indices)
    assert set(got) == set(ALL_KEYS) and list(got) == list(want)
    assert_batch_equal(got, want)
    assert got["part_label"].shape == (len(indices), 8, 5 if "part_label" in keys else 0)
    assert got["data_id"].device.type == "cpu" and got["data_id"].tolist() == indices
    assert all(v.device == cuda_device and v.is_contiguous() for k, v in got.items() if k != "data_id")
    prod.check()


# ---- 2. edges of the envelope ---------------------------------------------------------------------------------------------
def _edge_cases():
    rng = np.random.RandomState(4)
    docs = [[0, 4, 4, 4, 1, 2, 3], [0, 1, 1, 2, 3, 4, 4, 4]]  # the reference's docstring (partnet_data.py:113-125)
    wide = np.repeat(np.arange(1, 17), 4)[rng.permutation(64)]  # p = 64: sixteen groups of four, scattered
    return {
        "N5_dword_docstring_ids": (docs, 5, 9, 5, None),
        "N8_vec4_docstring_ids": (docs, 8, 8, 5, None),
        "N1000": ([[1, 1, 0], [2, 5]], 1000, 20, 5, None),
        "P4_no_padded_slot": ([[3, 3], [1, 1, 3, 3]], 8, 4, 5, None),
        "P64_full": ([wide, [7, 7]], 4, 64, 5, None),
        "ids_all_zero": ([[0] * 5, [0, 0]], 5, 6, 5, None),
        "ids_all_equal": ([[3] * 6, [9, 9]], 8, 6, 5, None),
        "C1": ([[2, 1, 2], [0, 1]], 5, 4, 1, [[1, 1, 1], [1, 1]]),
        "large_ids": ([[70000, 3, 70000, 16777215, 3], [16777215] * 2], 8, 5, 5, None),
    }


@pytest.mark.parametrize("case", list(_edge_cases()))
def test_edges_equal_the_host_label_functions(cuda_device, case):
    geos, N, P, C, sems = _edge_cases()[case]
    shapes = [shape_dict(g, n=N, seed=10 + i, sem=None if sems is None else sems[i]) for i, g in enumerate(geos)]
    store = PartNetStore.from_arrays(shapes, shape_ids=[40 + i for i in range(len(shapes))], contacts=contacts_for(shapes),
                                     max_num_part=P)
    prod = DevicePartNetProducer(store, KEYS, num_part_category=C, max_num_part=P, device=cuda_device)
    indices = [1, 0, 0, 1, 0]  # more than one block per sample, samples repeated
    got = prod.batch(indices)
    assert_batch_equal(got, numpy_batch(store, indices, P, C, KEYS), keys=ALL_KEYS)
    assert got["part_pcs"].shape == (5, P, N, 3) and got["part_label"].shape == (5, P, C)
    prod.check()


# ---- 3. every byte is written ---------------------------------------------------------------------------------------------
def test_every_output_byte_is_written_on_every_call(cuda_device, mini):
    store, host = mini
    prod = DevicePartNetProducer(store, KEYS, num_part_category=5, max_num_part=8, device=cuda_device)
    indices = [3, 0, 2]

    def poisoned():
        return {k: (torch.full(shape, float("nan"), dtype=dtype, device=cuda_device) if dtype.is_floating_point
                    else torch.full(shape, -7, dtype=dtype, device=cuda_device)) for k, (shape, dtype) in prod._spec(3).items()}

    out = poisoned()
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    got = prod.batch(indices, out=out)
    assert all(got[k] is out[k] and out[k].data_ptr() == ptrs[k] for k in out)
    assert not any(torch.isnan(v).any().item() for v in out.values() if v.dtype.is_floating_point)
    assert_batch_equal(got, host[KEYS].batch(indices))
    pad = got["part_valids"] == 0
    assert pad.sum().item() == 6 + 1 + 4
    for k in ("part_pcs", "part_trans", "part_quat", "sym", "part_ids", "match_ids", "instance_label", "part_label"):
        assert not got[k][pad].any().item(), k
    assert not got["contact_points"][pad].any().item() and not got["contact_points"].transpose(1, 2)[pad].any().item()
    again = prod.batch(indices, out=poisoned())
    assert all(torch.equal(again[k], got[k]) for k in got)
    with pytest.raises(ValueError, match="part_trans"):
        prod.batch(indices, out={"part_trans": torch.empty(3, 8, 4, device=cuda_device)})
    with pytest.raises(IndexError):
        prod.batch([0, 4])


# ---- 4. replayed part orders ----------------------------------------------------------------------------------------------
def test_replay_equals_the_shuffling_host_producer(cuda_device, mini):
    store, _ = mini
    host = PartNetBatchProducer(str(MINI), "Chair.train.npy", KEYS, num_part_category=5, max_num_part=8,
                                shuffle_parts=True, device="cpu")
    indices = [1, 0, 3, 2, 1]
    counts = np.diff(store.shape_part_off)[indices]
    np.random.seed(5)  # the draws PartNetBatchProducer.item will make, in its order: one permutation per sample
    perm = np.zeros((len(indices), 8), dtype=np.int32)
    for b, p in enumerate(counts):
        perm[b, :p] = np.random.permutation(p)
    np.random.seed(5)
    want = host.batch(indices)
    assert not np.array_equal(perm[0], np.arange(8))
    prod = DevicePartNetProducer(store, KEYS, num_part_category=5, max_num_part=8, device=cuda_device)
    got = prod.replay(indices, perm)
    assert_batch_equal(got, want)  # `contact_points` among them: it stays in stored order
    assert_batch_equal(got, numpy_batch(store, indices, 8, 5, KEYS, perm=perm), keys=ALL_KEYS)
    assert_batch_equal(prod.replay(indices, torch.from_numpy(perm).to(cuda_device)), want)
    prod.check()
    bad = perm.copy()
    bad[2, 1] = bad[2, 0]
    with pytest.raises(ValueError, match="not a permutation"):
        prod.replay(indices, bad)
    with pytest.raises(ValueError, match="perm must be"):
        prod.replay(indices, perm[:, :7])
    # a device-side order the wrapper cannot see: refused by the kernel — that sample is padding, the others stand
    got = prod.replay(torch.tensor(indices, device=cuda_device), torch.from_numpy(bad).to(cuda_device))
    assert got["part_valids"][2].sum().item() == 0 and not got["part_pcs"][2].any().item()
    keep = [0, 1, 3, 4]
    assert all(torch.equal(got[k][keep].cpu(), want[k][keep].cpu()) for k in want if k != "data_id")
    with pytest.raises(RuntimeError, match="no permutation"):
        prod.check()
    prod.check()


# ---- 5. device-random part orders -----------------------------------------------------------------------------------------
def test_device_random_order_is_the_documented_philox_shuffle(cuda_device, mini):
    shapes = [shape_dict([1, 1, 0, 2], n=4, seed=3)]
    store = PartNetStore.from_arrays(shapes, contacts=contacts_for(shapes), max_num_part=4)
    seed, B = 0x1234567890ABCDEF, 2048
    prod = DevicePartNetProducer(store, KEYS, num_part_category=5, max_num_part=4, shuffle_parts=True, seed=seed,
                                 device=cuda_device)
    indices = torch.zeros(B, dtype=torch.int64, device=cuda_device)
    got, order = prod.batch(indices, batch_counter=3, return_order=True)
    want = part_orders(seed, 3, B, 4)
    assert order.dtype == torch.int32 and np.array_equal(order.cpu().numpy(), want)
    assert len({tuple(r) for r in want.tolist()}) == 24  # every order of four parts occurs
    assert_batch_equal(got, numpy_batch(store, [0] * B, 4, 5, KEYS, perm=want), keys=ALL_KEYS[:-1])
    same, order2 = prod.batch(indices, batch_counter=3, return_order=True)
    assert torch.equal(order2, order) and all(torch.equal(same[k], got[k]) for k in got)
    word = torch.zeros(1, dtype=torch.int64, device=cuda_device)
    for value in (9, (1 << 33) + 2):  # the device word, rewritten between two calls
        word.fill_(value)
        _, order = prod.batch(indices, batch_counter=word, return_order=True)
        assert np.array_equal(order.cpu().numpy(), part_orders(seed, value, B, 4)), value
    assert prod.batch_counter == 0
    _, first = prod.batch(indices, return_order=True)  # the default counter: batches drawn so far
    _, second = prod.batch(indices, return_order=True)
    assert np.array_equal(first.cpu().numpy(), part_orders(seed, 0, B, 4))
    assert np.array_equal(second.cpu().numpy(), part_orders(seed, 1, B, 4)) and prod.batch_counter == 2
    # shapes of different part counts in one batch: row b follows the restatement for ITS p; padded slots are -1
    store, _ = mini
    prod = DevicePartNetProducer(store, KEYS, num_part_category=5, max_num_part=8, shuffle_parts=True, seed=5,
                                 device=cuda_device)
    idx = [0, 1, 2, 3, 2]
    got, order = prod.batch(idx, batch_counter=1, return_order=True)
    want = np.full((5, 8), -1, dtype=np.int64)
    for b, p in enumerate(np.diff(store.shape_part_off)[idx]):
        want[b, :p] = part_orders(5, 1, 5, p)[b]
    assert np.array_equal(order.cpu().numpy(), want)
    assert_batch_equal(got, numpy_batch(store, idx, 8, 5, KEYS, perm=np.maximum(want, 0)), keys=ALL_KEYS)


# ---- 6. indices in device memory, captured --------------------------------------------------------------------------------
def test_device_indices_and_a_captured_launch(cuda_device, mini):
    store, host = mini
    plain = DevicePartNetProducer(store, KEYS, num_part_category=5, max_num_part=8, device=cuda_device)
    idx = torch.tensor([2, 0, 3, 1], dtype=torch.int64, device=cuda_device)
    got = plain.batch(idx)
    assert got["data_id"] is idx
    assert_batch_equal(got, host[KEYS].batch([2, 0, 3, 1]))
    prod = DevicePartNetProducer(store, KEYS, num_part_category=5, max_num_part=8, shuffle_parts=True, seed=21,
                                 device=cuda_device)
    word = torch.full((1,), 4, dtype=torch.int64, device=cuda_device)
    out = {k: torch.zeros(shape, dtype=dtype, device=cuda_device) for k, (shape, dtype) in prod._spec(4).items()}
    prod.batch(idx, batch_counter=word, out=out)  # outside the capture first: the status word exists
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        prod.batch(idx, batch_counter=word, out=out)
    for values, counter in (([1, 1, 0, 2], 7), ([3, 2, 1, 0], (1 << 40) + 1)):
        idx.copy_(torch.tensor(values, device=cuda_device))
        word.fill_(counter)
        graph.replay()
        eager = prod.batch(values, batch_counter=counter)
        assert all(torch.equal(out[k], eager[k]) for k in out), (values, counter)
        assert not torch.equal(out["part_pcs"], plain.batch(values)["part_pcs"])  # (shuffled)
    prod.check()


# ---- 7. the run-time bounds check -----------------------------------------------------------------------------------------
def test_an_index_outside_the_store_is_padding_and_is_reported(cuda_device, mini):
    store, host = mini
    prod = DevicePartNetProducer(store, KEYS, num_part_category=5, max_num_part=8, device=cuda_device)
    want = host[KEYS].batch([0, 0, 2, 0])
    out = {k: torch.full(shape, float("nan") if dtype.is_floating_point else -7, dtype=dtype, device=cuda_device)
           for k, (shape, dtype) in prod._spec(4).items()}
    got = prod.batch(torch.tensor([0, len(store), 2, -1], dtype=torch.int64, device=cuda_device), out=out)
    for b in (1, 3):  # all padding, written (not left as it was)
        assert got["part_valids"][b].sum().item() == 0 and got["shape_id"][b].item() == -1
        assert all(not got[k][b].any().item() for k in got if k not in ("data_id", "shape_id")), b
    for k in want:
        if k != "data_id":
            assert torch.equal(got[k][[0, 2]].cpu(), want[k][[0, 2]]), k
    with pytest.raises(RuntimeError, match="outside the store"):
        prod.check()
    prod.check()  # reported once
    assert_batch_equal(prod.batch([1, 3]), host[KEYS].batch([1, 3]))
    prod.check()


# ---- 8. one captured training step --------------------------------------------------------------------------------------
def test_captured_step_fed_in_place_equals_the_host_built_batch(cuda_device, tmp_path, pinned_noise):  # noqa: F811
    from multi_part_assembly_amd.pn_transformer import build_model
    from multi_part_assembly_amd.trainer import Trainer
    cfg = config.dgl_partnet_chair()
    cfg.loss.match_sample = "device"
    P, N, keys = cfg.data.max_num_part, cfg.data.num_pc_points, tuple(cfg.data.data_keys)
    assert (P, N) == (20, 1000)
    store = synthetic.make_partnet_like_store(8, max_parts=P, num_points=N, seed=9)
    synthetic.write_partnet_folder(store, str(tmp_path))
    host = PartNetBatchProducer(str(tmp_path), "Chair.train.npy", keys, max_num_part=P, device=cuda_device)
    prod = DevicePartNetProducer(store, keys, max_num_part=P, device=cuda_device)

    def trainer():
        torch.manual_seed(3)
        return Trainer(build_model(cfg).to(cuda_device), cfg, use_graph=True, graph_warmup=1)

    a, b = trainer(), trainer()
    assert a.use_graph and a.static_batch is None
    steps = [[0, 1, 2, 3], [4, 5, 6, 7], [7, 2, 5, 0], [1, 6, 3, 4]]
    for idx in steps[:2]:  # one eager step, then the capture: both trainers on host-built batches
        assert float(a.train_step(host.batch(idx))) == float(b.train_step(host.batch(idx)))
    static = b.static_batch
    assert static is not None and b._graph is not None and set(keys) <= set(static)
    ptrs = {k: v.data_ptr() for k, v in static.items()}
    for idx in steps[2:]:
        want = a.train_step(host.batch(idx))
        fed = prod.batch(idx, out=static)
        assert all(fed[k] is static[k] for k in static)  # nothing left for the step to copy
        got = b.train_step(fed)
        assert np.isfinite(float(got)) and float(got) == float(want), (idx, float(got), float(want))
        assert_batch_equal(static, host.batch(idx), keys=list(static))
    assert b.static_batch is static and {k: v.data_ptr() for k, v in static.items()} == ptrs
    prod.check()
