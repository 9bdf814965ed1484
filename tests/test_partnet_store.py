"""`PartNetStore`, the argument contract of `mpa_partnet_gather_batch` and `DevicePartNetProducer` without a GPU; and the
numpy restatement of the documented device-random part order (include/mpa_hip.h: Philox tag, word layout, mulhi32 step)
that tests/test_partnet_gather_gpu.py uses as the oracle of the kernel's shuffle."""
import ctypes
import itertools
from pathlib import Path

import numpy as np
import pytest

from multi_part_assembly_amd import _build, _lib, datasets, synthetic
from multi_part_assembly_amd.datasets import DevicePartNetProducer, PartNetBatchProducer, PartNetStore
from test_mesh_store import philox4x32_10, philox4x32_10_np

MINI = Path(__file__).resolve().parent / "golden" / "partnet_mini"
KEYS = ("part_label", "part_ids", "match_ids", "contact_points", "sym", "valid_matrix")
ORDER_TAG = 0x706E0000


# ---- oracle restatements (shared with the GPU test) -----------------------------------------------------------------
def part_orders(seed, counter, B, p):
    """int64 [B, p]: the device-random part order of the samples 0..B-1 of a batch whose shapes all have p parts.
    Fisher-Yates on iota(p): for k = 0 .. p-2: j = k + mulhi32(w_k, p - k), swap; w_k = word k & 3 of the Philox block
    with counter (b, 0x706E0000 | (k >> 2), counter low word, high word) and key (seed low word, high word)."""
    seed, counter = int(seed) & 0xFFFFFFFFFFFFFFFF, int(counter) & 0xFFFFFFFFFFFFFFFF
    k0, k1, c0, c1 = seed & 0xFFFFFFFF, seed >> 32, counter & 0xFFFFFFFF, counter >> 32
    rows = np.arange(B)
    order = np.tile(np.arange(p, dtype=np.int64), (B, 1))
    blocks = {}
    for k in range(p - 1):
        if k >> 2 not in blocks:
            blocks[k >> 2] = philox4x32_10_np(rows.astype(np.uint64), ORDER_TAG | (k >> 2), c0, c1, k0, k1)
        w = blocks[k >> 2][k & 3]
        j = k + ((w * np.uint64(p - k)) >> np.uint64(32)).astype(np.int64)
        order[rows, k], order[rows, j] = order[rows, j], order[rows, k].copy()
    return order


def shape_dict(geo, n=5, sem=None, seed=0):
    """One shape in the layout of a `shape_data` file, seeded; `geo`: its geo_part_ids."""
    rng = np.random.RandomState(seed)
    p = len(geo)
    return {"part_pcs": rng.standard_normal((p, n, 3)).astype(np.float32),
            "part_poses": rng.standard_normal((p, 7)).astype(np.float32),
            "part_ids": np.asarray(rng.randint(1, 6, size=p) if sem is None else sem, dtype=np.int64),
            "geo_part_ids": np.asarray(geo, dtype=np.int64),
            "sym": rng.randint(0, 2, size=(p, 3)).astype(np.float32)}


@pytest.fixture(scope="module")
def built():
    return _build.build()


# ---- 1. the store from the reference's files ----------------------------------------------------------------------------
def test_store_from_partnet_mini_is_the_files_bit_for_bit():
    host = PartNetBatchProducer(str(MINI), "Chair.train.npy", KEYS, num_part_category=5, max_num_part=8, device="cpu")
    store = PartNetStore.from_folder(str(MINI), "Chair.train.npy", min_num_part=2, max_num_part=8)
    assert store.shape_ids.tolist() == [int(s) for s in host.shape_ids] == [101, 102, 103, 105]  # 104 has nine parts
    assert len(store) == 4 and store.num_points == 32 and store.has_contacts
    assert store.shape_part_off.tolist() == [0, 7, 15, 19, 21] and store.contact_off.tolist() == [0, 49, 113, 129, 133]
    for name, dtype in (("pcs", np.float32), ("poses", np.float32), ("sym", np.float32), ("geo_ids", np.int32),
                        ("sem_ids", np.int32), ("shape_part_off", np.int64), ("shape_ids", np.int64),
                        ("contacts", np.float32), ("contact_off", np.int64)):
        assert getattr(store, name).dtype == dtype, name
    for s, shape_id in enumerate(host.shape_ids):
        cur = host._load(shape_id)
        a, b = store.shape_part_off[s], store.shape_part_off[s + 1]
        assert np.array_equal(store.pcs[a:b], np.asarray(cur["part_pcs"]).astype(np.float32))
        assert np.array_equal(store.poses[a:b], np.asarray(cur["part_poses"]).astype(np.float32))
        assert np.array_equal(store.sym[a:b], np.asarray(cur["sym"]).astype(np.float32))
        assert np.array_equal(store.geo_ids[a:b], cur["geo_part_ids"])
        assert np.array_equal(store.sem_ids[a:b], cur["part_ids"])
        contact = np.load(MINI / "contact_points" / f"pairs_with_contact_points_{shape_id}_level3.npy", allow_pickle=True)
        block = store.contacts[store.contact_off[s]:store.contact_off[s + 1]].reshape(b - a, b - a, 4)
        assert np.array_equal(block, contact.astype(np.float32))
    assert PartNetStore.from_folder(str(MINI), "Chair.train.npy", max_num_part=8, overfit=2).shape_ids.tolist() == [101, 102]
    assert len(PartNetStore.from_folder(str(MINI), "Chair.train.npy", max_num_part=20)) == 5
    assert not PartNetStore.from_folder(str(MINI), "Chair.train.npy", max_num_part=8, with_contacts=False).has_contacts


def test_synthetic_store_is_seeded_and_writes_the_reference_format(tmp_path):
    a = synthetic.make_partnet_like_store(6, max_parts=20, num_points=16, seed=3)
    b = synthetic.make_partnet_like_store(6, max_parts=20, num_points=16, seed=3)
    c = synthetic.make_partnet_like_store(6, max_parts=20, num_points=16, seed=4)
    assert all(np.array_equal(getattr(a, n), getattr(b, n)) for n in PartNetStore.ARRAYS + ("contacts", "contact_off"))
    assert not np.array_equal(a.pcs, c.pcs)
    state = np.random.get_state()[1].copy()
    synthetic.make_partnet_like_store(2, num_points=4)
    assert np.array_equal(np.random.get_state()[1], state)  # numpy's global generator is not touched
    synthetic.write_partnet_folder(a, str(tmp_path))
    back = PartNetStore.from_folder(str(tmp_path), "Chair.train.npy")
    assert all(np.array_equal(getattr(a, n), getattr(back, n)) for n in PartNetStore.ARRAYS + ("contacts", "contact_off"))
    host = PartNetBatchProducer(str(tmp_path), "Chair.train.npy", KEYS, device="cpu")
    assert [int(s) for s in host.shape_ids] == a.shape_ids.tolist()
    assert host.item(1)["match_ids"].max() >= 1  # every shape has a group of identical parts


# ---- 2. round trip and validation ---------------------------------------------------------------------------------------
def test_save_load_round_trip_and_validation(tmp_path):
    store = PartNetStore.from_folder(str(MINI), "Chair.train.npy", max_num_part=8)
    store.save(tmp_path / "store.npz")
    with np.load(tmp_path / "store.npz", allow_pickle=False) as z:  # plain arrays: no pickle
        assert set(z.files) == set(PartNetStore.ARRAYS) | {"contacts", "contact_off", "part_limits"}
    back = PartNetStore.load(tmp_path / "store.npz")
    for n in PartNetStore.ARRAYS + ("contacts", "contact_off"):
        assert np.array_equal(getattr(store, n), getattr(back, n)) and getattr(store, n).dtype == getattr(back, n).dtype, n
    assert (back.min_num_part, back.max_num_part) == (2, 8)
    assert back.nbytes == store.nbytes == sum(getattr(store, n).nbytes for n in PartNetStore.ARRAYS + ("contacts", "contact_off"))
    assert PartNetStore.load(tmp_path / "store.npz", max_bytes=store.nbytes).nbytes == store.nbytes
    with pytest.raises(ValueError, match="max_bytes"):
        PartNetStore.load(tmp_path / "store.npz", max_bytes=store.nbytes - 1)
    with pytest.raises(ValueError, match="max_bytes"):
        PartNetStore.from_folder(str(MINI), "Chair.train.npy", max_num_part=8, max_bytes=1000)
    plain = PartNetStore.from_arrays([shape_dict([0, 1, 1])])
    plain.save(tmp_path / "plain.npz")
    assert not PartNetStore.load(tmp_path / "plain.npz").has_contacts

    args = [getattr(store, n) for n in PartNetStore.ARRAYS]
    kw = dict(min_num_part=2, max_num_part=8)
    PartNetStore(*args, **kw)
    bad = list(args)
    bad[5] = np.array([0, 7, 15, 19, 20])
    with pytest.raises(ValueError, match="offsets"):
        PartNetStore(*bad, **kw)
    bad = list(args)
    bad[1] = args[1][:-1]
    with pytest.raises(ValueError, match="offsets"):
        PartNetStore(*bad, **kw)
    with pytest.raises(ValueError, match="offsets"):  # contact blocks that are not p x p
        PartNetStore(*args, store.contacts, store.contact_off + 1, **kw)
    with pytest.raises(ValueError, match="come together"):
        PartNetStore(*args, store.contacts, None, **kw)
    with pytest.raises(ValueError, match="one N"):
        PartNetStore.from_arrays([shape_dict([1, 1], n=5), shape_dict([1, 1], n=6)])
    with pytest.raises(ValueError, match="part count outside"):
        PartNetStore.from_arrays([shape_dict([1])])
    with pytest.raises(ValueError, match="part count outside"):
        PartNetStore.from_arrays([shape_dict([1, 1, 2, 3])], max_num_part=3)
    with pytest.raises(ValueError, match="part count outside"):
        PartNetStore(*args, min_num_part=2, max_num_part=7)
    with pytest.raises(ValueError, match="start from 1"):
        PartNetStore.from_arrays([shape_dict([1, 1], sem=[1, 0])])
    with pytest.raises(ValueError, match="geo_ids"):
        PartNetStore.from_arrays([shape_dict([1, -1])])
    with pytest.raises(ValueError, match="no shapes"):
        PartNetStore.from_arrays([])
    with pytest.raises(ValueError, match=r"\[p, p, 4\]"):
        PartNetStore.from_arrays([shape_dict([1, 1])], contacts=[np.zeros((3, 3, 4))])


# ---- 3. the documented device-random order --------------------------------------------------------------------------------
def test_part_order_restatement_follows_the_documented_layout():
    for p in (1, 2, 3, 7, 20, 64):
        rows = part_orders(seed=11, counter=5, B=50, p=p)
        assert rows.shape == (50, p) and (np.sort(rows, axis=1) == np.arange(p)).all()
    # by hand, word for word: sample b = 5 of a batch, p = 6 -> w_0..w_3 from block 0, w_4 from block 1
    seed, counter = 0x0123456789ABCDEF, (3 << 32) + 7
    key = [0x89ABCDEF, 0x01234567]
    w = philox4x32_10([5, 0x706E0000, 7, 3], key) + philox4x32_10([5, 0x706E0001, 7, 3], key)
    order = list(range(6))
    for k in range(5):
        j = k + ((w[k] * (6 - k)) >> 32)
        assert k <= j < 6
        order[k], order[j] = order[j], order[k]
    assert part_orders(seed, counter, 6, 6)[5].tolist() == order
    # the tag is one neither other user of the generator produces: the mesh sampler's word 1 is below 4, the match
    # sampler's is 0x6D61xxxx
    assert ORDER_TAG >= 4 and (ORDER_TAG >> 16) != 0x6D61 and ((ORDER_TAG | 15) >> 16) == ORDER_TAG >> 16
    assert not np.array_equal(part_orders(1, 0, 8, 6), part_orders(1, 1, 8, 6))
    assert not np.array_equal(part_orders(1, 0, 8, 6), part_orders(2, 0, 8, 6))
    assert not np.array_equal(part_orders(1, 0, 8, 6), part_orders(1, 1 << 32, 8, 6))


def test_part_order_restatement_is_uniform_over_the_24_orders_of_four_parts():
    """Chi-square over the 24 orders of p = 4 from 24 000 draws: below the 0.999 quantile of df = 23.  Deterministic."""
    rows = part_orders(seed=2024, counter=0, B=24000, p=4)
    index = {perm: i for i, perm in enumerate(itertools.permutations(range(4)))}
    counts = np.bincount([index[tuple(r)] for r in rows.tolist()], minlength=24)
    chi2 = float(((counts - 1000.0) ** 2 / 1000.0).sum())
    print("chi2", chi2)
    assert counts.sum() == 24000 and chi2 < 49.7


# ---- 4. the C entry point and the producer without a GPU ----------------------------------------------------------------
def test_partnet_gather_batch_validates_its_arguments(built):
    assert "mpa_partnet_gather_batch" in _lib.declared_functions()
    assert len(_lib.SIGNATURES["mpa_partnet_gather_batch"][1]) == 35
    L = _lib.lib()
    assert L.mpa_abi_version() == 10  # a new symbol, no changed signature
    one = ctypes.c_void_p(16)  # a non-null pointer that validation never dereferences

    def call(B=2, P=4, N=8, C=0, S=3, store=one, contacts=None, index=one, perm=None, random_order=0, outs=one,
             part_label=None, contact_points=None, status=one, sem=one):
        return L.mpa_partnet_gather_batch(store, store, store, store, sem, store, store, contacts, contacts, S, index, B,
                                          P, N, C, perm, random_order, 1, 0, None, outs, outs, outs, outs, outs, outs,
                                          outs, part_label, contact_points, outs, outs, outs, None, status, None)

    assert call(P=0) == -1 and b"P=0" in L.mpa_last_error()
    assert call(P=65) == -1 and b"P=65" in L.mpa_last_error()
    assert call(B=-1) == -1 and b"negative" in L.mpa_last_error()
    assert call(N=-8) == -1 and call(C=-1) == -1 and call(S=-1) == -1
    assert call(B=0, P=65) == -1  # sizes are checked before the empty batch returns
    assert call(B=0) == 0 and call(B=0, store=None, index=None, outs=None, status=None) == 0
    assert call(index=None) == -1 and b"null" in L.mpa_last_error()
    assert call(status=None) == -1 and b"null" in L.mpa_last_error()
    assert call(store=None) == -1 and b"null" in L.mpa_last_error()
    assert call(C=5, part_label=one, sem=None) == -1 and b"null" in L.mpa_last_error()
    assert call(contact_points=one) == -1 and b"without contacts" in L.mpa_last_error()
    assert call(B=0, contact_points=one) == -1
    assert call(perm=one, random_order=1) == -1 and b"exclude" in L.mpa_last_error()


def test_device_producer_has_no_cpu_fallback_and_checks_its_keys():
    store = PartNetStore.from_folder(str(MINI), "Chair.train.npy", max_num_part=8)
    prod = DevicePartNetProducer(store, KEYS, num_part_category=5, max_num_part=8, device="cpu")
    assert len(prod) == 4
    with pytest.raises(RuntimeError, match="HIP device only"):
        prod.batch([0, 1])
    with pytest.raises(RuntimeError, match="HIP device only"):
        prod.replay([0], np.zeros((1, 8), np.int32))
    with pytest.raises(RuntimeError, match="HIP device only"):
        store.device_arrays("cpu")
    prod.check()  # nothing launched: nothing to report
    with pytest.raises(ValueError, match="ERROR: unknown data bbox"):
        DevicePartNetProducer(store, ("part_ids", "bbox"), max_num_part=8)
    with pytest.raises(ValueError, match="part count outside"):
        DevicePartNetProducer(store, KEYS, num_part_category=5, max_num_part=7)
    with pytest.raises(ValueError, match="part count outside"):
        DevicePartNetProducer(store, KEYS, num_part_category=5, min_num_part=3, max_num_part=8)
    with pytest.raises(ValueError, match="num_part_category"):
        DevicePartNetProducer(store, KEYS, num_part_category=4, max_num_part=8)
    DevicePartNetProducer(store, ("part_ids",), num_part_category=4, max_num_part=8)  # no part_label: no limit on it
    with pytest.raises(ValueError, match="max_num_part"):
        DevicePartNetProducer(store, KEYS, num_part_category=5, max_num_part=65)
    bare = PartNetStore.from_folder(str(MINI), "Chair.train.npy", max_num_part=8, with_contacts=False)
    with pytest.raises(ValueError, match="without contacts"):
        DevicePartNetProducer(bare, KEYS, num_part_category=5, max_num_part=8)
    spec = prod._spec(3)
    assert list(spec) == ["part_pcs", "part_trans", "part_quat", "part_valids", "shape_id", "instance_label", "part_label",
                          "part_ids", "match_ids", "contact_points", "sym", "valid_matrix"]
    assert spec["part_label"][0] == (3, 8, 5) and spec["part_pcs"][0] == (3, 8, 32, 3)
    assert DevicePartNetProducer(store, ("part_ids",), max_num_part=8)._spec(3)["part_label"][0] == (3, 8, 0)


def test_trainer_static_batch_is_none_before_the_capture():
    from multi_part_assembly_amd.trainer import Trainer
    assert isinstance(Trainer.static_batch, property) and Trainer.static_batch.fset is None
