"""The epoch order without a GPU: the numpy restatement of `mpa_epoch_order` (multi_part_assembly_amd/sampler_ref.py, the
oracle of tests/test_epoch_order_gpu.py), its sharding against torch's `DistributedSampler`, `EpochSampler`'s batch
counts and resume state, the argument contract of the new entry points, the bookkeeping of `fit.fit` with a stub trainer,
and tools/train.py's argument parser."""
import ctypes
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DistributedSampler

from multi_part_assembly_amd import _build, _lib, fit as fit_mod, sampler_ref
from multi_part_assembly_amd.sampler import EpochSampler
from test_mesh_store import philox4x32_10
from tool_loader import load_tool


@pytest.fixture(scope="module")
def built():
    return _build.build()


# ---- 1. the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 3, 64, 1000])
def test_restatement_is_a_permutation_shared_by_the_ranks(S):
    perm = sampler_ref.epoch_permutation(S, seed=5, epoch=3)
    assert perm.dtype == np.int64 and np.array_equal(np.sort(perm), np.arange(S))
    # every rank strides the SAME permutation: interleaving the shards gives it back, padded by wrapping around
    for world in (1, 2, 3):
        shards = [sampler_ref.epoch_order(S, 5, 3, world, r) for r in range(world)]
        total = -(-S // world) * world
        assert all(len(s) == total // world for s in shards)
        assert np.array_equal(np.stack(shards, axis=1).reshape(-1), perm[np.arange(total) % S])


def test_restatement_differs_between_epochs_and_seeds():
    base = sampler_ref.epoch_permutation(1000, seed=1, epoch=0)
    assert not np.array_equal(base, sampler_ref.epoch_permutation(1000, seed=1, epoch=1))
    assert not np.array_equal(base, sampler_ref.epoch_permutation(1000, seed=2, epoch=0))
    assert not np.array_equal(base, sampler_ref.epoch_permutation(1000, seed=1 | (1 << 32), epoch=0))
    assert not np.array_equal(base, sampler_ref.epoch_permutation(1000, seed=1, epoch=1 << 32))
    assert np.array_equal(base, sampler_ref.epoch_permutation(1000, seed=1, epoch=0))


@pytest.mark.parametrize("seed,epoch,i", [(0, 0, 0), (7, 1, 5), ((3 << 32) | 9, (1 << 32) + 5, 999), (2 ** 64 - 1, 2, 63)])
def test_keys_follow_the_documented_counter_layout(seed, epoch, i):
    """key_i = x | (y << 32) of the block with counter (i, 0x65700000, epoch low, epoch high) and key (seed low, seed
    high), from the plain-int Philox of tests/test_mesh_store.py (which reproduces the published vectors)."""
    w = philox4x32_10([i, 0x65700000, epoch & 0xFFFFFFFF, epoch >> 32], [seed & 0xFFFFFFFF, seed >> 32])
    assert int(sampler_ref.epoch_keys(1000, seed, epoch)[i]) == w[0] | (w[1] << 32)
    assert sampler_ref.ORDER_TAG == 0x65700000  # the mesh sampler: < 4; the match sampler: 0x6D61xxxx; PartNet: 0x706Exxxx


def test_position_of_an_element_is_uniform():
    """Chi-square of the position of element 0 over 2 000 epochs at S = 8 against the 99.9 % critical value for 7 degrees
    of freedom."""
    pos = [int(np.nonzero(sampler_ref.epoch_permutation(8, seed=2024, epoch=e) == 0)[0][0]) for e in range(2000)]
    counts = np.bincount(pos, minlength=8)
    chi2 = float(((counts - 250.0) ** 2 / 250.0).sum())
    assert chi2 < 24.32, (chi2, counts)


def test_ties_are_broken_by_index():
    keys = np.array([5, 1, 5, 1, 0], dtype=np.uint64)
    assert np.argsort(keys, kind="stable").tolist() == [4, 1, 3, 0, 2]  # what epoch_permutation applies to the keys


# ---- 2. sharding against torch's DistributedSampler ---------------------------------------------------------------------
@pytest.mark.parametrize("S,world", [(10, 1), (10, 3), (7, 4), (64, 2)])
def test_sharding_is_the_distributed_samplers(S, world):
    perm = sampler_ref.epoch_permutation(S, seed=11, epoch=2)
    seen = []
    for rank in range(world):
        ds = DistributedSampler(range(S), num_replicas=world, rank=rank, shuffle=False, drop_last=False)
        want = perm[np.array(list(ds), dtype=np.int64)]  # positions of the padded arange -> entries of the permutation
        got = sampler_ref.epoch_order(S, 11, 2, world, rank)
        assert len(got) == len(ds) == -(-S // world)
        assert np.array_equal(got, want)
        plain = sampler_ref.epoch_order(S, world=world, rank=rank, shuffle=False)
        assert np.array_equal(plain, np.array(list(ds), dtype=np.int64))
        seen.append(got)
    assert np.array_equal(np.unique(np.concatenate(seen)), np.arange(S))  # the ranks cover every index


def test_sharding_with_more_ranks_than_shapes():
    for rank in range(3):
        ds = DistributedSampler(range(1), num_replicas=3, rank=rank, shuffle=False, drop_last=False)
        assert sampler_ref.epoch_order(1, 4, 0, 3, rank).tolist() == list(ds) == [0]


# ---- 3. EpochSampler on the host ------------------------------------------------------------------------------------------
def test_batch_counts_and_views():
    s = EpochSampler(10, 4, seed=3, world=1, rank=0, drop_last=True, device="cpu")
    assert len(s) == 2
    s.set_epoch(1)
    batches = list(s)
    assert [len(b) for b in batches] == [4, 4] and all(b.dtype == torch.int64 for b in batches)
    assert np.array_equal(torch.cat(batches).numpy(), sampler_ref.epoch_order(10, 3, 1)[:8])
    assert batches[0].data_ptr() == s.order.data_ptr()  # views of the epoch's vector, no copies
    v = EpochSampler(10, 4, world=1, shuffle=False, drop_last=False, device="cpu")
    assert len(v) == 3
    v.set_epoch(0)
    assert [b.tolist() for b in v] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    r = EpochSampler(10, 2, seed=3, world=3, rank=2, device="cpu")  # total / world = 4
    assert len(r) == 2 and r.shard_len == 4
    assert len(EpochSampler(8, 4, drop_last=False, device="cpu")) == 2
    for bad in (dict(num_shapes=0, batch_size=1), dict(num_shapes=4, batch_size=0), dict(num_shapes=4, batch_size=1, world=0),
                dict(num_shapes=4, batch_size=1, world=2, rank=2), dict(num_shapes=4, batch_size=1, rank=-1)):
        with pytest.raises(ValueError):
            EpochSampler(device="cpu", **bad)


def test_state_round_trip_mid_epoch():
    a = EpochSampler(23, 3, seed=9, world=2, rank=1, device="cpu")
    a.set_epoch(4)
    full = [b.tolist() for b in a]
    assert len(full) == len(a) == 4
    a.set_epoch(4)
    it = iter(a)
    head = [next(it).tolist(), next(it).tolist()]
    state = a.state_dict()
    assert state == {"seed": 9, "epoch": 4, "next_step": 2}
    b = EpochSampler(23, 3, seed=0, world=2, rank=1, device="cpu")
    b.load_state_dict(state)
    assert head + [x.tolist() for x in b] == full
    b.set_epoch(5)
    assert b.next_step == 0 and len(list(b)) == 4


# ---- 4. the entry points without a GPU --------------------------------------------------------------------------------------
def test_entry_points_exist_and_validate_without_a_gpu(built):
    L = _lib.lib()
    for name in ("mpa_epoch_order", "mpa_epoch_order_workspace", "mpa_mesh_slot_table"):
        assert name in _lib.SIGNATURES and name in _lib.declared_functions()
    one = ctypes.c_void_p(8)  # a non-null, aligned pointer that validation never dereferences
    n = ctypes.c_int64()
    assert L.mpa_epoch_order_workspace(1000, ctypes.byref(n)) == 0 and n.value == 8000
    assert L.mpa_epoch_order_workspace(1 << 18, ctypes.byref(n)) == 0 and n.value == 8 << 18
    assert L.mpa_epoch_order_workspace((1 << 18) + 1, ctypes.byref(n)) == -1 and b"maximum" in L.mpa_last_error()
    assert L.mpa_epoch_order_workspace(0, ctypes.byref(n)) == -1
    assert sampler_ref.MAX_SHAPES == 1 << 18

    def call(S, world, rank, ws=one, out=one):
        return L.mpa_epoch_order(S, world, rank, 1, 0, None, ws, out, None)

    assert call(0, 1, 0) == -1 and b"S=0" in L.mpa_last_error()
    assert call(-5, 1, 0) == -1
    assert call(10, 0, 0) == -1 and b"world=0" in L.mpa_last_error()
    assert call(10, 2, 2) == -1 and b"rank=2" in L.mpa_last_error()
    assert call(10, 2, -1) == -1
    assert call((1 << 18) + 1, 1, 0) == -1 and b"maximum" in L.mpa_last_error()  # before any launch
    assert call(10, 1, 0, ws=None) == -1 and b"null" in L.mpa_last_error()
    assert call(10, 1, 0, out=None) == -1
    assert call(10, 1, 0, ws=ctypes.c_void_p(4)) == -1 and b"aligned" in L.mpa_last_error()

    def table(B, P, lo, hi, ptrs=one):
        return L.mpa_mesh_slot_table(ptrs, 4, ptrs, B, P, lo, hi, 0, ptrs, ptrs, ptrs, ptrs, ptrs, None)

    assert table(-1, 4, 2, 4) == -1 and b"negative" in L.mpa_last_error()
    assert table(2, 0, 0, 0) == -1 and b"P=0" in L.mpa_last_error()
    assert table(2, 4, 2, 5) == -1 and b"limits" in L.mpa_last_error()
    assert table(2, 4, 3, 2) == -1
    assert table(2, 4, 2, 4, ptrs=None) == -1 and b"null" in L.mpa_last_error()
    assert table(0, 4, 2, 4, ptrs=None) == 0


def test_cuda_sampler_refuses_more_shapes_than_the_kernel_sorts():
    with pytest.raises(ValueError, match="mpa_epoch_order"):
        EpochSampler((1 << 18) + 1, 32, device="cuda")
    EpochSampler((1 << 18) + 1, 32, shuffle=False, device="cpu")  # arange needs no kernel


# ---- 5. fit's bookkeeping with a stub trainer ---------------------------------------------------------------------------------
class StubOptimizer:
    lr = 0.0


class StubProducer:
    def __init__(self):
        self.batch_counter = 0
        self.seen = []

    def batch(self, indices):
        self.batch_counter += 1
        self.seen.append(indices.tolist())
        return {"idx": indices}


class StubTrainer:
    """Records every call `fit` makes; the loss of a step is the sum of its indices, the validation metrics are given."""

    static_batch = None

    def __init__(self, scores=None, monitor="val/part_acc"):
        self.calls, self.optimizer, self.epoch, self.steps = [], StubOptimizer(), 0, 0
        self.scores, self.monitor = scores or {}, monitor

    def set_epoch(self, epoch):
        self.epoch = epoch
        self.optimizer.lr = 0.1 / (1 + epoch)
        self.calls.append(("set_epoch", epoch))

    def train_step(self, batch):
        self.steps += 1
        self.calls.append(("step", batch["idx"].tolist()))
        return batch["idx"].sum().float()

    def check_health(self):
        self.calls.append(("health",))

    def evaluate(self, batches):
        self.calls.append(("evaluate", len(list(batches))))
        return {self.monitor: self.scores[self.epoch], "val/other": 1.0}

    def state_dict(self):
        self.calls.append(("state_dict", self.epoch))
        return {"model": {}, "optimizer": None, "epoch": self.epoch, "steps": self.steps}

    def load_state_dict(self, state):
        self.epoch, self.steps = state["epoch"], state["steps"]


def _files(path):
    return sorted(os.listdir(path))


def test_fit_call_order_validation_epochs_and_history(tmp_path):
    trainer, prod = StubTrainer(scores={1: 0.5, 3: 0.25}), StubProducer()
    sampler = EpochSampler(5, 2, seed=4, device="cpu")
    logged = []
    history = fit_mod.fit(trainer, prod, sampler, val_batches=[1, 2, 3], epochs=4, val_every=2, ckpt_dir=str(tmp_path),
                          keep=5, log_every=1, on_log=logged.append)
    want = []
    for e in range(4):
        want.append(("set_epoch", e))
        order = sampler_ref.epoch_order(5, 4, e)
        for k in range(2):
            want += [("step", order[2 * k:2 * k + 2].tolist()), ("health",)]
        if e in (1, 3):
            want.append(("evaluate", 3))
        want.append(("state_dict", e))
    assert trainer.calls == want
    assert [h["epoch"] for h in history] == [0, 1, 2, 3]
    assert [h["lr"] for h in history] == [0.1 / (1 + e) for e in range(4)]
    assert ["val/part_acc" in h for h in history] == [False, True, False, True]
    for e, h in enumerate(history):
        assert h["train/loss"] == pytest.approx(sampler_ref.epoch_order(5, 4, e)[:4].sum() / 2)
    assert [r for r in logged if "step" not in r] == history and len([r for r in logged if "step" in r]) == 8
    assert prod.batch_counter == 8
    assert _files(tmp_path) == ["last.pt"] + [f"model-epoch={e:03d}.pt" for e in range(4)]  # no temporary name is left
    last = torch.load(tmp_path / "last.pt", weights_only=False)
    assert last["epoch"] == 3 and last["fit"]["next_epoch"] == 4 and last["fit"]["batch_counters"] == [8]
    assert last["fit"]["sampler"] == {"seed": 4, "epoch": 3, "next_step": 2} and last["fit"]["history"] == history


@pytest.mark.parametrize("monitor,scores,kept", [
    ("val/part_acc", [0.1, 0.9, 0.3, 0.8, 0.2], [1, 3]),       # higher is better
    ("val/loss", [0.1, 0.9, 0.3, 0.8, 0.2], [0, 4]),           # lower is better
])
def test_fit_keeps_the_best_checkpoints_and_last(tmp_path, monitor, scores, kept):
    trainer = StubTrainer(scores=dict(enumerate(scores)), monitor=monitor)
    fit_mod.fit(trainer, StubProducer(), EpochSampler(4, 2, device="cpu"), val_batches=[0], epochs=5, val_every=1,
                ckpt_dir=str(tmp_path), keep=2, monitor=monitor, log_every=0)
    assert _files(tmp_path) == ["last.pt"] + [f"model-epoch={e:03d}.pt" for e in kept]
    assert torch.load(tmp_path / "last.pt", weights_only=False)["epoch"] == 4  # the newest, whatever its score


def test_fit_without_validation_keeps_the_newest(tmp_path):
    fit_mod.fit(StubTrainer(), StubProducer(), EpochSampler(4, 2, device="cpu"), epochs=4, ckpt_dir=str(tmp_path), keep=2,
                log_every=0)
    assert _files(tmp_path) == ["last.pt", "model-epoch=002.pt", "model-epoch=003.pt"]


@pytest.mark.parametrize("stop", [2, 3])  # at the end of epoch 0, and inside epoch 1
def test_resume_continues_with_the_batches_of_the_uninterrupted_run(tmp_path, stop):
    whole_t, whole_p = StubTrainer(), StubProducer()
    whole = fit_mod.fit(whole_t, whole_p, EpochSampler(5, 2, seed=8, device="cpu"), epochs=3, log_every=0)
    first_t, first_p = StubTrainer(), StubProducer()
    fit_mod.fit(first_t, first_p, EpochSampler(5, 2, seed=8, device="cpu"), epochs=3, ckpt_dir=str(tmp_path), log_every=0,
                max_steps=stop)
    assert "last.pt.tmp" not in _files(tmp_path)
    second_t, second_p = StubTrainer(), StubProducer()
    assert fit_mod.resume(second_t, str(tmp_path)) == stop // 2
    history = fit_mod.fit(second_t, second_p, EpochSampler(5, 2, seed=0, device="cpu"), epochs=3, ckpt_dir=str(tmp_path),
                          log_every=0)
    assert first_p.seen + second_p.seen == whole_p.seen and len(first_p.seen) == stop
    assert second_p.batch_counter == whole_p.batch_counter and second_t.steps == whole_t.steps
    assert history == whole
    assert fit_mod.resume(StubTrainer(), str(tmp_path / "nothing")) == 0


def test_a_second_fit_with_the_same_sampler_starts_its_epochs_anew():
    trainer, prod, sampler = StubTrainer(), StubProducer(), EpochSampler(5, 2, seed=8, device="cpu")
    first = fit_mod.fit(trainer, prod, sampler, epochs=1, log_every=0)
    seen = list(prod.seen)
    again = fit_mod.fit(trainer, prod, sampler, epochs=2, log_every=0)  # the sampler was left at the end of epoch 0
    assert len(seen) == 2 and prod.seen[2:4] == seen and len(prod.seen) == 6
    assert again[0] == first[0] and [h["epoch"] for h in again] == [0, 1]


def test_rng_states_travel_with_the_checkpoint(tmp_path):
    import random
    trainer = StubTrainer()
    torch.manual_seed(5), np.random.seed(6), random.seed(7)
    fit_mod.fit(trainer, StubProducer(), EpochSampler(4, 2, device="cpu"), epochs=1, ckpt_dir=str(tmp_path), log_every=0)
    want = (torch.rand(2), np.random.rand(2), random.random())
    torch.manual_seed(0), np.random.seed(0), random.seed(0)
    fresh = StubTrainer()
    assert fit_mod.resume(fresh, str(tmp_path)) == 1
    fit_mod.fit(fresh, StubProducer(), EpochSampler(4, 2, device="cpu"), epochs=1, log_every=0)  # nothing left to run
    got = (torch.rand(2), np.random.rand(2), random.random())
    assert torch.equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


# ---- 6. the tool's arguments ------------------------------------------------------------------------------------------------
def test_train_tool_arguments():
    tool = load_tool("train")
    a = tool.parse_args(["--preset", "pn_transformer_everyday", "--synthetic", "--epochs", "2"])
    assert a.synthetic and a.epochs == 2 and not a.graph and not a.resume and a.ckpt_dir == "" and a.log_every == 50
    a = tool.parse_args(["--preset", "dgl_partnet_chair", "--data-dir", "d", "--data-fn", "Chair.train.npy", "--val-fn",
                         "Chair.val.npy", "--category", "Chair", "--graph", "--ckpt-dir", "c", "--resume"])
    assert (a.data_dir, a.data_fn, a.val_fn, a.category, a.graph, a.ckpt_dir, a.resume) == \
        ("d", "Chair.train.npy", "Chair.val.npy", "Chair", True, "c", True)
    for bad in (["--synthetic"], ["--preset", "p"], ["--preset", "p", "--data-dir", "d"],
                ["--preset", "p", "--synthetic", "--resume"]):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)
