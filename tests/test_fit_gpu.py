"""`Trainer.fit` / `Trainer.resume` on the device: the loop equals a hand-written loop over the restatement's index batches
bit for bit (parameters and optimiser moments), captured equals eager, a resumed run equals the uninterrupted one (at an
epoch's end and inside an epoch), validation leaves the run alone, the loop reads the device once per `log_every` steps
and once per epoch, two ranks stride one order, and tools/train.py runs end to end on synthetic data."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from multi_part_assembly_amd import config, sampler_ref, synthetic
from multi_part_assembly_amd.datasets import DeviceGeometryProducer, DevicePartNetProducer, MeshStore
from multi_part_assembly_amd.optim import cosine_warmup_lr
from multi_part_assembly_amd.pn_transformer import build_model
from multi_part_assembly_amd.sampler import EpochSampler
from multi_part_assembly_amd.trainer import Trainer
from test_assemble_gpu import CopyCounter
from test_dp_gpu import _free_port
from test_semantic_device_gpu import pinned_noise  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPOCHS, SEED = 3, 21


# ---- the two small setups -------------------------------------------------------------------------------------------------
class Geometry:
    """pn_transformer at small widths on 14 synthetic fractures: B = 4, P = 5, N = 64 -> 3 steps per epoch."""
    S, B, P, N = 14, 4, 5, 64

    def __init__(self):
        counts = [2, 5, 3, 4, 2, 3, 5, 4, 2, 3, 4, 5, 3, 2]
        self.store = MeshStore.from_arrays(synthetic.make_fracture_meshes(3, self.S, counts, 24), 2, self.P)
        self.val_store = MeshStore.from_arrays(synthetic.make_fracture_meshes(4, 5, [3, 2, 5, 4, 3], 24), 2, self.P)

    def cfg(self):
        cfg = config.pn_transformer_everyday()
        cfg.model.pc_feat_dim, cfg.model.transformer_heads = 64, 4
        cfg.model.transformer_feat_dim, cfg.model.transformer_layers = 128, 2
        cfg.data.max_num_part, cfg.data.num_pc_points = self.P, self.N
        cfg.exp.num_epochs, cfg.exp.batch_size = EPOCHS, self.B
        return cfg

    def producer(self, dev, store=None):
        return DeviceGeometryProducer(store or self.store, num_points=self.N, max_num_part=self.P, seed=SEED, device=dev)


class PartNet:
    """dgl with the device-side matching draws on 12 PartNet-like shapes: B = 3, P = 8, N = 128 -> 4 steps per epoch."""
    S, B, P, N = 12, 3, 8, 128

    def __init__(self):
        self.store = synthetic.make_partnet_like_store(self.S, max_parts=self.P, num_points=self.N, seed=9)

    def cfg(self):
        cfg = config.dgl_partnet_chair()
        cfg.loss.match_sample = "device"
        cfg.data.max_num_part, cfg.data.num_pc_points = self.P, self.N
        cfg.exp.num_epochs, cfg.exp.batch_size = EPOCHS, self.B
        return cfg

    def producer(self, dev, store=None):
        cfg = self.cfg()
        return DevicePartNetProducer(store or self.store, tuple(cfg.data.data_keys), max_num_part=self.P,
                                     num_part_category=cfg.data.num_part_category, device=dev)


@pytest.fixture(scope="module")
def geometry():
    return Geometry()


@pytest.fixture(scope="module")
def partnet():
    return PartNet()


def trainer_for(setup, dev, **kw):
    """A fresh trainer: the same initial weights and the same host generator states in every call."""
    import random
    torch.manual_seed(7), np.random.seed(7), random.seed(7)
    cfg = setup.cfg()
    return Trainer(build_model(cfg).to(dev), cfg, **kw)


def sampler_for(setup, dev, **kw):
    return EpochSampler(setup.S, setup.B, seed=SEED, device=dev, **kw)


def state_of(trainer):
    torch.cuda.synchronize()
    return [trainer.flat.flat_param.clone(), trainer.optimizer.exp_avg.clone(), trainer.optimizer.exp_avg_sq.clone()]


def assert_same_state(a, b):
    for name, x, y in zip(("parameters", "exp_avg", "exp_avg_sq"), a, b):
        assert torch.equal(x, y), name


def hand_loop(setup, dev, epochs=EPOCHS):
    """What a user writes without `fit`: host index lists from the restatement into the producer, one step each."""
    trainer, prod = trainer_for(setup, dev), setup.producer(dev)
    steps = setup.S // setup.B
    for epoch in range(epochs):
        trainer.set_epoch(epoch)
        order = sampler_ref.epoch_order(setup.S, SEED, epoch)
        for k in range(steps):
            trainer.train_step(prod.batch(order[k * setup.B:(k + 1) * setup.B].tolist()))
            trainer.check_health()
    return trainer


@pytest.fixture(scope="module")
def whole_runs(cuda_device, geometry, partnet):
    """The uninterrupted eager `fit` of both setups, run once and shared: (final state, history)."""
    runs = {}
    for name, setup in (("geometry", geometry), ("partnet", partnet)):
        trainer = trainer_for(setup, cuda_device)
        history = trainer.fit(setup.producer(cuda_device), sampler_for(setup, cuda_device), log_every=2)
        runs[name] = (state_of(trainer), history)
    return runs


# ---- 1. fit is the hand-written loop ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["geometry", "partnet"])
def test_fit_equals_the_hand_written_loop(cuda_device, geometry, partnet, whole_runs, name):
    setup = {"geometry": geometry, "partnet": partnet}[name]
    state, history = whole_runs[name]
    assert_same_state(state, state_of(hand_loop(setup, cuda_device)))
    cfg = setup.cfg()
    lr = cosine_warmup_lr(EPOCHS, int(EPOCHS * cfg.optimizer.warmup_ratio), cfg.optimizer.lr,
                          cfg.optimizer.lr / cfg.optimizer.lr_decay_factor)
    assert [h["epoch"] for h in history] == list(range(EPOCHS))
    assert [h["lr"] for h in history] == [lr(e) for e in range(EPOCHS)]
    assert all(np.isfinite(h["train/loss"]) and h["train/loss"] > 0 for h in history)


# ---- 2. captured equals eager -----------------------------------------------------------------------------------------------
def test_captured_fit_writing_into_the_static_batch_equals_eager(cuda_device, partnet, pinned_noise):  # noqa: F811
    eager = trainer_for(partnet, cuda_device)
    eager.fit(partnet.producer(cuda_device), sampler_for(partnet, cuda_device), log_every=0)
    graph = trainer_for(partnet, cuda_device, use_graph=True, graph_warmup=1)
    prod = partnet.producer(cuda_device)
    fed = []
    batch = prod.batch
    prod.batch = lambda idx, out=None: fed.append(out is not None) or batch(idx, out=out)
    graph.fit(prod, sampler_for(partnet, cuda_device), log_every=0)
    assert graph._graph is not None and fed == [False, False] + [True] * (EPOCHS * 4 - 2)
    assert_same_state(state_of(graph), state_of(eager))
    prod.check()


# ---- 3. resume ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,stop", [("geometry", 3), ("geometry", 4), ("partnet", 5)])
def test_resumed_run_equals_the_uninterrupted_run(cuda_device, geometry, partnet, whole_runs, tmp_path, name, stop):
    """`stop` steps (geometry: 3 = the end of epoch 0, 4 = inside epoch 1; partnet: 5 = inside epoch 1, with the regressor's
    noise drawn from the restored CPU generator), then everything built afresh, `resume`, and the rest of the run."""
    setup = {"geometry": geometry, "partnet": partnet}[name]
    want, want_history = whole_runs[name]
    steps = setup.S // setup.B
    first = trainer_for(setup, cuda_device)
    first.fit(setup.producer(cuda_device), sampler_for(setup, cuda_device), ckpt_dir=str(tmp_path), log_every=2,
              max_steps=stop)
    assert "last.pt" in os.listdir(tmp_path) and not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]
    del first
    fresh = trainer_for(setup, cuda_device)
    torch.manual_seed(12345)  # whatever the process drew meanwhile must not matter
    assert fresh.resume(str(tmp_path)) == stop // steps
    history = fresh.fit(setup.producer(cuda_device), EpochSampler(setup.S, setup.B, seed=0, device=cuda_device),
                        ckpt_dir=str(tmp_path), log_every=2)
    assert_same_state(state_of(fresh), want)
    assert [h["epoch"] for h in history] == list(range(EPOCHS))
    assert [h["lr"] for h in history] == [h["lr"] for h in want_history]
    assert [h["train/loss"] for h in history] == pytest.approx([h["train/loss"] for h in want_history], rel=1e-6)
    assert torch.load(tmp_path / "last.pt", weights_only=False)["fit"]["next_epoch"] == EPOCHS


# ---- 4. validation --------------------------------------------------------------------------------------------------------------
def test_validation_runs_on_its_epochs_and_leaves_the_run_alone(cuda_device, geometry, whole_runs):
    val = geometry.producer(cuda_device, geometry.val_store)
    passes = []

    def val_batches():
        passes.append(1)
        return [val.batch([0, 1, 2], batch_counter=0), val.batch([3, 4], batch_counter=1)]

    trainer = trainer_for(geometry, cuda_device)
    history = trainer.fit(geometry.producer(cuda_device), sampler_for(geometry, cuda_device), val_batches=val_batches,
                          val_every=2, log_every=2)
    assert len(passes) == 1 and ["val/part_acc" in h for h in history] == [False, True, False]
    assert 0.0 <= history[1]["val/part_acc"] <= 1.0
    assert_same_state(state_of(trainer), whole_runs["geometry"][0])


# ---- 5. the host reads the device once per log_every steps and once per epoch --------------------------------------------------
def test_fit_reads_the_device_once_per_log_interval_and_epoch(cuda_device, geometry, monkeypatch):
    trainer, prod = trainer_for(geometry, cuda_device), geometry.producer(cuda_device)
    sampler = sampler_for(geometry, cuda_device)
    trainer.fit(prod, sampler, epochs=1, log_every=0)  # (first launches: code objects, lazily built buffers)
    counter = CopyCounter(monkeypatch)
    history = trainer.fit(prod, sampler, epochs=EPOCHS, log_every=2)  # 3 steps per epoch: one log read + the epoch's read
    reads = counter.count
    monkeypatch.undo()
    assert len(history) == EPOCHS and all(h["train/loss"] > 0 for h in history)  # every epoch ran its steps
    assert EPOCHS <= reads <= EPOCHS * (3 // 2 + 1)


# ---- 6. two ranks ------------------------------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    setup = Geometry()
    trainer = trainer_for(setup, dev)
    prod = setup.producer(dev)
    sampler = EpochSampler(12, 3, seed=SEED, world=world, rank=rank, device=dev)  # 12 of the 14 shapes: no padding
    seen, batch = [], prod.batch
    prod.batch = lambda idx: seen.append((sampler.epoch, idx.tolist())) or batch(idx)
    trainer.fit(prod, sampler, epochs=2, log_every=0)
    torch.save({"param": trainer.flat.flat_param.cpu(), "seen": seen}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_stride_one_order_and_stay_in_lock_step(cuda_device):
    with tempfile.TemporaryDirectory() as out_dir:
        mp.spawn(_rank_worker, args=(2, _free_port(), out_dir), nprocs=2, join=True)
        got = [torch.load(os.path.join(out_dir, f"rank{r}.pt")) for r in range(2)]
    assert torch.equal(got[0]["param"], got[1]["param"])
    for epoch in range(2):
        shards = [[i for e, idx in got[r]["seen"] if e == epoch for i in idx] for r in range(2)]
        assert len(shards[0]) == len(shards[1]) == 6 and not set(shards[0]) & set(shards[1])
        for r in range(2):
            assert shards[r] == sampler_ref.epoch_order(12, SEED, epoch, 2, r).tolist()
        assert sorted(shards[0] + shards[1]) == list(range(12))  # together: the whole (here unpadded) order


# ---- 7. the tool ------------------------------------------------------------------------------------------------------------------
def test_train_tool_runs_on_synthetic_data_and_resumes(cuda_device, tmp_path):
    base = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "train.py"), "--synthetic", "--preset",
            "pn_transformer_everyday", "--synthetic-shapes", "16", "--batch-size", "8", "--ckpt-dir", str(tmp_path),
            "--log-every", "1"]
    first = subprocess.run(base + ["--epochs", "2"], capture_output=True, text=True)
    assert first.returncode == 0, first.stdout + first.stderr
    assert "epoch: 1" in first.stdout and "done: 2 epochs" in first.stdout
    assert sorted(os.listdir(tmp_path)) == ["last.pt", "model-epoch=000.pt", "model-epoch=001.pt"]
    assert torch.load(tmp_path / "last.pt", weights_only=False)["fit"]["next_epoch"] == 2
    second = subprocess.run(base + ["--epochs", "3", "--resume"], capture_output=True, text=True)
    assert second.returncode == 0, second.stdout + second.stderr
    assert "resuming at epoch 2" in second.stdout and "epoch: 2" in second.stdout and "epoch: 0" not in second.stdout
    assert torch.load(tmp_path / "last.pt", weights_only=False)["fit"]["next_epoch"] == 3
