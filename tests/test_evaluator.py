"""The evaluation pass and the checkpoint round trip on the host (no GPU): `Evaluator.run` against `aggregate_eval`, what
a run must leave untouched, two gloo ranks against one process, `Trainer.load_state_dict`, and the category table.
The models' own `validation_step` needs the HIP operators (there is no CPU Chamfer), so a small stand-in model with the
same contract runs here; the real models are evaluated in tests/test_evaluator_gpu.py, where the continued training run
after a checkpoint round trip is checked too (the fused optimiser only steps on the GPU)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from multi_part_assembly_amd import config
from multi_part_assembly_amd.base_model import BaseModel
from multi_part_assembly_amd.evaluate import PAPER_METRICS, Evaluator, evaluate_categories, format_table
from multi_part_assembly_amd.trainer import Trainer
from tool_loader import load_tool


class Stub(nn.Module):
    """`validation_step` contract of BaseModel on library operators, with BatchNorm and dropout inside."""

    def __init__(self):
        super().__init__()
        self.encoder = nn.Sequential(nn.Linear(3, 8), nn.BatchNorm1d(8), nn.ReLU(), nn.Dropout(0.5))
        self.head = nn.Linear(8, 2)
        self.frozen = nn.BatchNorm1d(2)
        self.seen_fused = []

    def validation_step(self, batch, batch_idx=0):
        self.seen_fused.append((getattr(self, "fused_metrics", None), self.training, torch.is_grad_enabled()))
        y = self.frozen(self.head(self.encoder(batch["x"])))
        return {"trans_loss": y[:, 0].abs().mean(), "part_acc": (y[:, 1] > 0).float().mean(), "loss": y.square().mean(),
                "batch_size": batch["x"].shape[0]}

    aggregate_eval = staticmethod(BaseModel.aggregate_eval)


def _batches():
    g = torch.Generator().manual_seed(11)
    return [{"x": torch.randn(n, 3, generator=g)} for n in (8, 5, 3)]  # unequal sizes, ragged last batch


def _model(seed=3):
    torch.manual_seed(seed)
    m = Stub()
    with torch.no_grad():  # non-trivial running statistics
        m.encoder[1].running_mean.normal_()
        m.encoder[1].running_var.uniform_(0.5, 2.0)
    return m


def test_run_equals_aggregate_eval_and_leaves_the_model_alone():
    model = _model()
    model.train()
    model.frozen.eval()  # a sub-module the user keeps in eval mode must get THAT mode back
    batches = _batches()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    rng = torch.get_rng_state()
    got = Evaluator(model).run(batches, prefix="val")
    assert torch.equal(torch.get_rng_state(), rng)  # the CPU generator is not consumed
    assert model.training and model.encoder.training and not model.frozen.training
    assert "fused_metrics" not in vars(model)
    assert model.seen_fused == [(True, False, False)] * 3  # fused metrics on, eval mode, no_grad — for every batch
    for k, v in model.state_dict().items():  # running statistics and num_batches_tracked included
        assert torch.equal(v, state[k]), k
    model.eval()
    with torch.no_grad():
        want = model.aggregate_eval([model.validation_step(b, i) for i, b in enumerate(batches)], prefix="val")
    assert set(got) == set(want) == {"val/trans_loss", "val/part_acc", "val/loss"}
    for k in want:
        assert isinstance(got[k], float)
        np.testing.assert_allclose(got[k], float(want[k]), rtol=1e-6, err_msg=k)
    assert Evaluator(model, fused_metrics=False).run(batches[:1], prefix="test").keys() == {"test/trans_loss", "test/part_acc",
                                                                                          "test/loss"}
    assert model.seen_fused[-1][0] is False
    with pytest.raises(RuntimeError, match="no batches"):
        Evaluator(model).run([])


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model = _model()
    shard = _batches()[rank::world]  # rank 0: batches 0 and 2, rank 1: batch 1
    res = Evaluator(model, process_group=dist.group.WORLD).run(shard)
    torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_two_rank_gloo_evaluation_equals_one_process(tmp_path):
    """Each rank evaluates its shard; sums and sizes are all-reduced.  The all-reduce reorders a sum of three fp32-sized
    terms, hence 1e-6 relative."""
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    outs = [torch.load(tmp_path / f"rank{r}.pt") for r in range(2)]
    assert outs[0] == outs[1]
    want = Evaluator(_model()).run(_batches())
    assert set(outs[0]) == set(want)
    for k in want:
        np.testing.assert_allclose(outs[0][k], want[k], rtol=1e-6, err_msg=k)


# ---- Trainer.state_dict / load_state_dict ------------------------------------------------------------------------------------
def _trainer(seed):
    torch.manual_seed(seed)
    return Trainer(Stub(), config.pn_transformer_everyday())


def test_trainer_state_round_trip_on_the_host():
    a = _trainer(1)
    with torch.no_grad():  # a trained state: moved weights and statistics, moments, step count, epoch
        a.flat.flat_param.add_(0.25)
        a.model.encoder[1].running_mean.add_(1.5)
        a.model.encoder[1].num_batches_tracked.add_(7)
        a.optimizer.exp_avg.uniform_(-1, 1)
        a.optimizer.exp_avg_sq.uniform_(0, 1)
    a.optimizer.step_count = 41
    a.set_epoch(30)
    state = a.state_dict()
    assert set(state) >= {"model", "optimizer", "epoch"}
    b = _trainer(2)
    assert not torch.equal(b.flat.params[0], a.flat.params[0])
    b.load_state_dict(state)
    for p, q in zip(a.flat.params, b.flat.params):  # (the alignment gaps of the flat buffer belong to no parameter)
        assert torch.equal(p, q)
    for p, off in zip(b.flat.params, b.flat.offsets):  # the parameters are still views of the flat buffer
        assert p.data_ptr() == b.flat.flat_param[off:].data_ptr()
    for (k, v), (_, w) in zip(sorted(a.model.state_dict().items()), sorted(b.model.state_dict().items())):
        assert torch.equal(v, w), k
    assert torch.equal(b.optimizer.exp_avg, a.optimizer.exp_avg) and torch.equal(b.optimizer.exp_avg_sq, a.optimizer.exp_avg_sq)
    assert b.optimizer.step_count == 41 and b.epoch == 30
    assert b.optimizer.lr == a.optimizer.lr == a.schedule(30) != a.schedule(0)


def test_trainer_accepts_a_lightning_style_checkpoint():
    a, b = _trainer(1), _trainer(2)
    with torch.no_grad():
        b.optimizer.exp_avg.fill_(0.5)
    b.optimizer.step_count = 9
    b.load_state_dict({"state_dict": a.model.state_dict(), "epoch": 123, "global_step": 4567})
    assert all(torch.equal(p, q) for p, q in zip(a.flat.params, b.flat.params))
    assert b.optimizer.step_count == 9 and b.epoch == 0 and float(b.optimizer.exp_avg[0]) == 0.5  # weights only


def test_state_dict_refuses_after_a_reported_failure(monkeypatch):
    """`raise_if_failed` clears the status word as it reports, so a caller that caught the error could
    still checkpoint the parameters behind the failed launch.  The trainer remembers."""
    from multi_part_assembly_amd import trainer as trainer_mod
    t = _trainer(1)
    good = t.state_dict()
    calls = []

    def failing(device=None, synchronize=False):
        calls.append(synchronize)
        raise RuntimeError("gru: a launch of csrc/gru.hip gave up")

    monkeypatch.setattr(trainer_mod._gru, "raise_if_failed", failing)
    with pytest.raises(RuntimeError, match="gave up"):
        t.check_health()
    monkeypatch.undo()  # the status word reads clean again ...
    t.check_health()
    with pytest.raises(RuntimeError, match="earlier check_health"):  # ... the trainer does not
        t.state_dict()
    t.load_state_dict(good)
    assert set(t.state_dict()) == set(good)


# ---- the category table ---------------------------------------------------------------------------------------------------------
class _StubEvaluator:
    def __init__(self, table):
        self.table, self.calls = table, []

    def run(self, batches, prefix="val"):
        self.calls.append((batches, prefix))
        return {f"{prefix}/{k}": v for k, v in self.table[batches].items()}


def test_evaluate_categories_scales_rounds_and_averages():
    table = {"Bottle": {"rot_rmse": 80.149, "rot_mae": 68.0, "trans_rmse": 0.15049, "trans_mae": 0.1212,
                        "transform_pt_cd_loss": 0.014849, "part_acc": 0.2474, "loss": 3.0},
             "Mug": {"rot_rmse": 79.71, "rot_mae": 67.31, "trans_rmse": 0.1611, "trans_mae": 0.1299,
                     "transform_pt_cd_loss": 0.0204, "part_acc": 0.301, "loss": 2.0}}
    ev = _StubEvaluator(table)
    res = evaluate_categories(ev, lambda cat: cat, ["Bottle", "Mug"])
    assert ev.calls == [("Bottle", "test"), ("Mug", "test")]
    assert res["categories"] == ["Bottle", "Mug"] and list(res["metrics"]) == list(PAPER_METRICS)
    m = res["metrics"]
    assert m["rot_rmse"] == {"values": [80.1, 79.7], "mean": 79.9}  # the mean of the ROUNDED values, rounded again
    assert m["trans_rmse"]["values"] == [15.0, 16.1] and m["trans_mae"]["values"] == [12.1, 13.0]
    assert m["transform_pt_cd_loss"] == {"values": [14.8, 20.4], "mean": 17.6}
    assert m["part_acc"] == {"values": [24.7, 30.1], "mean": 27.4}
    text = format_table(res)
    assert "part_acc:\n24.7 & 30.1 & 27.4" in text and text.splitlines()[0] == "categories: Bottle & Mug & mean"
    # a semantic model reports neither rot_* nor trans_*: those rows are left out
    sem = {"Chair": {"part_acc": 0.5, "transform_pt_cd_loss": 0.01, "connectivity_acc": 0.4}}
    res = evaluate_categories(_StubEvaluator(sem), lambda cat: cat, ["Chair"])
    assert list(res["metrics"]) == ["transform_pt_cd_loss", "part_acc"]


# ---- tools/evaluate.py: the data list -----------------------------------------------------------------------------
_TETRA = "v 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 0 1\nf 1 2 3\nf 1 2 4\nf 1 3 4\nf 2 3 4\n"


def _fracture_tree(root):
    """A Breaking-Bad-like tree: shape folders holding fracture folders holding one .obj per part."""
    layout = {"everyday/Bottle/s1": {"fractured_0": 2, "fractured_1": 3, "mode_0": 5, "redundant": 2},
              "everyday/Cup/s2": {"fractured_0": 1, "mode_3": 2}}
    for shape, fracs in layout.items():
        for frac, parts in fracs.items():
            os.makedirs(os.path.join(root, shape, frac))
            for k in range(parts):
                with open(os.path.join(root, shape, frac, f"piece_{k}.obj"), "w") as fh:
                    fh.write(_TETRA)
    with open(os.path.join(root, "everyday.val.txt"), "w") as fh:
        fh.write("everyday/Bottle/s1\neveryday/Cup/s2\neveryday/Cup/missing\n")


def test_data_list_expands_shape_folders_and_skips_part_counts_out_of_range(tmp_path):
    """The split files name SHAPE folders; their `fractured_*` / `mode_*` sub-folders are the samples, and a fracture with
    too few or too many parts is skipped without an error (reference geometry_data.py:48-71)."""
    from multi_part_assembly_amd import datasets
    root = str(tmp_path)
    _fracture_tree(root)
    got = datasets.read_fracture_list(root, "everyday.val.txt", "", 2, 4)
    assert sorted(got) == ["everyday/Bottle/s1/fractured_0", "everyday/Bottle/s1/fractured_1", "everyday/Cup/s2/mode_3"]
    assert sorted(datasets.read_fracture_list(root, "everyday.val.txt", "all", 2, 20)) == sorted(got + ["everyday/Bottle/s1/mode_0"])
    assert datasets.read_fracture_list(root, "everyday.val.txt", "Cup", 1, 20) != []
    assert sorted(datasets.read_fracture_list(root, "everyday.val.txt", "Cup", 1, 1)) == ["everyday/Cup/s2/fractured_0"]
    assert datasets.read_fracture_list(root, "everyday.val.txt", "Bott", 2, 20) == []  # a whole path component, not a prefix

    tool = load_tool("evaluate")
    args = type("Args", (), {"data_dir": root, "data_fn": "everyday.val.txt"})()
    cfg = config.pn_transformer_everyday()
    cfg.data.min_num_part, cfg.data.max_num_part = 2, 4
    store = tool.mesh_store(cfg, args, "")
    assert store.num_shapes == 3 and store.num_parts == 2 + 3 + 2 and len(store.tri) == 4 * store.num_parts
    store = tool.mesh_store(cfg, args, "Bottle")
    assert store.num_shapes == 2 and sorted(np.diff(store.shape_part_off).tolist()) == [2, 3]
    cfg.data.min_num_part, cfg.data.max_num_part = 6, 20
    with pytest.raises(ValueError, match="no fracture"):
        tool.mesh_store(cfg, args, "Cup")


def test_a_run_without_a_process_group_stays_local(monkeypatch):
    """`Evaluator(model)` inside an initialised multi-rank job must not start a collective the other ranks never join."""
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)

    def boom(*a, **k):
        raise AssertionError("all_reduce called without a process group")
    monkeypatch.setattr(dist, "all_reduce", boom)
    want = Evaluator(_model()).run(_batches())
    assert set(want) == {"val/trans_loss", "val/part_acc", "val/loss"}
