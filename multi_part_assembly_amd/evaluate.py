"""The evaluation pass: `validation_step` over a loader, the reference's batch-size-weighted average behind it
(`validation_epoch_end` / `test_epoch_end`, models/modules/base_model.py:69-111), and the per-category table of its
test script (scripts/test.py:16-66) — without Lightning.

`Evaluator.run` issues no host synchronisation per batch: every batch's values are stacked and added, weighted by the
batch size, into one float64 device vector whose last element collects the sizes; one health check, one device-to-host
copy and the division come at the end.  With a process group every rank runs its own shard of the loader and the vector
is all-reduced (only then: without one a run is local to its process, also inside a multi-rank job), which gives the result of one process over the union of the shards (the reference tests with DP for the
same reason: DDP's sampler would duplicate samples, scripts/test.py:24-25).

An evaluation leaves the training state alone: the modules run in eval mode under `no_grad` (BatchNorm statistics and
`num_batches_tracked` untouched, dropout off — so the dropout-seed streams of training are not advanced), no optimiser is
involved, and every module gets its previous mode back.  Semantic models draw their matching sub-samples from the CPU
generator exactly as the reference's evaluation does; nothing else consumes it.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.distributed as dist

from . import gru as _gru

# scripts/test.py:37-44: metric -> factor it is presented with in the paper's tables
PAPER_METRICS = {
    "rot_rmse": 1.0,
    "rot_mae": 1.0,
    "trans_rmse": 100.0,            # x 1e-2
    "trans_mae": 100.0,             # x 1e-2
    "transform_pt_cd_loss": 1000.0,  # x 1e-3
    "part_acc": 100.0,              # %
}
# the column `evaluate_categories(..., connectivity=True)` adds behind them when the runs report it (batches that carry a
# contact table: `contacts.contact_points`, the data key "contact_points")
CONNECTIVITY_METRIC = {"connectivity_acc": 100.0}  # %


class Evaluator:
    def __init__(self, model, process_group=None, fused_metrics=True, health=None):
        """`process_group`: every rank of it must call `run`, each on its own shard; None = no reduction.
        `fused_metrics`: value of `model.fused_metrics` during a run (csrc/eval_metrics.hip instead of the per-function
        composition).  `health`: called once at the end of a run instead of `gru.raise_if_failed` (a Trainer passes its
        own `check_health`, which also remembers a failure)."""
        self.model, self.group, self.fused_metrics, self.health = model, process_group, fused_metrics, health

    def _check_health(self, device):
        if self.health is not None:
            self.health()
        elif device.type == "cuda":
            _gru.raise_if_failed(device, synchronize=True)

    @torch.no_grad()
    def run(self, batches, prefix="val"):
        """{f"{prefix}/{key}": float} over every batch of `batches` (any batch sizes; a ragged last batch is fine)."""
        model = self.model
        modes = [(m, m.training) for m in model.modules()]
        had_attr = "fused_metrics" in vars(model)
        prev_fused = getattr(model, "fused_metrics", False)
        model.eval()
        model.fused_metrics = self.fused_metrics
        keys, acc = None, None
        try:
            for i, batch in enumerate(batches):
                res = model.validation_step(batch, i)
                size = res["batch_size"]
                ks = [k for k in res if k != "batch_size"]
                if keys is None:
                    keys = ks
                elif ks != keys:
                    raise RuntimeError(f"Evaluator: batch {i} returned the keys {ks}, the first batch {keys}")
                vals = torch.stack([torch.as_tensor(res[k]).detach().reshape(()) for k in keys]).double()
                dev = vals.device
                if torch.is_tensor(size):  # (a data-parallel step reports its sizes as a tensor)
                    w = size.detach().double().sum().reshape(1).to(dev)
                else:
                    w = torch.full((1,), float(size), dtype=torch.float64, device=dev)
                term = torch.cat([vals * w, w])
                acc = term if acc is None else acc.add_(term)
        finally:
            for m, mode in modes:
                m.training = mode
            if had_attr:
                model.fused_metrics = prev_fused
            else:
                del model.fused_metrics
        if acc is None:
            raise RuntimeError("Evaluator: no batches (every rank of a process group needs at least one)")
        if self.group is not None:
            dist.all_reduce(acc, group=self.group)
        self._check_health(acc.device)
        host = acc.cpu()  # the pass's one device-to-host copy
        total = host[-1]
        return {f"{prefix}/{k}": float(host[i] / total) for i, k in enumerate(keys)}


def evaluate_categories(evaluator, batches_for, categories, metrics=None, prefix="test", connectivity=False):
    """The per-category loop of scripts/test.py:45-58: one `evaluator.run(batches_for(category))` per category, each paper
    metric scaled and rounded to one decimal, plus the mean over the categories (of the rounded values, rounded again —
    as the reference prints it).  Metrics a model does not report (rot_* / trans_* on semantic data) are left out.
    `connectivity` adds the connectivity accuracy (%) behind the paper's metrics — a column only when the runs report it.
    Returns {"categories": [...], "metrics": {name: {"values": [per category], "mean": float}}}."""
    metrics = PAPER_METRICS if metrics is None else metrics
    if connectivity:
        metrics = {**metrics, **CONNECTIVITY_METRIC}
    categories = list(categories)
    rows = {m: [] for m in metrics}
    for cat in categories:
        res = evaluator.run(batches_for(cat), prefix=prefix)
        for m in list(rows):
            key = f"{prefix}/{m}"
            if key not in res:
                if rows[m]:
                    raise RuntimeError(f"evaluate_categories: {cat} does not report {m}, earlier categories did")
                del rows[m]
                continue
            rows[m].append(res[key] * metrics[m])
    out = {}
    for m, vals in rows.items():
        vals = np.array(vals, dtype=np.float64).round(1)
        out[m] = {"values": vals.tolist(), "mean": float(np.mean(vals).round(1))}
    return {"categories": categories, "metrics": out}


def format_table(results):
    """The test script's LaTeX rows: `metric:` then the per-category values and their mean joined by ` & `."""
    lines = ["categories: " + " & ".join(results["categories"] + ["mean"])]
    for m, row in results["metrics"].items():
        lines.append(f"{m}:")
        lines.append(" & ".join(str(v) for v in row["values"] + [row["mean"]]))
    return "\n".join(lines)
