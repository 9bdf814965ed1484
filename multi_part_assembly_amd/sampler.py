"""`EpochSampler`: the index batches of an epoch — `DistributedSampler` + `BatchSampler` of the reference's loaders
(multi_part_assembly/datasets/geometry_data.py:226-248) with the order drawn and sharded on the device.

`set_epoch(e)` is one call of `mpa_epoch_order` (csrc/epoch_order.hip) into a device vector this sampler owns; iterating
yields int64 views of that vector, which `DevicePartNetProducer.batch` and `DeviceGeometryProducer.batch` take as they
are: no copy, no host synchronisation, no Python index list.  Every rank computes the same permutation from
`(seed, epoch)` and keeps its own stride of it, so ranks need not talk to each other.  On `device="cpu"` the order comes
from `sampler_ref`, the numpy restatement the kernel is tested against bit for bit, so a host-fed producer or a CPU test
sees the batches the device would."""
from __future__ import annotations

import torch

from . import _lib, sampler_ref


class EpochSampler:
    def __init__(self, num_shapes, batch_size, seed=0, world=1, rank=0, shuffle=True, drop_last=True, device="cuda"):
        self.num_shapes, self.batch_size = int(num_shapes), int(batch_size)
        self.world, self.rank = int(world), int(rank)
        if self.num_shapes < 1 or self.batch_size < 1:
            raise ValueError(f"EpochSampler: num_shapes={num_shapes} and batch_size={batch_size} must be positive")
        if self.world < 1 or not 0 <= self.rank < self.world:
            raise ValueError(f"EpochSampler: rank={rank} outside [0, world={world})")
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.shuffle, self.drop_last = bool(shuffle), bool(drop_last)
        self.device = torch.device(device)
        if self.shuffle and self.device.type == "cuda" and self.num_shapes > sampler_ref.MAX_SHAPES:
            raise ValueError(f"EpochSampler: num_shapes={num_shapes} above the {sampler_ref.MAX_SHAPES} shapes "
                             "mpa_epoch_order sorts")
        self.shard_len = -(-self.num_shapes // self.world)  # total / world
        self.epoch, self.next_step = 0, 0
        self._order, self._workspace, self._drawn = None, None, None

    def __len__(self):
        """Steps per epoch on this rank."""
        full = self.shard_len // self.batch_size
        return full if self.drop_last or self.shard_len % self.batch_size == 0 else full + 1

    @property
    def order(self):
        """This rank's index vector of the current epoch, int64 [total / world] on `device` (drawn on first use)."""
        if self._drawn != self.epoch:
            self._draw()
        return self._order

    def _draw(self):
        if not self.shuffle:  # arange with the same padding and striding: the same vector in every epoch, no kernel
            if self._order is None:
                host = sampler_ref.epoch_order(self.num_shapes, world=self.world, rank=self.rank, shuffle=False)
                self._order = torch.from_numpy(host).to(self.device)
        elif self.device.type != "cuda":
            host = sampler_ref.epoch_order(self.num_shapes, self.seed, self.epoch, self.world, self.rank)
            self._order = torch.from_numpy(host)
        else:
            with torch.cuda.device(self.device):
                if self._order is None:
                    self._order = torch.empty(self.shard_len, dtype=torch.int64, device=self.device)
                    nbytes = _lib.query("mpa_epoch_order_workspace", self.num_shapes)
                    self._workspace = torch.empty(nbytes // 8, dtype=torch.int64, device=self.device)
                _lib.launch("mpa_epoch_order", self.device, self.num_shapes, self.world, self.rank, self.seed,
                            self.epoch, None, self._workspace, self._order)
        self._drawn = self.epoch

    def set_epoch(self, epoch):
        """Draw the order of `epoch` (one launch) and start at its first batch."""
        self.epoch, self.next_step = int(epoch), 0
        self._draw()

    def batch_indices(self, step):
        """The index batch of step `step` of the current epoch: a view of `order`."""
        lo = step * self.batch_size
        return self.order[lo:min(lo + self.batch_size, self.shard_len)]

    def __iter__(self):
        """The remaining batches of the current epoch, from `next_step` on (0 after `set_epoch`)."""
        steps = len(self)
        while self.next_step < steps:
            step = self.next_step
            self.next_step = step + 1
            yield self.batch_indices(step)

    def state_dict(self):
        return {"seed": self.seed, "epoch": self.epoch, "next_step": self.next_step}

    def load_state_dict(self, state):
        """Continue where `state_dict()` was taken: the same epoch's order, from the step that came next."""
        self.seed = int(state["seed"]) & 0xFFFFFFFFFFFFFFFF
        self._drawn = None
        self.set_epoch(state["epoch"])
        self.next_step = int(state["next_step"])
