"""numpy restatement of `mpa_epoch_order` (include/mpa_hip.h): the Philox keys, the stable argsort and the
`DistributedSampler` sharding.  It is the oracle of the device kernel and what `EpochSampler(device="cpu")` runs, so that
CPU tests and host-fed producers follow the order the device draws.  Imports nothing but numpy (and `philox_ref`, which
does the same)."""
from __future__ import annotations

import numpy as np

from .philox_ref import philox4x32_10

ORDER_TAG = 0x65700000   # counter word 1 of the epoch order (csrc/epoch_order.hip)
MAX_SHAPES = 1 << 18     # the kernel's cap on S


def epoch_keys(num_shapes, seed, epoch):
    """key_i uint64 [S]: x | (y << 32) of the block with key = the two words of `seed` and counter = (i, ORDER_TAG,
    epoch low word, epoch high word)."""
    seed, epoch = int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFFFFFFFFFF
    i = np.arange(int(num_shapes), dtype=np.uint64)
    x, y, _, _ = philox4x32_10(i, ORDER_TAG, epoch & 0xFFFFFFFF, epoch >> 32, seed & 0xFFFFFFFF, seed >> 32)
    return x | (y << np.uint64(32))


def epoch_permutation(num_shapes, seed, epoch):
    """0..S-1 sorted ascending by (key_i, i), int64 [S]."""
    return np.argsort(epoch_keys(num_shapes, seed, epoch), kind="stable").astype(np.int64)


def shard(order, world=1, rank=0):
    """`DistributedSampler(drop_last=False)` on an order: pad to a multiple of `world` by wrapping around, then every
    world-th entry from `rank` on; int64 [ceil(S / world)]."""
    order = np.asarray(order, dtype=np.int64).reshape(-1)
    S, world, rank = len(order), int(world), int(rank)
    if S < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"shard: S={S}, world={world}, rank={rank}")
    total = -(-S // world) * world
    return order[np.arange(rank, total, world) % S]


def epoch_order(num_shapes, seed=0, epoch=0, world=1, rank=0, shuffle=True):
    """What `mpa_epoch_order` writes for rank `rank` (shuffle=False: the same padding and striding of arange)."""
    S = int(num_shapes)
    if S < 1:
        raise ValueError(f"epoch_order: S={S} must be positive")
    return shard(epoch_permutation(S, seed, epoch) if shuffle else np.arange(S, dtype=np.int64), world, rank)
