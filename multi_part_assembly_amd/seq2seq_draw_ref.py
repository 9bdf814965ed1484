"""numpy restatement of `mpa_seq2seq_draw` (include/mpa_hip.h): the teacher-forcing coin, the decoder noise and the
LockedDropout mask of one B-LSTM forward, from Philox4x32-10 blocks.  This file is the specification the kernel
(csrc/seq2seq_draw.hip) is tested against.  Philox runs on plain integers (numpy uint64 arrays holding 32-bit words); the
coin and the mask are integer comparisons, the normals are evaluated in float64.  Imports nothing but numpy (and
`philox_ref`, which does the same)."""
from __future__ import annotations

import numpy as np

from .philox_ref import philox4x32_10

TAG = 0x73320000          # counter word 1 = TAG | kind (csrc/seq2seq_draw.hip); the taken values: include/mpa_hip.h
KIND_TEACHER, KIND_NOISE, KIND_MASK = 0, 1, 2
NOISE_DIM = 16            # noise channels of the decoder's initial state
CHANNELS = 128            # decoder input width: the mask's channels
MAX_BATCH, MAX_STEPS = 64, 4096
_U64 = 0xFFFFFFFFFFFFFFFF


def step_value(counter=0, salt=0):
    """c = counter + salt as an unsigned 64-bit number (wraps around)."""
    return (int(counter) + int(salt)) & _U64


def words(kind, blocks, seed=0, counter=0, salt=0):
    """uint64 [blocks, 4]: the output words of the blocks i = 0 .. blocks - 1 of `kind`."""
    seed, c = int(seed) & _U64, step_value(counter, salt)
    i = np.arange(int(blocks), dtype=np.uint64)
    return np.stack(philox4x32_10(i, TAG | kind, c & 0xFFFFFFFF, c >> 32, seed & 0xFFFFFFFF, seed >> 32), axis=1)


def _threshold24(x):
    """The smallest integer k with float(k) * 2^-24 >= x for a float32 x: `u < x` is `k < threshold`, `u >= x` is
    `k >= threshold` for the 24-bit integer k behind u (the product below is exact in float64)."""
    return int(np.ceil(np.float64(np.float32(x)) * 16777216.0))


def teacher(ratio, seed=0, counter=0, salt=0):
    """int32 [1]: 1 = teacher forcing.  u = (w >> 8) * 2^-24 < float32(ratio), as an integer comparison."""
    w = int(words(KIND_TEACHER, 1, seed, counter, salt)[0, 0])
    return np.array([1 if (w >> 8) < _threshold24(ratio) else 0], dtype=np.int32)


def noise_uniforms(B, seed=0, counter=0, salt=0):
    """(u1, u2) float64 [B * 8] each, exact: pair j comes from words (0, 1) (j even) or (2, 3) (j odd) of block j // 2
    and gives the flat noise elements 2 j (cosine) and 2 j + 1 (sine)."""
    w = words(KIND_NOISE, int(B) * NOISE_DIM // 4, seed, counter, salt).reshape(-1, 2)
    u1 = ((w[:, 0] >> np.uint64(9)).astype(np.float64) + 0.5) / 8388608.0
    u2 = (w[:, 1] >> np.uint64(8)).astype(np.float64) / 16777216.0
    return u1, u2


def box_muller(u1, u2, dtype=np.float64):
    """[len(u1), 2]: (r cos a, r sin a), r = sqrt(-2 log u1), a = 2 pi u2, every operation in `dtype` (float32: the
    kernel's formulas with numpy's functions, the yardstick of the kernel's own rounding error)."""
    u1, u2 = np.asarray(u1).astype(dtype), np.asarray(u2).astype(dtype)
    r = np.sqrt(dtype(-2.0) * np.log(u1))
    a = dtype(2.0 * np.pi) * u2
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=1).astype(dtype)


def noise(B, seed=0, counter=0, salt=0, dtype=np.float64):
    """[B, 16] standard normals in `dtype` (float64: the reference values)."""
    return box_muller(*noise_uniforms(B, seed, counter, salt), dtype=dtype).reshape(int(B), NOISE_DIM)


def mask(T, B, p, seed=0, counter=0, salt=0):
    """float32 [T, B, 128]: element e = word e % 4 of block e // 4; kept (1 / (1 - p), rounded once in float32) where
    u = (w >> 8) * 2^-24 >= float32(p), else 0."""
    n = int(T) * int(B) * CHANNELS
    w = words(KIND_MASK, n // 4, seed, counter, salt).reshape(-1)
    keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    out = np.where((w >> np.uint64(8)) >= np.uint64(_threshold24(p)), keep, np.float32(0.0)).astype(np.float32)
    return out.reshape(int(T), int(B), CHANNELS)


def check_args(B, T, p):
    """The kernel's refusals (MPA_EINVAL there, ValueError here)."""
    if not 1 <= int(B) <= MAX_BATCH:
        raise ValueError(f"seq2seq_draw: B={B} outside [1, {MAX_BATCH}]")
    if not 1 <= int(T) <= MAX_STEPS:
        raise ValueError(f"seq2seq_draw: T={T} outside [1, {MAX_STEPS}]")
    if not 0.0 <= float(np.float32(p)) < 1.0:
        raise ValueError(f"seq2seq_draw: p={p} outside [0, 1)")


def draw(B, T, p, ratio, training, seed=0, counter=0, salt=0):
    """(noise float64 [B, 16], teacher int32 [1], mask float32 [T, B, 128] or None outside training): one launch."""
    check_args(B, T, p)
    return (noise(B, seed, counter, salt), teacher(ratio, seed, counter, salt),
            mask(T, B, p, seed, counter, salt) if training else None)
