"""Host side of the device-drawn semantic step: a numpy restatement of `mpa_match_sample_indices` (the partial
Fisher-Yates shuffle on Philox4x32-10 words that include/mpa_hip.h fixes; tests/test_semantic_device_gpu.py uses it as the
oracle of the kernel), its uniformity, the models' shape with and without `cfg.loss.match_sample = "device"`, the ABI
surface of the new entry points and the PartNet presets.  Nothing here needs a GPU."""
import ctypes
import json
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

from multi_part_assembly_amd import _build, _lib, config, matching
from multi_part_assembly_amd.pn_transformer import build_model
from test_mesh_store import philox4x32_10_np

GOLDEN = Path(__file__).resolve().parent / "golden"
U64 = 0xFFFFFFFFFFFFFFFF
CAP = matching.MAX_POINTS  # N of the draw: 16384 (the permutation lives in LDS)
SHAPES = [(1000, 100), (100, 100), (64, 64), (101, 100), (CAP, 100)]


# ---- oracle restatement (shared with the GPU test) --------------------------------------------------------------------------
def restate_draw(slots, N, n, seed, counter, salt=0, first_slot=0):
    """[slots, n] int32: row s = the first n entries of the permutation of slot `first_slot + s` (= b * G + g), as
    include/mpa_hip.h states it — perm = iota(N); for k < n: j = k + mulhi32(w_k, N - k), swap perm[k] and perm[j], emit
    perm[k]; w_k = word k & 3 of Philox4x32-10 with key = the two words of `seed` and counter = (slot, 0x6D610000 | k >> 2,
    the two words of c), c = counter + salt mod 2^64.  Vectorised over the slots."""
    seed, c = int(seed) & U64, (int(counter) + int(salt)) & U64
    slot = np.arange(first_slot, first_slot + slots, dtype=np.uint64)
    words = np.empty((slots, 4 * ((n + 3) // 4)), dtype=np.uint64)
    for block in range((n + 3) // 4):
        r = philox4x32_10_np(slot, 0x6D610000 | block, c & 0xFFFFFFFF, c >> 32, seed & 0xFFFFFFFF, seed >> 32)
        for i in range(4):
            words[:, 4 * block + i] = r[i]
    perm = np.tile(np.arange(N, dtype=np.int32 if N > 32767 else np.int16), (slots, 1))
    rows = np.arange(slots)
    out = np.empty((slots, n), dtype=np.int32)
    for k in range(n):
        j = k + ((words[:, k] * np.uint64(N - k)) >> np.uint64(32)).astype(np.int64)  # 32 x 32 bits: fits in 64
        a, b = perm[rows, k].copy(), perm[rows, j].copy()
        perm[rows, j] = a
        perm[rows, k] = b
        out[:, k] = b
    return out


@pytest.mark.parametrize("N,n", SHAPES)
def test_restated_rows_are_prefixes_of_permutations(N, n):
    rows = restate_draw(12, N, n, seed=0x1234567890ABCDEF, counter=3, salt=matching.SALT_STEP)
    assert rows.shape == (12, n) and rows.min() >= 0 and rows.max() < N
    for r in rows:
        assert len(set(r.tolist())) == n
    if n == N:  # a whole permutation
        assert (np.sort(rows, axis=1) == np.arange(N)).all()
    # slots, counters, salts and seeds are separate streams; the same arguments give the same rows
    assert np.array_equal(rows, restate_draw(12, N, n, 0x1234567890ABCDEF, 3, matching.SALT_STEP))
    assert np.array_equal(rows[5:9], restate_draw(4, N, n, 0x1234567890ABCDEF, 3, matching.SALT_STEP, first_slot=5))
    for other in (restate_draw(12, N, n, 0x1234567890ABCDEF, 4, matching.SALT_STEP),
                  restate_draw(12, N, n, 0x1234567890ABCDEF, 3, 2 * matching.SALT_STEP),
                  restate_draw(12, N, n, 0x1234567890ABCDEE, 3, matching.SALT_STEP)):
        assert not (rows == other).all(axis=1).any()
    assert len({tuple(r) for r in rows.tolist()}) == 12


def test_restatement_follows_the_documented_layout_word_for_word():
    """One row by hand, from the scalar Philox of tests/test_mesh_store.py: pins the counter / key layout independently of
    the vectorised restatement above."""
    from test_mesh_store import philox4x32_10
    seed, counter, salt, slot, N, n = 0xDEADBEEF00C0FFEE, (1 << 32) + 5, 7 * matching.SALT_STEP, 9, 101, 10
    c = (counter + salt) & U64
    perm, want = list(range(N)), []
    for k in range(n):
        w = philox4x32_10([slot, 0x6D610000 | (k >> 2), c & 0xFFFFFFFF, c >> 32], [seed & 0xFFFFFFFF, seed >> 32])[k & 3]
        j = k + ((w * (N - k)) >> 32)
        perm[k], perm[j] = perm[j], perm[k]
        want.append(perm[k])
    assert restate_draw(1, N, n, seed, counter, salt, first_slot=slot)[0].tolist() == want


def test_draw_is_uniform():
    """N = 200, n = 100, 64 slots x 2000 counters = R = 128000 rows (fixed inputs: a deterministic result).
    Position 0 is one of N values with equal probability: Pearson's statistic of its histogram is chi-square with N - 1
    degrees of freedom.  Inclusion: a row holds index i with probability p = n / N; rows are independent, and inside a row
    (a sample without replacement) two indicators have covariance -p (1 - p) / (N - 1), so the counts O have covariance
    R p (1 - p) N / (N - 1) (I - J / N) and (N - 1) / N * sum_i (O_i - R p)^2 / (R p (1 - p)) is chi-square with N - 1
    degrees of freedom as well.  Both are held against the quantile at 1 - 1e-6."""
    from scipy.stats import chi2
    N, n, slots, counters = 200, 100, 64, 2000
    first = np.zeros(N, dtype=np.int64)
    included = np.zeros(N, dtype=np.int64)
    for lo in range(0, counters, 500):  # 500 counters at a time bound the working set
        for counter in range(lo, lo + 500):
            rows = restate_draw(slots, N, n, seed=20240613, counter=counter)
            first += np.bincount(rows[:, 0], minlength=N)
            included += np.bincount(rows.reshape(-1), minlength=N)
    R = slots * counters
    p = n / N
    bound = chi2.ppf(1.0 - 1e-6, N - 1)
    stat_first = float(((first - R / N) ** 2 / (R / N)).sum())
    stat_incl = float((N - 1) / N * ((included - R * p) ** 2 / (R * p * (1 - p))).sum())
    print(f"chi-square, {N - 1} degrees of freedom: position 0 {stat_first:.1f}, inclusion {stat_incl:.1f}, bound {bound:.1f}")
    assert first.sum() == R and included.sum() == R * n
    assert stat_first < bound and stat_incl < bound


# ---- model shape --------------------------------------------------------------------------------------------------------
def _module_names(model):
    return [name for name, _ in model.named_modules()]


@pytest.mark.parametrize("preset", ["global_partnet_chair", "lstm_partnet_chair"])
def test_default_config_builds_the_model_of_the_parent_commit(preset):
    """`match_sample` defaults to "host": no sampler module, the recorded `state_dict` keys (those of the reference)."""
    cfg = getattr(config, preset)()
    assert "match_sample" not in cfg.loss
    model = build_model(cfg)
    assert model.match_sample == "host" and not hasattr(model, "match_sampler")
    assert not any("match_sampler" in n for n in _module_names(model))
    want = set(json.loads((GOLDEN / "state_dict_keys.json").read_text())["state_dict_keys"][preset])
    got = {k for k in model.state_dict() if not (k.endswith(".num_batches_tracked") and k not in want)}
    assert got == want


def test_device_mode_adds_no_state_and_lets_the_trainer_capture():
    from multi_part_assembly_amd.trainer import Trainer
    base = build_model(config.global_partnet_chair())
    cfg = config.global_partnet_chair()
    cfg.loss.match_sample = "device"
    model = build_model(cfg)
    assert list(model.state_dict().keys()) == list(base.state_dict().keys())
    assert [n for n in _module_names(model) if n not in _module_names(base)] == ["match_sampler"]
    sampler = model.match_sampler
    assert not list(sampler.parameters()) and not list(sampler.buffers())
    assert sampler._calls == 0 and callable(sampler.advance_seed)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        tr = Trainer(model, cfg, use_graph=True)
    assert tr.use_graph and not any("semantic part matching" in str(w.message) for w in caught)
    assert tr.state_dict()["dropout_calls"] == [0]
    # geometric data never matches: the option is inert there
    geo = config.dgl_everyday()
    geo.loss.match_sample = "device"
    assert not hasattr(build_model(geo), "match_sampler")
    bad = config.global_partnet_chair()
    bad.loss.match_sample = "gpu"
    with pytest.raises(ValueError, match="match_sample"):
        build_model(bad)


def test_sampler_counts_steps_the_same_way_eager_and_replayed():
    """An eager training step takes the next counter at `begin_step`; a replay takes the one `advance_seed` announced.
    Evaluation passes draw from a stream of their own and leave the training position alone."""
    s = matching.MatchSampler()
    dev = torch.device("cpu")
    s.begin_step(True)
    a0, a1 = s.draw_args(dev), s.draw_args(dev)
    assert (a0["counter"], a0["salt"]) == (1, 0) and (a1["counter"], a1["salt"]) == (1, matching.SALT_STEP)
    s.begin_step(False)
    assert s.draw_args(dev)["counter"] == (1 << 62) | 1 and s._calls == 1
    s.begin_step(True)
    assert s.draw_args(dev) == {"seed": torch.initial_seed() & U64, "salt": 0, "counter": 2}
    s.advance_seed()
    assert s._calls == 3


# ---- ABI, presets, dataset contract ---------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_and_validate_their_arguments():
    _build.build()
    L = _lib.lib()
    assert L.mpa_abi_version() == _lib.ABI_VERSION
    declared = _lib.declared_functions()
    for name, nargs in (("mpa_match_sample_indices", 10), ("mpa_merge_equal_parts", 13),
                        ("mpa_merge_equal_parts_backward", 13)):
        assert name in declared and len(_lib.SIGNATURES[name][1]) == nargs, name
    one = ctypes.c_void_p(8)  # a non-null pointer that is never dereferenced: every call below stops at its checks
    draw = lambda B, G, N, n, out=one: L.mpa_match_sample_indices(B, G, N, n, 1, 2, None, 3, out, None)
    assert draw(0, 4, 1000, 100) == 0  # an empty batch: nothing to do
    assert draw(2, 4, 1000, 100, out=None) == -1 and b"null" in L.mpa_last_error()
    assert draw(2, 4, CAP + 1, 100) == -1 and b"N=16385" in L.mpa_last_error()
    assert draw(2, 4, 1000, 129) == -1 and b"n=129" in L.mpa_last_error()
    assert draw(2, 4, 64, 65) == -1 and draw(2, 4, 0, 1) == -1 and draw(2, 4, 10, 0) == -1
    assert draw(2, 0, 1000, 100) == -1 and draw(-1, 4, 1000, 100) == -1
    args = [None] * 4
    assert L.mpa_merge_equal_parts(*args, 3, 65, 128, 128, *([None] * 5)) == -1 and b"P=65" in L.mpa_last_error()
    assert L.mpa_merge_equal_parts(*args, 3, 8, 128, 128, *([None] * 5)) == -1 and b"null" in L.mpa_last_error()
    assert L.mpa_merge_equal_parts_backward(*([None] * 6), 3, 8, 0, 128, None, None, None) == -1
    assert L.mpa_merge_equal_parts_backward(*([None] * 6), 3, 8, 64, 128, None, None, None) == -1
    assert b"null" in L.mpa_last_error()


def test_wrappers_have_no_cpu_fallback():
    from multi_part_assembly_amd import gnn_ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        matching.sample_indices(2, 2, 64, 16, seed=1, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gnn_ops.merge_equal_parts(torch.zeros(1, 2, 4), torch.zeros(1, 2, 4), torch.ones(1, 2), torch.zeros(1, 2))


def test_partnet_presets_restate_the_shipped_files_and_build():
    """configs/dgl/dgl-32x1-cosine_300e-partnet_chair.py, configs/rgl_net/rgl_net-32x1-cosine_300e-partnet_chair.py and
    configs/pn_transformer/pn_transformer/pn_transformer-32x1-cosine_400e-partnet_chair.py."""
    from multi_part_assembly_amd.gnn import DGLModel, RGLNet
    from multi_part_assembly_amd.pn_transformer import PNTransformer
    graph_keys = ("part_ids", "match_ids", "contact_points", "valid_matrix")
    for preset, cls, epochs, keys in (("dgl_partnet_chair", DGLModel, 300, graph_keys),
                                      ("rgl_net_partnet_chair", RGLNet, 300, graph_keys),
                                      ("pn_transformer_partnet_chair", PNTransformer, 400,
                                       ("part_ids", "match_ids", "contact_points"))):
        cfg = getattr(config, preset)()
        assert cfg.exp.num_epochs == epochs and cfg.exp.batch_size == 32 and cfg.data.data_keys == keys
        assert cfg.data.dataset == "partnet" and cfg.data.max_num_part == 20 and cfg.data.num_pc_points == 1000
        assert dict(cfg.loss) == dict(config.semantic_loss()) and cfg.loss.sample_iter == 5 and cfg.loss.noise_dim == 32
        assert cfg.optimizer.lr == 1e-3 and cfg.optimizer.lr_scheduler == "cosine"
        model = build_model(cfg)
        assert type(model) is cls and model.semantic and model.match_sample == "host"
    assert config.pn_transformer_partnet_chair().optimizer.warmup_ratio == 0.05
    assert config.dgl_partnet_chair().optimizer.warmup_ratio == 0.0
    assert config.rgl_net_partnet_chair().data.shuffle_parts is True
    assert "shuffle_parts" not in config.dgl_partnet_chair().data
    dgl = build_model(config.dgl_partnet_chair())
    assert dgl.merge_node and dgl.merge_on_device is True
    # the pose heads see features + pose + the P-wide instance label + 32 noise channels
    assert dgl.pose_predictors[0].fc_layers[0].in_features == 128 + 7 + 20 + 32


def test_match_ids_never_exceed_the_static_group_count():
    from multi_part_assembly_amd.datasets import match_ids
    assert matching.static_groups(20) == 10 and matching.static_groups(2) == 1 and matching.static_groups(1) == 1
    rng = np.random.RandomState(5)
    for _ in range(200):
        P = int(rng.randint(2, 21))
        geo = rng.randint(1, 8, size=int(rng.randint(2, P + 1)))
        out = match_ids(geo, P)
        assert out.max() <= matching.static_groups(P)
        labels = sorted(set(out[out > 0].tolist()))
        assert labels == list(range(1, len(labels) + 1))  # consecutive from 1
        assert all((out == g).sum() >= 2 for g in labels)
    assert match_ids(np.array([3, 3, 5, 5]), 4).tolist() == [1, 1, 2, 2]  # every slot grouped: exactly P // 2 groups
