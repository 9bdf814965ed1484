"""The one rig of the trainer-tail tests (guarded step, buffer rollback, weight average; tests/test_step_guard*.py,
tests/test_step_guard_rollback*.py, tests/test_weight_average*.py): the tiny model per family, the trainer factory, the
clean / poisoned / clean batches, bit views, random bytes between guard zones, the launch recorder, the
`fit` stubs and the two-rank launcher.  A plain module, imported by the test files (and by their rank programs)."""
import inspect
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from multi_part_assembly_amd import _build, _lib, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BT, PT, NT = 2, 3, 64  # samples, part slots, points per part
ZONE, SENTINEL = 256, 0xA5
PRESETS = {"pn": "pn_transformer_everyday", "dgl": "dgl_everyday"}  # (dgl: its MLPs' BatchNorm layers are csrc/mlp.hip's)


@pytest.fixture(scope="module")
def built():
    return _build.build()


# ---- model, trainer, batches ---------------------------------------------------------------------------------------------------
def tiny_cfg(preset="pn_transformer_everyday", layers=1):
    cfg = getattr(config, preset)()
    if preset.startswith("pn_transformer"):
        cfg.model.pc_feat_dim, cfg.model.transformer_heads = 64, 4
        cfg.model.transformer_feat_dim, cfg.model.transformer_layers = 128, layers
    cfg.data.max_num_part = PT
    return cfg


def model(dev, family="pn"):
    """The tiny model of a family (seed 7, two transformer layers) with every dropout switched off, and its cfg."""
    from multi_part_assembly_amd.pn_transformer import build_model
    cfg = tiny_cfg(PRESETS[family], layers=2)
    torch.manual_seed(7)
    net = build_model(cfg)
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    return net.to(dev), cfg


def trainer(dev, family="pn", **kw):
    from multi_part_assembly_amd.trainer import Trainer
    net, cfg = model(dev, family)
    return Trainer(net, cfg, **kw)


def cpu_trainer(**kw):
    """(trainer, cfg) on host tensors: one transformer layer, seed 1, dropout as the preset has it."""
    from multi_part_assembly_amd.pn_transformer import build_model
    from multi_part_assembly_amd.trainer import Trainer
    cfg = tiny_cfg()
    torch.manual_seed(1)
    return Trainer(build_model(cfg), cfg, **kw), cfg


def batch(dev, seed):
    from multi_part_assembly_amd import synthetic
    out = synthetic.make_batch(BT, PT, NT, preset="everyday", seed=seed, device=dev)
    out.pop("num_parts")
    return out


def batches(dev):
    """([clean, poisoned, clean], the clean twin of the second): the NaN sits in one sample's `part_trans`, which enters
    the loss only."""
    out = [batch(dev, seed) for seed in (60, 61, 62)]
    clean2 = {k: v.clone() for k, v in out[1].items()}
    out[1]["part_trans"][1, 0, 1] = float("nan")
    return out, clean2


# ---- bits ----------------------------------------------------------------------------------------------------------------------
def bits_i32(a):
    """A numpy array as a copy of its int32 words."""
    return np.ascontiguousarray(a).view(np.int32).copy()


def bits_bytes(a):
    """A numpy array as its bytes."""
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def i32(t):
    """A float32 / int32 tensor as a host tensor of its int32 words."""
    return t.detach().view(torch.int32).cpu().clone()


def u8(t):
    """Any tensor as a flat host tensor of its bytes."""
    return t.detach().reshape(-1).contiguous().view(torch.uint8).cpu().clone()


def opt_state(t, bits):
    """([parameters, exp_avg, exp_avg_sq] through `bits`, the device's count of applied steps)."""
    torch.cuda.synchronize()
    opt = t.optimizer
    return [bits(t.flat.flat_param), bits(opt.exp_avg), bits(opt.exp_avg_sq)], \
        int(opt._hyper_dev[4:5].view(torch.int32).item())


def buffers(t):
    torch.cuda.synchronize()
    return {name: u8(b) for name, b in t.model.named_buffers()}


def random_bytes(n, seed):
    """Random bits: about one float32 word in 256 is a NaN or an infinity and one in 256 a denormal; the first words are
    fixed special values (NaN payloads, both infinities, denormals, -0)."""
    a = np.random.RandomState(seed).randint(0, 256, size=n).astype(np.uint8)
    if n >= 32:
        a[:32].view(np.uint32)[:] = [0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x80000000,
                                     0x7FA00000]
    return a


class Zoned:
    """Bytes on the device (`mid`) between two sentinel-filled guard zones."""

    def __init__(self, host, dev):
        self.n = host.size
        self.buf = torch.full((ZONE + self.n + ZONE,), SENTINEL, dtype=torch.uint8, device=dev)
        self.mid = self.buf[ZONE:ZONE + self.n]
        self.mid.copy_(torch.from_numpy(host))
        assert self.mid.data_ptr() % 16 == 0

    def bytes(self):
        return self.mid.cpu().numpy()

    def words(self):
        return self.bytes().view(np.int32)

    def zones_intact(self):
        z = self.buf.cpu()
        return bool((z[:ZONE] == SENTINEL).all()) and bool((z[ZONE + self.n:] == SENTINEL).all())


# ---- launches, presets ------------------------------------------------------------------------------------------------------------
def record(monkeypatch):
    """`_lib.launch` replaced by a recorder (host tensors, nothing runs): the list of (name, args) it fills."""
    calls = []
    monkeypatch.setattr(_lib, "launch", lambda name, dev, *args, **kw: calls.append((name, args)))
    return calls


def optimizer_presets():
    """Every preset of `config` that has an optimiser section, built."""
    made = [f() for name, f in inspect.getmembers(config, inspect.isfunction)
            if not name.startswith("_") and not inspect.signature(f).parameters and f.__module__ == config.__name__]
    return [cfg for cfg in made if "optimizer" in cfg]


# ---- fit with stubs -----------------------------------------------------------------------------------------------------------------
class StubOptimizer:
    """Guard words and norm as host tensors (scripted by StubTrainer)."""

    lr = 0.5

    def __init__(self):
        self.words = torch.zeros(8, dtype=torch.int32)
        self.norm = torch.zeros(1)

    def grad_norm(self):
        return self.norm

    def guard_words(self):
        return self.words

    def guard_report(self, flat=None):
        return {"text": f"stub report: {int(self.words[2])} skipped"}

    def state_dict(self):
        return {"step": int(self.words[1]), "guard": self.words.clone()}

    def load_state_dict(self, state):
        self.words.copy_(state["guard"])


class StubTrainer:
    """What `fit` needs.  The optional parts: `skip` (step numbers; given, the trainer is a guarded one whose step k is
    skipped when k is in `skip`) and `average` (given, the trainer averages); `evaluate` records the weights it was asked
    for in `asked`."""

    static_batch, _fit_pending = None, None

    def __init__(self, skip=None, average=None):
        self.optimizer, self.skip, self.steps, self.epoch, self.asked = StubOptimizer(), set(skip or ()), 0, 0, []
        if skip is not None:
            self.guard_step = True
        if average is not None:
            self.average = average

    def set_epoch(self, epoch):
        self.epoch = epoch

    def train_step(self, batch):
        self.steps += 1
        w = self.optimizer.words
        if self.steps in self.skip:
            w[2] += 1
            w[3] += 1
            self.optimizer.norm[0] = float("inf")
        else:
            w[1] += 1
            w[3] = 0
            self.optimizer.norm[0] = float(self.steps)
        return torch.tensor(1.0)

    def check_health(self):
        pass

    def evaluate(self, batches, prefix="val", weights="live"):
        self.asked.append(weights)
        return {"val/part_acc": 0.5}

    def state_dict(self):
        return {"model": {}, "optimizer": self.optimizer.state_dict(), "epoch": self.epoch}

    def load_state_dict(self, state):
        self.optimizer.load_state_dict(state["optimizer"])
        self.epoch = state["epoch"]


class StubProducer:
    batch_counter = 0

    def batch(self, indices):
        return {"idx": indices}


class StubSampler:
    """Two steps per epoch, with the position a checkpoint carries."""

    def __init__(self):
        self.epoch, self.next_step = 0, 0

    def set_epoch(self, epoch):
        self.epoch, self.next_step = epoch, 0

    def __len__(self):
        return 2

    def __iter__(self):
        while self.next_step < 2:
            self.next_step += 1
            yield self.next_step

    def state_dict(self):
        return {"epoch": self.epoch, "next_step": self.next_step}

    def load_state_dict(self, s):
        self.epoch, self.next_step = s["epoch"], s["next_step"]


# ---- two ranks -------------------------------------------------------------------------------------------------------------------
def rank_setup(rank, port):
    """In a rank program: the gloo group of two; returns the rank's device."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=2)
    return torch.device("cuda", 0)


def run_two_ranks(file, **load_kw):
    """Start `python <file> <rank> <port> <out_dir>` for ranks 0 and 1, each under its own time limit; both must exit 0.
    Returns what each saved as `<out_dir>/rank<r>.pt` (`load_kw`: for `torch.load`)."""
    from test_dp_gpu import _free_port
    port = _free_port()
    with tempfile.TemporaryDirectory() as out_dir:
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
        procs = [subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(file), str(r), str(port),
                                   out_dir], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                 for r in range(2)]
        logs = [p.communicate()[0] for p in procs]
        assert [p.returncode for p in procs] == [0, 0], "\n".join(logs)
        return [torch.load(os.path.join(out_dir, f"rank{r}.pt"), **load_kw) for r in range(2)]
