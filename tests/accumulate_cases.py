"""What the gradient-accumulation tests (tests/test_grad_accumulate.py, tests/test_grad_accumulate_gpu.py and their rank
programs) share beyond `trainer_cases`: a host trainer whose forward and backward are a stub and whose launches are
recorded (the accumulate launch also RUNS, through the restatement), the `fit` stubs that know windows, and the hand-built
twin of a window on the device.  A plain module, imported by the test files."""
import numpy as np
import torch

from multi_part_assembly_amd import _lib, accum_ref
from trainer_cases import StubSampler, StubTrainer, cpu_trainer, i32, u8

# the tail of a step as the existing tests pin it (tests/test_weight_average.py, tests/test_step_guard*.py):
# (guard_step, guard_buffers) -> launches, in front of which clipping without a guard puts mpa_grad_clip_coef
TAILS = {(False, False): ["mpa_adam_step_dev"],
         (True, False): ["mpa_step_guard", "mpa_adam_step_guarded"],
         (True, True): ["mpa_step_guard", "mpa_adam_step_guarded", "mpa_guard_commit"]}


def tail(guard_step, guard_buffers, clip, average):
    names = list(TAILS[(guard_step, guard_buffers)])
    if clip and not guard_step:
        names.insert(0, "mpa_grad_clip_coef")
    return names + (["mpa_ema_update"] if average else [])


# ---- a trainer on host tensors ------------------------------------------------------------------------------------------------
def host_launches(monkeypatch):
    """`_lib.launch` replaced: every call is recorded as (name, args) and nothing runs, except mpa_grad_accumulate by
    value, which is carried out on the host tensors by the restatement (so a window's sum and a checkpoint's window can
    be followed without a device)."""
    calls = []

    def launch(name, dev, *args, **kw):
        calls.append((name, args))
        if name == "mpa_grad_accumulate" and args[4] is None:
            grad, acc = accum_ref.accumulate(args[3], args[0].numpy(), args[1].numpy())
            args[0].copy_(torch.from_numpy(grad))
            args[1].copy_(torch.from_numpy(acc))

    monkeypatch.setattr(_lib, "launch", launch)
    return calls


def host_trainer(grads=None, **kw):
    """`trainer_cases.cpu_trainer` whose forward + backward is a stub: micro-batch j writes `grads[j]` (a float: the whole
    flat gradient filled with it) and returns the loss j; the optimiser's device words are host tensors."""
    t, cfg = cpu_trainer(**kw)
    t.optimizer._hyper_dev = torch.zeros(8)
    t.seen = []

    def fwd_bwd(batch, loss_out=None, batch_idx=0):
        j = len(t.seen)
        t.seen.append(batch)
        t.optimizer.zero_grad()
        if grads is not None:
            t.flat.flat_grad.fill_(grads[j])
        return torch.tensor(float(j))

    t._fwd_bwd = fwd_bwd
    return t


def accumulate_modes(calls):
    return [c[1][3] for c in calls if c[0] == "mpa_grad_accumulate"]


# ---- fit with stubs -----------------------------------------------------------------------------------------------------------------
class WindowStubTrainer(StubTrainer):
    """A `StubTrainer` that accumulates: `calls` holds (batch, close_window) of every `train_step`."""

    def __init__(self, accumulate, **kw):
        super().__init__(**kw)
        self.accumulate, self.window, self.calls = accumulate, 0, []

    def train_step(self, batch, batch_idx=0, close_window=None):
        self.calls.append((batch["idx"], close_window))
        self.window += 1
        if close_window or self.window == self.accumulate:
            self.window = 0
            return super().train_step(batch)
        return torch.tensor(1.0)


class OldStubTrainer(StubTrainer):
    """A trainer from before the windows: no `accumulate`, and a `train_step` that takes the batch only."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def train_step(self, *args, **kw):
        self.calls.append((args, kw))
        return super().train_step(*args)


class Sampler(StubSampler):
    """`StubSampler` with `n` steps per epoch."""

    def __init__(self, n):
        super().__init__()
        self.n = n

    def __len__(self):
        return self.n

    def __iter__(self):
        while self.next_step < self.n:
            self.next_step += 1
            yield self.next_step


# ---- the device ------------------------------------------------------------------------------------------------------------------------
def state(t):
    """(parameters, exp_avg, exp_avg_sq as int32 words, the device's count of applied steps, every buffer's bytes)."""
    torch.cuda.synchronize()
    opt = t.optimizer
    count = int(opt._hyper_dev[4:5].view(torch.int32).item()) if opt._hyper_dev is not None else 0
    return {"param": i32(t.flat.flat_param), "exp_avg": i32(opt.exp_avg), "exp_avg_sq": i32(opt.exp_avg_sq), "count": count,
            "buffers": {name: u8(b) for name, b in t.model.named_buffers()}}


def assert_same(a, b, what="", buffers=True):
    for key in ("param", "exp_avg", "exp_avg_sq"):
        assert torch.equal(a[key], b[key]), (what, key)
    assert a["count"] == b["count"], (what, "count")
    if buffers:
        assert list(a["buffers"]) == list(b["buffers"])
        for name in a["buffers"]:
            assert torch.equal(a["buffers"][name], b["buffers"][name]), (what, name)


def twin_window(t, window):
    """The hand-built step of a trainer `t` (accumulate = 1, never stepped through `train_step`) over the micro-batches
    `window`: one zero_grad / forward / backward per batch and no step, each flat gradient recorded;
    `accum_ref.window_sum` written into the flat gradient; ONE `FusedAdam.step` with grad_scale = 1 / len(window).
    Returns the micro-batch losses."""
    t.model.train()
    grads, losses = [], []
    for b in window:
        losses.append(t._fwd_bwd(b).clone())
        torch.cuda.synchronize()
        grads.append(t.flat.flat_grad.cpu().numpy().copy())
    t.flat.flat_grad.copy_(torch.from_numpy(accum_ref.window_sum(grads)))
    t.optimizer.grad_scale = 1.0 / len(window)
    t.optimizer.step()
    return losses


def loss_bits(losses):
    torch.cuda.synchronize()
    return [np.float32(float(l)).view(np.int32).item() for l in losses]
