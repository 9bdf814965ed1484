"""The measuring rig of the `tools/*_rate.py` scripts (and lstm_step.py, rmat_step.py): what they all do the same way.

  window       a host clock around `calls` calls of `fn(i)` between two device synchronises, in ms per call
  alternate    the protocol of every timed arm: a warm-up window per arm, then `windows` rounds over the arms in their
               order, one window each; an arm's call index runs on across its windows; the median of an arm's windows is
               its figure, the windows stay beside it
  report       those figures into the result, rounded, under `<key>` and `<key>_windows`
  emit         the result as one JSON line on stdout, and into `--out` when given

and the inputs they share: the part counts of `bench.representative_parts`, the c2 batches made from them, the recorder
of `_lib.launch` entry points.  Importing this module puts the repository root on `sys.path`; a tool puts its own
directory there first (tests load the tools by file path).  HIP-event timings stay with the two tools that have them."""
import functools
import importlib.util
import json
import os
import statistics
import sys
from time import perf_counter

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def require_gpu(tool):
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool}: needs the GPU (a host timing says nothing about the device)")


@functools.lru_cache(maxsize=None)
def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def representative_parts(seed, preset="everyday"):
    """`bench.representative_parts(preset, seed)`; bench.py is executed once per process."""
    return _bench().representative_parts(preset, seed)


def c2_batches(dev, count, seed=1234, B=32, P=20, N=1000, keep_num_parts=False):
    """`count` synthetic batches of the c2 workload; batch i has seed + i and the representative part counts of seed + i."""
    from multi_part_assembly_amd import synthetic
    batches = [synthetic.make_batch(B, P, N, seed=seed + i, device=dev, num_parts=representative_parts(seed + i))
               for i in range(count)]
    if not keep_num_parts:
        for b in batches:
            b.pop("num_parts")
    return batches


def window(fn, calls, start=0):
    """ms per call of fn(start) .. fn(start + calls - 1), the window opened and closed by a device synchronise."""
    torch.cuda.synchronize()
    t0 = perf_counter()
    for i in range(calls):
        fn(start + i)
    torch.cuda.synchronize()
    return (perf_counter() - t0) * 1e3 / calls


def alternate(arms, calls, windows, warmup):
    """arms: name -> fn(i); calls, warmup: an int or name -> int (a warm-up of 0 runs no window).
    -> name -> (median ms, [window ms]), unrounded."""
    calls = calls if isinstance(calls, dict) else dict.fromkeys(arms, calls)
    warmup = warmup if isinstance(warmup, dict) else dict.fromkeys(arms, warmup)
    for name, fn in arms.items():
        if warmup[name]:
            window(fn, warmup[name])
    times = {name: [] for name in arms}
    for w in range(windows):
        for name, fn in arms.items():
            times[name].append(window(fn, calls[name], start=warmup[name] + w * calls[name]))
    return {name: (statistics.median(ts), ts) for name, ts in times.items()}


def report(out, result, key="{name}_ms", digits=4, group=None):
    """`alternate`'s figures into out (or out[group]): key -> the median, key + "_windows" -> the windows, rounded."""
    dest = out if group is None else out.setdefault(group, {})
    for name, (med, ts) in result.items():
        k = key.format(name=name)
        dest[k] = round(med, digits)
        dest[k + "_windows"] = [round(t, digits) for t in ts]


def recorded_launches(fn):
    """The entry-point names `_lib.launch` is called with while fn() runs; nothing is launched."""
    from multi_part_assembly_amd import _lib
    names, real = [], _lib.launch
    _lib.launch = lambda name, dev, *a, **k: names.append(name)
    try:
        fn()
    finally:
        _lib.launch = real
    return names


def emit(result, out):
    line = json.dumps(result)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(line + "\n")
