"""tools/rate_rig.py, the measuring rig of the rate tools, without a GPU: the order of synchronises, clock reads and calls
in `window` and `alternate` (the rig's clock and `torch.cuda.synchronize` replaced by a scripted clock and an event log),
the keys and rounding of `report`, the line and file of `emit`, the launch recorder, the cached part counts, and that each
of the fifteen tools imports by its path, has a `main` and keeps no private copy of what the rig holds."""
import importlib.util
import json
import os
import statistics
import sys

import pytest

from multi_part_assembly_amd import _lib
from tool_loader import ROOT, load_tool

sys.path.insert(0, os.path.join(ROOT, "tools"))
import rate_rig as rig  # noqa: E402

TOOLS = ["assembly_rate", "contact_rate", "ema_rate", "epoch_rate", "eval_rate", "geometry_producer_rate", "guard_rate",
         "partnet_producer_rate", "pointnet2_rate", "pointnet2_eval_rate", "pointnet2_interp_rate", "repulsion_rate",
         "semantic_step_rate", "lstm_step", "rmat_step"]
RIG_NAMES = ("window", "_window", "alternate", "report", "representative_parts", "optimizer_launches")


class Script:
    """The rig's clock reading scripted times, its synchronise and the arms writing into one event log."""

    def __init__(self, monkeypatch, times):
        self.events, self.times = [], iter(times)
        monkeypatch.setattr(rig, "perf_counter", self.clock)
        monkeypatch.setattr(rig.torch.cuda, "synchronize", lambda: self.events.append("sync"))

    def clock(self):
        t = next(self.times)
        self.events.append(("clock", t))
        return t

    def arm(self, name):
        return lambda i: self.events.append((name, i))


def windows_clock(durations, gap=1.0):
    """Clock reads for consecutive windows of the given durations (seconds), `gap` apart."""
    t, reads = 5.0, []
    for d in durations:
        reads += [t, t + d]
        t += d + gap
    return reads


# ---- window ----------------------------------------------------------------------------------------------------------------------
def test_window_is_sync_clock_calls_sync_clock(monkeypatch):
    s = Script(monkeypatch, [10.0, 10.5])
    ms = rig.window(s.arm("f"), 4, start=3)
    assert s.events == ["sync", ("clock", 10.0), ("f", 3), ("f", 4), ("f", 5), ("f", 6), "sync", ("clock", 10.5)]
    assert ms == (10.5 - 10.0) * 1e3 / 4
    s = Script(monkeypatch, [2.0, 2.25])
    assert rig.window(s.arm("f"), 2) == 125.0 and [e for e in s.events if e[0] == "f"] == [("f", 0), ("f", 1)]


# ---- alternate -------------------------------------------------------------------------------------------------------------------
CALLS, WARMUP = {"a": 2, "b": 3, "c": 1}, {"a": 1, "b": 2, "c": 3}
TIMED = {"a": [0.2, 0.4], "b": [0.3, 0.9], "c": [0.05, 0.01]}  # seconds per window


def expected_window(name, start, calls, t0, t1):
    return ["sync", ("clock", t0)] + [(name, start + i) for i in range(calls)] + ["sync", ("clock", t1)]


def test_alternate_runs_all_warmups_then_interleaves_the_arms(monkeypatch):
    order = [(n, 0, WARMUP[n], 0.125) for n in CALLS]  # (arm, first index, calls, seconds)
    order += [(n, WARMUP[n] + w * CALLS[n], CALLS[n], TIMED[n][w]) for w in range(2) for n in CALLS]
    reads = windows_clock([d for *_, d in order])
    s = Script(monkeypatch, reads)
    got = rig.alternate({n: s.arm(n) for n in CALLS}, CALLS, 2, WARMUP)
    want = []
    for k, (n, start, calls, _) in enumerate(order):
        want += expected_window(n, start, calls, reads[2 * k], reads[2 * k + 1])
    assert s.events == want
    for n in CALLS:  # every index once and in order
        assert [e[1] for e in s.events if e[0] == n] == list(range(WARMUP[n] + 2 * CALLS[n]))
    assert list(got) == list(CALLS)
    for n, (med, ts) in got.items():
        per_call = [d * 1e3 / CALLS[n] for d in TIMED[n]]
        assert ts == pytest.approx(per_call, rel=1e-12) and med == pytest.approx(statistics.median(per_call), rel=1e-12)
    assert got["a"][0] == pytest.approx(150.0) and got["b"][0] == pytest.approx(200.0) and got["c"][0] == pytest.approx(30.0)


def test_alternate_int_and_dict_forms_agree(monkeypatch):
    durations = [0.5] * 2 + [0.1, 0.3, 0.2, 0.8, 0.6, 0.4]  # two warm-ups, then three rounds over two arms
    runs = []
    for calls, warmup in ((4, 2), ({"x": 4, "y": 4}, {"x": 2, "y": 2}), (4, {"x": 2, "y": 2})):
        s = Script(monkeypatch, windows_clock(durations))
        runs.append((rig.alternate({"x": s.arm("x"), "y": s.arm("y")}, calls, 3, warmup), s.events))
    assert runs[0] == runs[1] == runs[2]
    got = runs[0][0]
    assert got["x"][1] == pytest.approx([25.0, 50.0, 150.0]) and got["x"][0] == pytest.approx(50.0)
    assert got["y"][1] == pytest.approx([75.0, 200.0, 100.0]) and got["y"][0] == pytest.approx(100.0)


def test_alternate_without_warmup_starts_at_index_zero(monkeypatch):
    s = Script(monkeypatch, windows_clock([0.1, 0.1]))
    rig.alternate({"x": s.arm("x")}, 2, 2, 0)
    assert s.events.count("sync") == 4 and [e for e in s.events if e[0] == "x"] == [("x", i) for i in range(4)]


# ---- report ----------------------------------------------------------------------------------------------------------------------
def test_report_keys_groups_and_rounding():
    result = {"a": (1.234567, [1.234549, 2.0, 0.000049]), "b": (0.5, [0.5])}
    frozen = json.dumps(result)
    out = {"kept": 1}
    rig.report(out, result)
    assert out == {"kept": 1, "a_ms": 1.2346, "a_ms_windows": [1.2345, 2.0, 0.0], "b_ms": 0.5, "b_ms_windows": [0.5]}
    out = {}
    rig.report(out, result, key="ms_{name}")
    assert out == {"ms_a": 1.2346, "ms_a_windows": [1.2345, 2.0, 0.0], "ms_b": 0.5, "ms_b_windows": [0.5]}
    out = {}
    rig.report(out, {"a": result["a"]}, key="{name}_alone_ms", digits=5)
    assert out == {"a_alone_ms": 1.23457, "a_alone_ms_windows": [1.23455, 2.0, 0.00005]}
    out = {"step": {"dgl": {"data_keys": ["k"]}}, "top": 0}
    rig.report(out, {"b": result["b"]}, group="producer")
    rig.report(out["step"], {"b": result["b"]}, group="dgl")
    assert out == {"step": {"dgl": {"data_keys": ["k"], "b_ms": 0.5, "b_ms_windows": [0.5]}}, "top": 0,
                   "producer": {"b_ms": 0.5, "b_ms_windows": [0.5]}}
    assert json.dumps(result) == frozen  # the figures handed in stay unrounded


# ---- emit ------------------------------------------------------------------------------------------------------------------------
def test_emit_prints_one_line_and_writes_it(tmp_path, capsys, monkeypatch):
    result = {"tool": "t", "nested": {"x_ms": 0.1234, "x_ms_windows": [0.1, 0.2]}, "flag": True, "none": None}
    path = tmp_path / "missing" / "dir" / "out.json"
    rig.emit(result, str(path))
    printed = capsys.readouterr().out
    assert printed.endswith("\n") and printed.count("\n") == 1 and json.loads(printed) == result
    assert path.read_text() == printed == json.dumps(result) + "\n"
    monkeypatch.chdir(tmp_path)
    before = sorted(p.name for p in tmp_path.iterdir())
    for out in ("", None):
        rig.emit(result, out)
        assert json.loads(capsys.readouterr().out) == result
    assert sorted(p.name for p in tmp_path.iterdir()) == before
    rig.emit(result, "bare.json")  # a file name without a directory
    assert (tmp_path / "bare.json").read_text() == json.dumps(result) + "\n"


# ---- recorded_launches -----------------------------------------------------------------------------------------------------------
def test_recorded_launches_records_and_restores(monkeypatch):
    reached = []
    real = lambda *a, **k: reached.append(a)  # noqa: E731
    monkeypatch.setattr(_lib, "launch", real)

    def calls():
        _lib.launch("mpa_b", "dev", 1, 2)
        _lib.launch("mpa_a", "dev", x=3)
        _lib.launch("mpa_b", "dev")

    assert rig.recorded_launches(calls) == ["mpa_b", "mpa_a", "mpa_b"]
    assert reached == [] and _lib.launch is real

    def raises():
        _lib.launch("mpa_c", "dev")
        raise ValueError("stop")

    with pytest.raises(ValueError, match="stop"):
        rig.recorded_launches(raises)
    assert reached == [] and _lib.launch is real


# ---- representative_parts --------------------------------------------------------------------------------------------------------
def test_representative_parts_are_bench_s_and_bench_runs_once(monkeypatch):
    spec = importlib.util.spec_from_file_location("bench_for_rate_rig_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    want = [bench.representative_parts("everyday", s) for s in range(1234, 1238)]
    executed, real = [], importlib.util.spec_from_file_location

    def counted(name, path, *a, **k):
        executed.append(os.path.basename(str(path)))
        return real(name, path, *a, **k)

    monkeypatch.setattr(importlib.util, "spec_from_file_location", counted)
    rig._bench.cache_clear()
    got = [rig.representative_parts(s) for s in range(1234, 1238)]
    assert got == want and len({tuple(p) for p in got}) > 1
    assert executed == ["bench.py"]
    assert rig.representative_parts(1234, preset="everyday") == want[0] and executed == ["bench.py"]


# ---- the tools -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TOOLS)
def test_tool_imports_by_path_and_keeps_no_private_rig(name):
    mod = load_tool(name)
    assert callable(mod.main)
    assert mod.rig is rig
    for attr in RIG_NAMES:
        if hasattr(mod, attr):
            assert getattr(mod, attr) is getattr(rig, attr, None), f"{name}.{attr} is a private copy"
