"""tools/benchkit.py, the timing kit of the per-feature benchmarks, on the CPU: the statistic, the verdict, where ``wall_times`` waits for the
device, the parser, the header and the tail - and that every tools/*_bench.py imports without a GPU and carries no timing code of its own."""
import glob
import importlib.util
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
KIT_NAMES = ("spread", "event_ms", "wall_ms", "event_times", "wall_times", "below", "event_mean_ms")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(TOOLS, name + ".py"))
    module = importlib.util.module_from_spec(spec)
    sys.modules[name] = module          # the tools say ``from benchkit import ...``: they get this object
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def kit():
    had = sys.modules.get("benchkit")
    yield _load("benchkit")
    sys.modules.pop("benchkit")
    if had is not None:
        sys.modules["benchkit"] = had


def test_spread_is_median_and_exclusive_interquartile_range(kit):
    assert kit.spread([1, 2, 3, 4, 5, 6, 7, 8]) == {"median": 4.5, "iqr": 4.5}          # quartiles 2.25 and 6.75
    assert kit.spread([0.123456]) == {"median": 0.1235, "iqr": None}
    assert kit.spread([0.1234567, 0.1234567, 0.2234567, 0.2234567], digits=6) == {"median": 0.173457, "iqr": 0.1}
    assert kit.spread([0.1234567], digits=6) == {"median": 0.123457, "iqr": None}


def test_below_is_strict_and_a_bool(kit):
    a = {"median": 1.0, "iqr": 0.2}
    assert kit.below(a, {"median": 1.5, "iqr": 0.2}) is True
    assert kit.below(a, {"median": 1.4, "iqr": 0.2}) is False          # 1.0 + 0.2 + 0.2 is not below 1.4
    assert kit.below({"median": 1.5, "iqr": 0.2}, a) is False


@pytest.mark.parametrize("sync,per_rep", [("none", 0), ("before", 1), ("both", 2)])
def test_wall_times_waits_for_the_device_where_sync_says(kit, monkeypatch, sync, per_rep):
    waits, calls = [], []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: waits.append(len(calls)))

    def fn():
        calls.append(len(waits))
        return len(calls)

    times, last = kit.wall_times(fn, 5, 3, sync)
    assert len(calls) == 3 + 5 and last == 8
    assert len(times) == 5 and all(t >= 0 for t in times)
    assert len(waits) == per_rep * 5
    assert calls[:3] == [0, 0, 0]          # the warm-up calls wait for nothing
    if sync == "both":          # one wait before and one after each timed call
        assert waits == [3, 4, 4, 5, 5, 6, 6, 7, 7, 8]
    if sync == "before":
        assert waits == [3, 4, 5, 6, 7]
    assert set(kit.wall_ms(fn, 5, 0, sync)) == {"median", "iqr"}


def test_wall_times_none_never_touches_the_device(kit, monkeypatch):
    def refuse(*a):
        raise AssertionError("sync='none' touched torch.cuda")

    monkeypatch.setattr(torch.cuda, "synchronize", refuse)
    times, last = kit.wall_times(lambda: "r", 4, 1, "none")
    assert len(times) == 4 and last == "r"
    with pytest.raises(AssertionError):
        kit.wall_times(lambda: "r", 1, 0, "before")


def test_wall_times_refuses_an_unknown_sync(kit):
    calls = []
    for sync in ("after", True, False, None):
        with pytest.raises(ValueError):
            kit.wall_times(lambda: calls.append(1), 2, 1, sync)
    assert not calls


def test_arguments_have_lib_only_when_asked(kit):
    args = kit.arguments("doc with a % sign").parse_args([])
    assert (args.reps, args.out) == (200, None) and not hasattr(args, "lib")
    with pytest.raises(SystemExit):
        kit.arguments("doc").parse_args(["--lib", "x.so"])
    args = kit.arguments("doc", lib=True).parse_args(["--lib", "x.so", "--reps", "7", "--out", "o.json"])
    assert (args.lib, args.reps, args.out) == ("x.so", 7, "o.json")
    assert kit.arguments("doc", lib=True).parse_args([]).lib is None


def test_header_has_the_common_keys_then_the_callers(kit, monkeypatch):
    monkeypatch.setattr(torch.cuda, "get_device_name", lambda *a: "a device")
    got = kit.header(x=1, a=2)
    assert list(got) == ["device", "cpus_usable", "cpus_machine", "lib", "x", "a"]
    assert got["cpus_usable"] == len(os.sched_getaffinity(0)) and got["cpus_machine"] == os.cpu_count()
    assert got["lib"].endswith("libadain_hip.so") and (got["x"], got["a"]) == (1, 2)


def test_emit_writes_the_printed_line_and_a_newline(kit, tmp_path, capsys):
    res = {"b": [1, 2.5], "a": {"c": None}}
    out = tmp_path / "record.json"
    kit.emit(res, str(out))
    printed = capsys.readouterr().out
    assert printed == json.dumps(res) + "\n" and out.read_text() == printed
    kit.emit(res, None)
    assert capsys.readouterr().out == printed and os.listdir(tmp_path) == ["record.json"]
    kit.write("a line", str(out))          # the writer of the tools that rewrite --out after every cell
    assert out.read_text() == "a line\n"


BENCHES = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(TOOLS, "*_bench.py")))


def test_the_sixteen_tools_are_found():
    assert len(BENCHES) == 16


@pytest.mark.parametrize("name", BENCHES)
def test_tool_imports_without_a_gpu_and_times_with_the_kit(kit, monkeypatch, name):
    monkeypatch.setattr(sys, "path", list(sys.path))          # the tools put the repository and tests/ on the path themselves
    environment = dict(os.environ)          # two tools set the host libraries' thread counts on import
    try:
        tool = _load(name)
    finally:
        sys.modules.pop(name, None)
        os.environ.clear()
        os.environ.update(environment)
    assert callable(tool.main)
    shared = [k for k in KIT_NAMES if hasattr(tool, k)]
    assert shared, "every tool takes at least one loop from the kit"
    for k in shared:
        assert getattr(tool, k) is getattr(kit, k), f"tools/{name}.py has a {k} of its own"
