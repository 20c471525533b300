"""tools/guide_loss_benchmark.py without a GPU: it imports, has a ``main``, and times with tools/benchkit.py's loops, statistic and verdict -
what tests/test_benchkit_host.py holds the sixteen tools/*_bench.py to (that file counts them, so this tool carries another suffix)."""
import importlib.util
import os
import sys

import numpy as np

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
KIT_NAMES = ("spread", "event_ms", "wall_ms", "event_times", "wall_times", "below", "event_mean_ms")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(TOOLS, name + ".py"))
    module = importlib.util.module_from_spec(spec)
    sys.modules[name] = module          # the tool says ``from benchkit import ...``: it gets this object
    spec.loader.exec_module(module)
    return module


def test_the_tool_imports_without_a_gpu_and_times_with_the_kit(monkeypatch):
    monkeypatch.setattr(sys, "path", list(sys.path))          # the tool puts the repository on the path itself
    had = sys.modules.get("benchkit")
    try:
        kit = _load("benchkit")
        tool = _load("guide_loss_benchmark")
    finally:
        sys.modules.pop("guide_loss_benchmark", None)
        sys.modules.pop("benchkit", None)
        if had is not None:
            sys.modules["benchkit"] = had
    assert callable(tool.main)
    shared = [k for k in KIT_NAMES if hasattr(tool, k)]
    assert {"event_ms", "wall_ms", "below", "spread"} <= set(shared)
    for k in shared:
        assert getattr(tool, k) is getattr(kit, k), f"tools/guide_loss_benchmark.py has a {k} of its own"
    assert tool.RENDERS == [(800, 800), (1080, 1920), (1200, 1600), (256, 456)] and tool.GUIDE == (512, 512)
    frame = tool.stylised_frame(32, 48)
    assert frame.shape == (32, 48, 3) and frame.dtype == np.uint8 and np.array_equal(frame, tool.stylised_frame(32, 48))
    assert tool.to_tensor(frame).shape == (3, 32, 48) and float(tool.to_tensor(frame).max()) <= 1.0
