"""The event loops of tools/benchkit.py on the device: how often they call, and that each time is a time."""
import importlib.util
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

KIT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "benchkit.py")


@pytest.fixture(scope="module")
def kit():
    spec = importlib.util.spec_from_file_location("benchkit_under_test", KIT)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_event_times_calls_warmup_plus_reps_and_times_each_rep(kit):
    x = torch.zeros(1, device="cuda")
    times, last = kit.event_times(lambda: x.add_(1), reps=8, warmup=2)
    assert len(times) == 8 and all(math.isfinite(t) and t >= 0 for t in times)
    assert x.item() == 10 and last is x
    got = kit.event_ms(lambda: x.add_(1), 4, 1)
    assert set(got) == {"median", "iqr"} and got["median"] >= 0 and got["iqr"] >= 0 and x.item() == 15


def test_event_mean_ms_calls_once_and_then_reps_times(kit):
    x = torch.zeros(1, device="cuda")
    ms = kit.event_mean_ms(lambda: x.add_(1), 8)
    assert math.isfinite(ms) and ms >= 0
    assert x.item() == 9
