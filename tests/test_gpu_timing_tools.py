"""tools/measure.py's event-timed blocks on the device, at the smallest case where a lost warm-up, a swapped loop nesting or a dropped call
would show: two kinds, two calls per block, three blocks each."""
import math

import pytest
import torch

from tools import measure

pytestmark = pytest.mark.gpu


def _kind(name, order):
    t = torch.zeros(1, dtype=torch.int32, device="cuda")

    def fn():
        t.add_(1)
        order.append(name)

    return t, fn


def _figures_ok(runs):
    return len(runs) == 3 and all(math.isfinite(x) and x >= 0.0 for x in runs)


def test_alternate(ctx):
    order = []
    ta, fa = _kind("a", order)
    tb, fb = _kind("b", order)
    runs = measure.alternate({"a": fa, "b": fb}, calls=2, repeats=3)
    assert order == ["a", "b"] + ["a", "a", "b", "b"] * 3        # one warm-up call of each kind, then the kinds block by block
    assert list(runs) == ["a", "b"] and _figures_ok(runs["a"]) and _figures_ok(runs["b"])
    assert ta.item() == 7 and tb.item() == 7


def test_blocks_ms(ctx):
    order = []
    t, fn = _kind("a", order)
    runs = measure.blocks_ms(fn, warmup=1, calls=2, repeats=3)
    assert order == ["a"] * 7 and _figures_ok(runs) and t.item() == 7


def test_event_and_wall_blocks_count_their_calls(ctx):
    order = []
    t, fn = _kind("a", order)
    assert measure.event_ms(fn, 3) >= 0.0 and t.item() == 3
    runs = measure.wall_ms(fn, calls=2, repeats=3, warmup=1)
    assert _figures_ok(runs) and t.item() == 3 + 7 and len(order) == 10
    assert measure.stream() == torch.cuda.current_stream().cuda_stream and measure.ptr(None) is None and measure.ptr(t) == t.data_ptr()
