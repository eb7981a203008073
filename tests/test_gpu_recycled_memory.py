"""Results must not depend on what a recycled block held (tests/recycled_scenarios.py has the scenarios).

Every device buffer comes from the pool of flo_amd/csrc/devpool.cpp, which hands freed blocks out again uncleared, and
pinned download buffers are recycled the same way; DESIGN.md ("What a block holds when it arrives") says for every
allocation site who writes what before whom. flo_debug_pool_fill makes both allocators fill what they hand out:

* each scenario runs with the switch off, under 0x00 (what hides a missing clear), under 0x7F (3.4e38 as f32, 1.4e306 as
  f64, a large positive integer: wins every max, breaks every counter), under 0xFF (NaN, -1, the largest unsigned: a
  float max discards it, so it alone would hide a stale maximum) and with the switch off again: five identical records,
  and equal to the CPU-side anchors where the suite has them;
* what an object keeps between calls the switch cannot reach: A, B, A on one object, B larger and harsher than A; both A
  records identical and equal to A's on a fresh object.

Correct code never reads the fill, so equal bytes is all that is asserted."""
import pytest

import flo_amd
import recycled_scenarios as S
from gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def switch_off_afterwards():
    """the ctx fixture lasts the session and the pool the process: a fill left on would reach every later test"""
    yield
    flo_amd.debug_pool_fill(None)


def test_the_switch_returns_the_previous_setting():
    assert flo_amd.debug_pool_fill(None) is None            # off at the start (and left off by whoever used it)
    assert flo_amd.debug_pool_fill(0x7F) is None
    assert flo_amd.debug_pool_fill(0) == 0x7F
    assert flo_amd.debug_pool_fill(None) == 0
    L = flo_amd._native.lib()
    assert L.flo_debug_pool_fill(256) == -1 and L.flo_debug_pool_fill(-2) == -1 and L.flo_debug_pool_fill(-1) == -1   # refused: unchanged
    with pytest.raises(ValueError):
        flo_amd.debug_pool_fill(300)


@pytest.mark.parametrize("name", [s["name"] for s in S.SCENARIOS])
def test_fill(ctx, name):
    run = next(s["run"] for s in S.SCENARIOS if s["name"] == name)
    records = []
    try:
        for fill in S.FILLS:
            flo_amd.debug_pool_fill(fill)
            records.append(run(ctx))
    finally:
        flo_amd.debug_pool_fill(None)
    for fill, rec in zip(S.FILLS[1:], records[1:]):
        diff = S.first_difference(records[0], rec)
        assert diff is None, (name, "fill %s against the switch off" % ("off" if fill is None else hex(fill)), diff)


@pytest.mark.parametrize("name", [s["name"] for s in S.LEFTOVERS])
def test_leftovers(ctx, name):
    run = next(s["run"] for s in S.LEFTOVERS if s["name"] == name)
    assert flo_amd.debug_pool_fill(None) is None
    fresh, first, again = run(ctx)
    diff = S.first_difference(first, again)
    assert diff is None, (name, "A after B against A before it", diff)
    diff = S.first_difference(fresh, first)
    assert diff is None, (name, "A against A on a fresh object", diff)
