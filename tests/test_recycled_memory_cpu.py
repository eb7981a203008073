"""The scenarios of tests/test_gpu_recycled_memory.py reach every entry point that touches device or pinned memory: each
name of flo_amd._native.EXPORTS is in some scenario's `covers` or in recycled_scenarios.EXEMPT with its one-line reason,
and never in both. No GPU needed."""
import re

import normalize_recycled  # noqa: F401  (registers the normalise scenario: the registry is whole when this module runs alone)
import recycled_scenarios as S
from flo_amd import _native


def _covered():
    return set(S.ALWAYS) | {n for s in S.SCENARIOS + S.LEFTOVERS for n in s["covers"]}


def test_every_export_is_covered_or_exempt():
    covered = _covered()
    assert not covered - set(_native.EXPORTS), sorted(covered - set(_native.EXPORTS))
    assert not set(S.EXEMPT) - set(_native.EXPORTS), sorted(set(S.EXEMPT) - set(_native.EXPORTS))
    assert not covered & set(S.EXEMPT), sorted(covered & set(S.EXEMPT))
    missing = [n for n in _native.EXPORTS if n not in covered and n not in S.EXEMPT]
    assert not missing, missing


def test_the_only_reasons_for_an_exemption():
    # host-only entry points, and the multi-rank exchange (which a single process cannot drive)
    for name, reason in S.EXEMPT.items():
        assert reason and "\n" not in reason, name
        assert name.startswith("flo_dist_") == ("several ranks" in reason), name


def test_a_scenario_calls_what_it_says_it_covers():
    """every covered name occurs in the scenarios' source or in the wrapper the source calls (flo_amd/api.py)"""
    import inspect

    import flo_amd.api as api
    text = inspect.getsource(S) + inspect.getsource(api)
    for name in _covered():
        assert re.search(r"\b%s\b" % name, text), name


def test_the_order_of_the_passes_and_the_scenarios():
    assert S.FILLS == (None, 0x00, 0x7F, 0xFF, None)
    names = [s["name"] for s in S.SCENARIOS]
    assert len(set(names)) == len(names) and len({s["name"] for s in S.LEFTOVERS}) == len(S.LEFTOVERS)
    assert names[0].startswith("one-shot lossy") and names[-1].startswith("rate-targeted")
    assert S.SUSPECT in S.analysis_cases()
    assert {c["family"] for c in S.AM.cases()} == {S.AM.case(n)["family"] for n in S.analysis_cases()}
