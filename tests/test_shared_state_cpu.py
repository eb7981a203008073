"""Every writable object with static storage in the built library is listed in tests/shared_state.py with what guards it,
or is one of the toolchain's: a new global that two contexts' threads could meet in cannot arrive unnoticed. Needs the built
library (and binutils' nm), no GPU."""
import os
import re

import pytest

import shared_state as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "flo_amd", "libflo_hip.so")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="flo_amd/libflo_hip.so is not built")


def test_every_writable_static_is_listed_with_its_guard():
    names = W.writable_statics(LIB)
    assert len(names) > 50, names            # (the kernels' handles alone are more: nm found the library's symbols)
    unlisted, twice = [], []
    for n in names:
        (kind, _), hits = W.classify(n)
        if kind is None:
            unlisted.append(n)
        elif hits != 1:
            twice.append(n)
    assert not unlisted, "writable statics that tests/shared_state.py does not list: %r" % unlisted
    assert not twice, twice


def test_every_entry_names_a_guard_and_still_exists():
    names = W.writable_statics(LIB)
    for pattern, guard, what, reached in W.SHARED:
        assert guard.startswith(W.GUARDS), (pattern, guard)
        assert what and reached and "\n" not in what + reached, pattern
        assert any(re.fullmatch(pattern, n) for n in names), "no such object any more: " + pattern
    for pattern, reason in W.TOOLCHAIN:
        assert reason and "\n" not in reason, pattern
    # a mutex an entry names is itself an object of the library
    for _, guard, _, _ in W.SHARED:
        if guard.startswith("mutex "):
            mu = guard[len("mutex "):].replace("()", r"\(.*\)")
            assert any(re.search(mu + "$", n) for n in names), guard


def test_the_design_document_has_the_same_list():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    assert "What the contexts of a process share" in text
    section = text.split("What the contexts of a process share", 1)[1]
    for word in ("g_mu", "g_live", "g_free", "g_cached", "g_pool_fill", "g_stream_delay", "crc_mu", "allow_big_lds", "rs_allow_lds", "np_allow_lds",
                 "tw_table", "term_table", "trace", "small_limit", "two", "g_create_err", "shader_mhz"):
        assert word in section, word
