"""flo_amd.default_context() is per thread: one object within a thread, different objects across threads, destroyed when its
thread has finished. The header's rule is one flo_ctx per host thread; the free functions and every object built without
ctx= go through default_context(), so this is what makes them keep the rule. api.Context is replaced by a stand-in, so the
logic is checked without a device (tests/test_gpu_concurrent_contexts.py has the same checks on real contexts)."""
import gc
import threading
import weakref

import pytest

import flo_amd
from flo_amd import api

T = 4


class StubContext:
    closed = []

    def __init__(self, device=0):
        self.device, self.made_on = device, threading.get_ident()

    def close(self):
        StubContext.closed.append(self.made_on)

    def __del__(self):
        self.close()


@pytest.fixture
def stub(monkeypatch):
    StubContext.closed = []
    monkeypatch.setattr(api, "Context", StubContext)
    monkeypatch.setattr(api, "_default", threading.local())   # (the main thread's real default context, if any, is left alone)
    return StubContext


def _on_threads(fn, n=T):
    out, barrier = [None] * n, threading.Barrier(n, timeout=30.0)

    def work(i):
        barrier.wait()
        out[i] = fn()
    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(30.0)
        assert not t.is_alive()
    return out


def test_one_object_within_a_thread_and_one_per_thread(stub):
    def within():
        a = api.default_context()
        b = flo_amd.default_context()
        made_here = a.made_on == threading.get_ident()
        built = api.Decoder()                         # an object built without ctx= keeps its builder's context
        return a is b and made_here and built._ctx is a and a.device == 0, id(a), weakref.ref(a), a.made_on
    mine = api.default_context()
    assert mine is api.default_context() and isinstance(mine, stub)
    got = _on_threads(within)
    assert all(ok for ok, _, _, _ in got)
    assert len({made_on for _, _, _, made_on in got}) == T and mine.made_on not in {m for _, _, _, m in got}
    assert api.default_context() is mine              # the main thread's is untouched by the others


def test_a_finished_threads_context_is_destroyed(stub):
    def within():
        c = api.default_context()
        return weakref.ref(c), c.made_on
    got = _on_threads(within)
    gc.collect()
    assert [r() for r, _ in got] == [None] * T, "a finished thread's default context is still alive"
    assert sorted(stub.closed) == sorted(m for _, m in got)       # each closed, once
    mine = api.default_context()                                   # a living thread keeps its own
    gc.collect()
    assert weakref.ref(mine)() is mine and mine.made_on not in stub.closed


def test_first_calls_that_race_make_one_context_each(stub):
    """the old module-level default raced on creation: two threads made two contexts and one was dropped"""
    made = []
    init = stub.__init__

    def counting(self, device=0):
        init(self, device)
        made.append(self.made_on)
    stub.__init__ = counting
    try:
        _on_threads(lambda: [api.default_context() for _ in range(3)] and None)
    finally:
        stub.__init__ = init
    assert len(made) == T and len(set(made)) == T
