"""The harness of the concurrent-context tests (tests/concurrent_harness.py) can fail: fed a job whose record depends on
state the threads share it reports a difference, fed a job that never returns it reports a thread that did not come back,
within its limit. No GPU: the contexts are stand-ins."""
import threading
import time

import concurrent_harness as H
import recycled_scenarios as S


class FakeContext:
    made = []

    def __init__(self):
        self.thread, self.closed_on = threading.get_ident(), None
        FakeContext.made.append(self)

    def close(self):
        self.closed_on = threading.get_ident()


def _independent(ctx):
    return [("a", b"same"), ("thread owns its context", bytes([ctx.thread == threading.get_ident()]))]


def test_independent_jobs_pass_and_each_thread_owns_its_context():
    FakeContext.made.clear()
    alone = _independent(FakeContext())
    r = H.run_side_by_side([_independent] * H.T, limit=30.0, make_context=FakeContext)
    assert r.all_back and H.problems(r, [alone] * H.T) == []
    ctxs = FakeContext.made[1:]
    assert len(ctxs) == H.T and len({c.thread for c in ctxs}) == H.T                 # one per thread, made on it
    assert all(c.closed_on == c.thread for c in ctxs)                                # and closed on it
    assert threading.get_ident() not in {c.thread for c in ctxs}
    assert S.ENV_FROZEN is False


def test_the_environment_is_left_alone_while_threads_run():
    import os
    seen = []

    def job(ctx):
        with S.env("FLO_HARNESS_SELF_TEST", "1"):
            seen.append((S.ENV_FROZEN, os.environ.get("FLO_HARNESS_SELF_TEST")))
        return []
    r = H.run_side_by_side([job] * 2, limit=30.0, make_context=FakeContext)
    assert r.all_back and seen == [(True, None)] * 2
    with S.env("FLO_HARNESS_SELF_TEST", "1"):       # single-threaded users: as before
        assert os.environ.get("FLO_HARNESS_SELF_TEST") == "1"
    assert "FLO_HARNESS_SELF_TEST" not in os.environ


def test_a_record_that_depends_on_shared_state_is_a_difference():
    counter, mu = [0], threading.Lock()

    def job(ctx):
        with mu:
            counter[0] += 1
            return [("a", b"same"), ("calls so far", bytes([counter[0]]))]
    alone = job(FakeContext())
    counter[0] = 0
    r = H.run_side_by_side([job] * H.T, limit=30.0, make_context=FakeContext)
    assert r.all_back
    found = H.problems(r, [alone] * H.T)
    assert len(found) == H.T - 1 and all("calls so far: first difference at byte 0" in p for p in found), found


def test_an_exception_is_reported_with_its_thread():
    def bad(ctx):
        raise ValueError("k must be 1 .. 64")
    alone = _independent(FakeContext())
    r = H.run_side_by_side([_independent, bad], limit=30.0, make_context=FakeContext)
    found = H.problems(r, [alone, alone], names=["fine", "bad"])
    assert len(found) == 1 and "thread 1 (bad) raised ValueError: k must be 1 .. 64" in found[0], found


def test_a_job_that_never_returns_is_a_thread_that_did_not_come_back():
    never = threading.Event()

    def stuck(ctx):
        never.wait()
        return []
    alone = _independent(FakeContext())
    t0 = time.perf_counter()
    try:
        r = H.run_side_by_side([_independent, stuck, _independent], limit=0.25, make_context=FakeContext, barrier_limit=0.25)
        took = time.perf_counter() - t0
        assert not r.all_back and [o.back for o in r.outcomes] == [True, False, True]
        found = H.problems(r, [alone] * 3)
        assert found == ["thread 1 (job 1) did not come back within the limit"], found
        assert took < 5.0, took                      # the limit, not the job, ended the pass
        assert S.ENV_FROZEN is True                  # a thread may still be inside the library: the environment stays frozen
    finally:
        never.set()                                  # (the stand-in can be let go; a real one could not)
        S.ENV_FROZEN = False


def test_the_churn_runs_beside_the_jobs_and_stops_with_them():
    started = threading.Event()

    def churn(stop):
        rounds = 0
        while not stop.is_set():
            rounds += 1
            started.set()
        return rounds

    def job(ctx):
        assert started.wait(30.0)                    # the churn runs while the job does
        return _independent(ctx)
    r = H.run_side_by_side([job] * 3, limit=30.0, make_context=FakeContext, churn=churn)
    assert r.all_back and r.churned >= 1 and H.problems(r, [_independent(FakeContext())] * 3) == []


def test_a_churn_that_raises_is_a_failure_of_the_pass_not_a_missing_thread():
    def churn(stop):
        raise RuntimeError("flo_batch_create failed")
    alone = _independent(FakeContext())
    r = H.run_side_by_side([_independent] * 2, limit=30.0, make_context=FakeContext, churn=churn)
    assert r.all_back and r.churned is None                # every thread is back: the session may go on
    assert H.problems(r, [alone] * 2) == ["the churn thread raised RuntimeError: flo_batch_create failed"]
    assert S.ENV_FROZEN is False


def test_a_churn_that_never_stops_is_a_thread_that_did_not_come_back():
    never = threading.Event()
    alone = _independent(FakeContext())
    try:
        r = H.run_side_by_side([_independent], limit=0.1, make_context=FakeContext, churn=lambda stop: never.wait(), barrier_limit=0.1)
        assert not r.all_back and H.problems(r, [alone]) == ["the churn thread did not come back within the limit"]
    finally:
        never.set()
        S.ENV_FROZEN = False


def test_the_oracle_lock_is_taken_off_again():
    from oracle import oracle as O
    before = O.crc32
    H.lock_oracle()
    try:
        assert O.crc32 is not before and O.crc32.__wrapped__ is before
        H.lock_oracle()                                    # (twice is once)
        assert O.crc32.__wrapped__ is before
    finally:
        H.unlock_oracle()
    assert O.crc32 is before


def test_the_join_limit():
    assert H.T == 4
    assert H.join_limit(0.5) == 60.0 and H.join_limit(6.0) == 60.0 and H.join_limit(9.0) == 90.0
