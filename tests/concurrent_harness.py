"""The harness of tests/test_gpu_concurrent_contexts.py: T jobs side by side, each on a thread of its own with a context
of its own. A job is a scenario's `run` of tests/recycled_scenarios.py, a function (ctx) -> [(label, bytes)].

Each thread makes its context on that thread, all threads meet at a barrier, each runs its job, closes its context on that
thread and leaves its record or its exception. The threads are daemon threads; the barrier and the join carry a time limit;
a thread that is not back at the limit is reported as such and nothing waits for it any longer (the caller then starts
nothing more on the GPU). Nothing is retried. No GPU is needed to import this module: tests/test_concurrent_harness_cpu.py
shows on fake jobs that the harness can fail."""
import threading
import time
from typing import NamedTuple

import recycled_scenarios as S

T = 4                    # threads of a side-by-side pass: a process has 4 hardware queues, a command 16 CPUs
BARRIER_LIMIT = 60.0     # seconds for all threads to have made their contexts
FLOOR = 60.0             # the least join limit, seconds
FACTOR = 10.0            # join limit = FACTOR x the sum of the jobs' times alone, where that is more than FLOOR


class Outcome(NamedTuple):
    record: object      # what the job returned (None if it did not)
    error: object       # the exception that ended the thread, or None
    back: bool          # the thread finished within the limit
    seconds: float      # the job alone, behind the barrier


class Pass(NamedTuple):
    outcomes: list      # one Outcome per job, in order
    wall: float         # from the start of the first thread to the last join, seconds
    churn: object       # the Outcome of the churn beside the jobs (its record: the rounds it made), None without one

    @property
    def all_back(self):
        """every thread finished within the limit (whether or not it raised)"""
        return all(o.back for o in self.outcomes) and (self.churn is None or self.churn.back)

    @property
    def churned(self):
        return self.churn.record if self.churn is not None and self.churn.back and self.churn.error is None else None


def join_limit(sequential_seconds):
    """the hang guard of a pass whose jobs took `sequential_seconds` one after another on one thread"""
    return max(FLOOR, FACTOR * float(sequential_seconds))


def _real_context():
    import flo_amd
    return flo_amd.Context(0)


_ORACLE_ORIGINALS = {}


def lock_oracle():
    """One thread at a time inside the CPU oracle, until unlock_oracle(). The scenarios check what they get against it as
    they run; it is test infrastructure with lazily made state of its own and was never asked to be re-entrant, and it is
    not what is under test here."""
    if _ORACLE_ORIGINALS:
        return
    import functools
    import types

    from oracle import oracle as O
    mu = threading.RLock()

    def locked(fn):
        @functools.wraps(fn)
        def call(*a, **kw):
            with mu:
                return fn(*a, **kw)
        return call
    for name, fn in list(vars(O).items()):
        if isinstance(fn, types.FunctionType) and fn.__module__ == O.__name__:
            _ORACLE_ORIGINALS[name] = fn
            setattr(O, name, locked(fn))


def unlock_oracle():
    """the oracle's own functions again"""
    from oracle import oracle as O
    for name, fn in _ORACLE_ORIGINALS.items():
        setattr(O, name, fn)
    _ORACLE_ORIGINALS.clear()


def run_side_by_side(jobs, limit, make_context=_real_context, churn=None, barrier_limit=BARRIER_LIMIT):
    """Run jobs[i](ctx_i) on len(jobs) threads at once -> Pass. `churn`, if given, is a function (stop) -> rounds that runs
    on one more thread from the same barrier until `stop` (a threading.Event) is set, which happens when every job thread
    is back or the limit has passed. While the threads run, recycled_scenarios.env leaves the environment alone (see
    S.ENV_FROZEN); it is released again only if every thread came back."""
    n = len(jobs) + (churn is not None)
    barrier = threading.Barrier(n, timeout=barrier_limit)
    stop = threading.Event()
    slots = [dict(record=None, error=None, seconds=0.0, done=False) for _ in range(n)]

    def work(i, job):
        s = slots[i]
        passed = False
        try:
            ctx = make_context()
            try:
                barrier.wait()
                passed = True
                t0 = time.perf_counter()
                try:
                    s["record"] = job(ctx)
                finally:
                    s["seconds"] = time.perf_counter() - t0
            finally:
                ctx.close()
        except BaseException as e:   # (reported, not raised: the thread has no one to raise to)
            s["error"] = e
            if not passed:
                barrier.abort()      # nobody waits for a thread that will not come
        finally:
            s["done"] = True

    def churning(i):
        s = slots[i]
        passed = False
        try:
            barrier.wait()
            passed = True
            s["record"] = churn(stop)
        except BaseException as e:
            s["error"] = e
            if not passed:
                barrier.abort()
        finally:
            s["done"] = True

    threads = [threading.Thread(target=work, args=(i, job), daemon=True, name="side-by-side %d" % i) for i, job in enumerate(jobs)]
    if churn is not None:
        threads.append(threading.Thread(target=churning, args=(n - 1,), daemon=True, name="churn"))
    frozen_before = S.ENV_FROZEN
    S.ENV_FROZEN = True
    t0 = time.perf_counter()
    deadline = time.monotonic() + barrier_limit + limit
    try:
        for t in threads:
            t.start()
        for t in threads[:len(jobs)]:
            t.join(max(0.0, deadline - time.monotonic()))
        stop.set()
        if churn is not None:
            threads[-1].join(max(barrier_limit, deadline - time.monotonic()))   # (its round in flight ends; it starts no other)
    finally:
        stop.set()
        back = [not t.is_alive() and s["done"] for t, s in zip(threads, slots)]
        if all(back):
            S.ENV_FROZEN = frozen_before
    wall = time.perf_counter() - t0
    outcomes = [Outcome(s["record"], s["error"], b, s["seconds"]) for s, b in zip(slots, back)]
    return Pass(outcomes[:len(jobs)], wall, outcomes[-1] if churn is not None else None)


def problems(result, expected, names=None):
    """What is wrong with a Pass, as a list of lines (empty: nothing): threads that did not come back, exceptions, and each
    record's first difference from expected[i], the record of the same job alone; a churn that did not come back or
    raised (an ordinary failure of the pass: result.all_back says whether every thread is back)"""
    out = []
    for i, o in enumerate(result.outcomes):
        who = "thread %d (%s)" % (i, names[i] if names else "job %d" % i)
        if not o.back:
            out.append("%s did not come back within the limit" % who)
        elif o.error is not None:
            out.append("%s raised %s: %s" % (who, type(o.error).__name__, o.error))
        else:
            diff = S.first_difference(expected[i], o.record)
            if diff is not None:
                out.append("%s differs from the record of the same job alone: %s" % (who, diff))
    if result.churn is not None and not result.churn.back:
        out.append("the churn thread did not come back within the limit")
    elif result.churn is not None and result.churn.error is not None:
        out.append("the churn thread raised %s: %s" % (type(result.churn.error).__name__, result.churn.error))
    return out
