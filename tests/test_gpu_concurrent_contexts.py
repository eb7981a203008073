"""Results must not depend on other host threads: one context per thread, several threads at once.

include/flo_hip.h: "One flo_ctx per host thread / GPU; contexts are independent." In the code the contexts of a process
share the device pool (a block freed by one context is the next block another receives in that class, stale bytes and all),
the lazily made tables and per-device kernel attributes, and the debug switches; DESIGN.md ("What the contexts of a process
share") lists them. Here T = 4 threads each make a flo_amd.Context(0) of their own, meet at a barrier and run scenarios of
tests/recycled_scenarios.py side by side (tests/concurrent_harness.py). The yardstick throughout is the record the same
scenario returns alone: fresh context, main thread, every switch off, which the per-feature tests pin to their models and to
the oracle. Records are compared with recycled_scenarios.first_difference; equal bytes is the only criterion.

* the same scenario on every context at once, fill off: everyone takes and frees the same classes at the same moments;
* different scenarios side by side, thread i running scenario (k + 3 i) mod N - with 14 scenarios a stride of 3 never
  puts two scenarios of one feature together (asserted below) - with the fill off (stale bytes arrive from a foreign
  feature), under fill 0x7F and under 0xFF (a block handed across contexts is visibly different; the fill's device-wide
  wait inside pool_alloc runs on several threads at once, which is intended);
* churn beside work: one thread creates and destroys contexts, each with a small batch, while three threads run scenarios
  k, k + 1, k + 2. k = 5: the two lossy batches and the lossless batch, the scenarios that hold the most pool blocks at a
  time (PCM, coefficients, streams, files, ladders and resampled batches of up to 70 clips); k = 8: the corpus, the
  streaming decoders and the streaming encoders, the objects that keep their blocks longest;
* error text stays with its owner: flo_last_create_error is per thread, flo_last_error per context;
* first use, raced: one fresh child process per first-use site (tests/concurrent_child.py), four threads whose very first
  library call is the same scenario. One child at a time, so two processes have the GPU open:
    - "one-shot lossy encodes": the CRC host tables and the per-device device table (container_kernels.hip, crc_mu) and
      the lossy kernels' dynamic-LDS attribute set (lossy_kernels.hip, allow_big_lds);
    - "stage calls and resample": the resample kernels' attribute set (resample_kernels.hip, rs_allow_lds);
    - "normalise and true peaks": the normalise kernels' attribute set (normalize_kernels.hip, np_allow_lds);
    - "analysis": analysis.cpp's twiddle table (a function-local static) and each context's side streams;
* the Python default context is per thread: four threads call the free functions on the same inputs at once.

"rate-targeted encodes and free functions" goes through flo_amd.default_context(): with one module-level default context
(as before this test) it is the scenario that shared one flo_ctx among the four threads of the passes above.

The join limit is a hang guard, not a performance assertion: 60 s, or FACTOR = 10 x the sum of the four jobs' times
alone in this session where that is more (concurrent_harness.join_limit). The factor has to cover four-way contention for
the device and the device-wide wait of every filled allocation. Measured on an MI355X in one session of the whole suite
(ms; "alone" is the sum of the four jobs' times one after another on one thread, "at once" the pass from the first thread's
start to the last join, context creation included):

  same scenario on every context, fill off, alone -> at once: lossy encodes 4 -> 13, lossless encodes 8 -> 15, decodes
  34 -> 26, analysis 143 -> 76, stage calls 9 -> 9, lossy batch of six 44 -> 54, of 70 clips 160 -> 228, lossless batch
  13 -> 30, corpus 5 -> 12, streaming decoders 13 -> 24, streaming encoders 10 -> 15, fingerprint index 10 -> 6,
  normalise 17 -> 19, rate-targeted 12 -> 27;
  different scenarios from k = 0 .. 13, alone -> at once with the fill off / 0x7F / 0xFF: 80 -> 99 / 99 / 99,
  10 -> 17 / 20 / 20, 23 -> 31 / 41 / 42, 83 -> 90 / 95 / 98, 11 -> 21 / 28 / 28, 15 -> 31 / 35 / 31, 50 -> 69 / 72 / 73,
  17 -> 26 / 34 / 36, 40 -> 44 / 52 / 46, 12 -> 20 / 23 / 22, 25 -> 31 / 44 / 43, 79 -> 84 / 89 / 90, 12 -> 19 / 23 / 25,
  24 -> 39 / 44 / 45;
  churn beside work: k = 5, 54 -> 149 with 133 contexts created and destroyed beside it; k = 8, 7 -> 22 with 8;
  a first-use child: 2.2 .. 2.7 s in all (3.9 s for analysis, whose threads check their results against the model behind
  the oracle's lock), its four threads 21 .. 23 ms each from the barrier (1.6 s for analysis), entering the library together;
  the free functions on four threads: 30 ms.

A pass at once takes between half and three times its jobs' sequential sum, so the floor of 60 s is the limit everywhere,
hundreds of times what a pass needs, and the factor of 10 has never come into play. A thread that does not
come back ends the session: nothing more is started on the GPU. Nothing is retried."""
import gc
import json
import subprocess
import sys
import threading
import time
import weakref

import pytest

import concurrent_child
import concurrent_harness as H
import flo_amd
import normalize_recycled  # noqa: F401  (registers the normalise scenario)
import recycled_scenarios as S

pytestmark = pytest.mark.gpu

N = len(S.SCENARIOS)
NAMES = [s["name"] for s in S.SCENARIOS]
STRIDE = 3


def side_by_side(k):
    return [(k + i * STRIDE) % N for i in range(H.T)]


def _feature(name):
    return "lossy batch" if name.startswith("lossy batch") else name


for _k in range(N):   # the four are different scenarios of different features
    assert len({_feature(NAMES[j]) for j in side_by_side(_k)}) == H.T, [NAMES[j] for j in side_by_side(_k)]

CHURN_KS = [5, 8]
# What a child spends outside its threads - interpreter start, imports (numpy, the library, the oracle, the scenarios; 0.29 s
# of it) and shutdown - measured on an MI355X host: 0.7 s. The allowance is 10 x that, rounded up.
IMPORT_ALLOWANCE = 10.0


@pytest.fixture(scope="module", autouse=True)
def switches_off_afterwards():
    """the switches are process-wide: left on they would reach every later test"""
    H.lock_oracle()
    yield
    H.unlock_oracle()
    flo_amd.debug_stream_delay(None)
    flo_amd.debug_pool_fill(None)
    gc.collect()     # whatever a finished thread left behind goes now, not in the middle of a later module's test


_ALONE = {}   # scenario name -> (its record alone, seconds)


def alone(j):
    """scenario j's record alone: a fresh context, the main thread, the switches off. Made once per session, by two runs:
    the first fills the scenarios' cached inputs, so that no thread ever builds an input beside another and the time is the
    scenario's own; the second is timed, and must repeat the first."""
    name = NAMES[j]
    if name not in _ALONE:
        assert flo_amd.debug_pool_fill(None) is None and flo_amd.debug_stream_delay(None) is None
        c = flo_amd.Context(0)
        try:
            first = S.SCENARIOS[j]["run"](c)
            t0 = time.perf_counter()
            rec = S.SCENARIOS[j]["run"](c)
            seconds = time.perf_counter() - t0
        finally:
            c.close()
        assert S.first_difference(first, rec) is None, (name, "alone, twice", S.first_difference(first, rec))
        _ALONE[name] = (rec, seconds)
    return _ALONE[name]


def _fill_name(fill):
    return "off" if fill is None else hex(fill)


def _pass(js, fill=None, churn=None, what=""):
    """scenarios js side by side under `fill`; every record must be its scenario's record alone"""
    expected = [alone(j)[0] for j in js]
    sequential = sum(alone(j)[1] for j in js)
    limit = H.join_limit(sequential)
    r = None
    flo_amd.debug_pool_fill(fill)        # (process-wide: set before the barrier, restored after the join)
    try:
        r = H.run_side_by_side([S.SCENARIOS[j]["run"] for j in js], limit, churn=churn)
    finally:
        if r is None or r.all_back:      # (a thread that is still inside the library keeps the setting it started under)
            flo_amd.debug_pool_fill(None)
    print("%s fill %s: alone %.0f ms one after another, side by side %.0f ms (limit %.0f s)%s: %s"
          % (what, _fill_name(fill), 1e3 * sequential, 1e3 * r.wall, limit, "" if churn is None else ", %s rounds of churn" % r.churned,
             "; ".join("%s %.0f ms" % (NAMES[j], 1e3 * o.seconds) for j, o in zip(js, r.outcomes))))
    found = H.problems(r, expected, [NAMES[j] for j in js])
    if not r.all_back:
        pytest.exit("a thread did not come back: nothing more is started on the GPU. " + "; ".join(found), returncode=1)
    assert not found, found
    return r


# ---- 1. side by side ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(N), ids=NAMES)
def test_the_same_scenario_on_every_context_at_once(k):
    _pass([k] * H.T, None, what="same scenario,")


@pytest.mark.parametrize("k", range(N), ids=["%d: %s" % (k, NAMES[k]) for k in range(N)])
def test_different_scenarios_side_by_side(k):
    for fill in (None, 0x7F, 0xFF):
        _pass(side_by_side(k), fill, what="different scenarios from %d," % k)


def _churn(stop):
    """create a context, create and close a small batch on it, close the context, for as long as the others run"""
    rounds = 0
    while not stop.is_set():
        c = flo_amd.Context(0)
        try:
            b = flo_amd.Batch(c, flo_amd.MODE_LOSSY, [2 * 2048, 2 * 1], S.SR, 2, 0.55)
            b.close()
        finally:
            c.close()
        rounds += 1
    return rounds


@pytest.mark.parametrize("k", CHURN_KS, ids=["%d: %s .." % (k, NAMES[k]) for k in CHURN_KS])
def test_churn_beside_work(k):
    r = _pass([(k + i) % N for i in range(3)], None, churn=_churn, what="churn beside %d.. ," % k)
    assert r.churned >= 1, "no context was created and destroyed while the others ran"


# ---- 2. error text -----------------------------------------------------------------------------------------------------
def test_error_text_stays_with_its_owner():
    L = flo_amd._native.lib()
    a_failed, b_failed = threading.Event(), threading.Event()
    seen = {}

    def thread_a():
        try:
            flo_amd.Context(10 ** 6)
            seen["a raised"] = None
        except flo_amd.FloError as e:
            seen["a raised"] = str(e)
        seen["a create error"] = L.flo_last_create_error().decode()
        a_failed.set()
        assert b_failed.wait(60.0)
        seen["a create error afterwards"] = L.flo_last_create_error().decode()

    def thread_b():
        try:
            assert a_failed.wait(60.0)
            c = flo_amd.Context(0)
            try:
                ix = flo_amd.FingerprintIndex(S._fingerprints(300, 7), c)
                try:
                    ix.topk_self(65)
                    seen["b raised"] = None
                except flo_amd.FloError as e:
                    seen["b raised"] = str(e)
                seen["b last error"] = L.flo_last_error(c._h).decode()
                seen["b create error"] = L.flo_last_create_error().decode()
                ix.close()
            finally:
                c.close()
        finally:
            b_failed.set()

    S._fingerprints(300, 7)
    threads = [threading.Thread(target=f, daemon=True) for f in (thread_a, thread_b)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120.0)
    if any(t.is_alive() for t in threads):
        pytest.exit("a thread did not come back: nothing more is started on the GPU", returncode=1)
    print(seen)
    assert seen["a raised"] is not None and "device index" in seen["a raised"] and seen["a create error"] == seen["a raised"]
    assert seen["b raised"] == "k must be at most 64" and seen["b last error"] == seen["b raised"]
    assert seen["a create error afterwards"] == seen["a create error"], "B's failure changed A's create error"
    assert seen["b create error"] == "", "A's create error is visible on B"


# ---- 3. first use, raced -------------------------------------------------------------------------------------------------
FIRST_USE = ["one-shot lossy encodes", "stage calls and resample", "normalise and true peaks", "analysis"]
_CHILD = {"failed": None}


@pytest.mark.parametrize("name", FIRST_USE)
def test_first_use_raced_in_a_fresh_process(name):
    assert _CHILD["failed"] is None, "not started: the child for %r failed" % _CHILD["failed"]
    j = NAMES.index(name)
    rec, seconds = alone(j)
    want = concurrent_child.digests(rec)
    limit = H.join_limit(H.T * seconds)
    timeout = IMPORT_ALLOWANCE + H.BARRIER_LIMIT + limit + 30.0
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [concurrent_child.__file__, name, "%.1f" % limit]
    _CHILD["failed"] = name
    t0 = time.perf_counter()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)   # a fresh child process, one at a time
    except subprocess.TimeoutExpired:
        pytest.exit("the child for %r ran into its limit of %.0f s: nothing more is started on the GPU" % (name, timeout), returncode=1)
    took = time.perf_counter() - t0
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    print("%s: alone %.2f s, the child %.2f s in all (timeout %.0f s): %s" % (name, seconds, took, timeout, [x for x in lines if "digests" not in x]
                                                                             + [(x["thread"], x["seconds"]) for x in lines if "digests" in x]))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    threads = [x for x in lines if "thread" in x]
    assert [x["thread"] for x in threads] == list(range(H.T)) and all("digests" in x for x in threads), threads
    for x in threads:
        assert list(x["digests"]) == list(want), (name, x["thread"], "the records' labels differ")
        differing = [k for k in want if x["digests"][k] != want[k]]
        assert not differing, (name, "thread %d differs from the record alone" % x["thread"], differing[:8])
    _CHILD["failed"] = None


# ---- 4. the Python default context ---------------------------------------------------------------------------------------
def _free_functions():
    """a spread of free functions (each goes through flo_amd.default_context()) on fixed inputs"""
    from flo_amd import api
    x, y = S.music(5000, 2, 1), S.synth(3000, 2, 7)
    f_ll = api.encode(y, S.SR, 2, 16)
    f_lossy = api.encode_lossy(x, S.SR, 2, 16, 2)
    norm, report = api.normalize(x, S.SR, 2, target_lufs=-16.0, limit=True)
    rec = [("encode", f_ll), ("encode_lossy", f_lossy), ("decode lossless", S._b(api.decode(f_ll))), ("decode lossy", S._b(api.decode(f_lossy))),
           ("resample", S._b(api.resample(x, 44100, 48000, 2))), ("normalize", S._b(norm)), ("normalize report", repr(report).encode()),
           ("true_peak", repr(api.true_peak(x, S.SR, 2)).encode()), ("compare", S.fidelity_raw([api.compare(x, f_lossy, blocks=True)]))]
    rec += [("encode_ladder rung %d" % i, f) for i, f in enumerate(api.encode_ladder(x, S.SR, 2, S.LADDER5))]
    rec.append(("encode_to_bitrate", api.encode_to_bitrate(x, S.SR, 2, 96)))
    rec.append(("Encoder().encode", api.Encoder(S.SR, 2, 16).encode(y)))
    return rec


def test_free_functions_on_four_threads_use_four_contexts():
    want = _free_functions()
    mine = flo_amd.default_context()
    assert mine is flo_amd.default_context()
    out = [None] * H.T
    barrier = threading.Barrier(H.T, timeout=H.BARRIER_LIMIT)

    def work(i):
        try:
            barrier.wait()
            c = flo_amd.default_context()
            barrier.wait()               # all four contexts exist at once: their identities can be told apart
            rec = _free_functions()
            out[i] = (rec, weakref.ref(c), id(c), c is flo_amd.default_context(), flo_amd.Decoder()._ctx is c)
        except BaseException as e:
            out[i] = e

    t0 = time.perf_counter()
    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(H.T)]
    for t in threads:
        t.start()
    deadline = time.monotonic() + H.BARRIER_LIMIT + H.FLOOR
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    if any(t.is_alive() for t in threads):
        pytest.exit("a thread did not come back: nothing more is started on the GPU", returncode=1)
    print("free functions on %d threads: %.2f s" % (H.T, time.perf_counter() - t0))
    for i, o in enumerate(out):
        assert not isinstance(o, BaseException), (i, repr(o))
        rec, _, _, same_within, kept = o
        assert S.first_difference(want, rec) is None, (i, S.first_difference(want, rec))
        assert same_within and kept, (i, "default_context() is not one object within the thread")
    assert len({o[2] for o in out} | {id(mine)}) == H.T + 1, "two threads shared a default context"
    refs = [o[1] for o in out]
    del out, o, rec
    gc.collect()
    assert [r() for r in refs] == [None] * H.T, "a finished thread's default context is still alive"
    assert flo_amd.default_context() is mine
    assert S.first_difference(want, _free_functions()) is None
