"""First use, raced: run by tests/test_gpu_concurrent_contexts.py in a fresh process, one process per first-use site.

    python concurrent_child.py "<scenario name>" <limit in seconds>

Four threads each make a Context(0), meet at a barrier, and each thread's very first library call behind it is the named
scenario of tests/recycled_scenarios.py: whatever that scenario initialises once per process or per device (the CRC tables,
a kernel's dynamic-LDS attribute, a host table behind a function-local static) is reached by four threads at once, none of
them having been there before. What the scenario needs that is made on the host alone (its signals, the oracle's
coefficients) is built before the threads start - WARM below - so that the threads enter the library together and not one
after another behind the oracle's lock. Prints one JSON line per thread, {"thread": i, "seconds": s, "digests": {"NNN label":
sha256}}, and a last line {"import_seconds": s}. Exit status 0 only if every thread came back and none raised. Not a test
module; reads nothing outside the repository."""
import hashlib
import json
import os
import sys
import time

T0 = time.perf_counter()
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def digests(record):
    """{"NNN label": sha256 of the bytes}: the position keeps equal labels apart and fixes the order"""
    return {"%03d %s" % (i, k): hashlib.sha256(v).hexdigest() for i, (k, v) in enumerate(record)}


def _warm_lossy(S):
    S.music(5000, 2, 1), S.music(1, 1, 2), S.music(3000, 3, 3)


def _warm_stages(S):
    S._stage_inputs(), S.music(3 * 2048, 1, 12), S.music(3000, 2, 13)


def _warm_normalise(S):
    S.noise(5000, 2, 81), S.noise(0, 2, 82), S.noise(2048, 2, 83, 0.3), S.noise(1, 2, 84), S.noise(6300, 2, 85, 0.05)


def _warm_analysis(S):
    for name in S.analysis_cases():
        S._case_input(name)


# scenario name -> what builds its cached host-only inputs (no call into the library)
WARM = {"one-shot lossy encodes": _warm_lossy, "stage calls and resample": _warm_stages, "normalise and true peaks": _warm_normalise,
        "analysis": _warm_analysis}


def main(argv):
    name, limit = argv[1], float(argv[2])
    import concurrent_harness as H
    import normalize_recycled  # noqa: F401  (registers the normalise scenario)
    import recycled_scenarios as S
    import_seconds = time.perf_counter() - T0
    run = next(s["run"] for s in S.SCENARIOS if s["name"] == name)
    WARM[name](S)
    H.lock_oracle()
    r = H.run_side_by_side([run] * H.T, limit)
    status = 0
    for i, o in enumerate(r.outcomes):
        if not o.back:
            print(json.dumps({"thread": i, "error": "did not come back within %.0f s" % limit}), flush=True)
            status = 3
        elif o.error is not None:
            print(json.dumps({"thread": i, "error": "%s: %s" % (type(o.error).__name__, o.error)}), flush=True)
            status = max(status, 2)
        else:
            print(json.dumps({"thread": i, "seconds": round(o.seconds, 3), "digests": digests(o.record)}), flush=True)
    print(json.dumps({"import_seconds": round(import_seconds, 3), "wall_seconds": round(r.wall, 3)}), flush=True)
    if status == 3:
        os._exit(status)   # a thread is still inside the library: no interpreter shutdown behind it
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv))
