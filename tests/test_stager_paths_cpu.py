"""The upload stager's three routes on the CPU, against a runtime whose device runs late: flo_amd/csrc/stager.cpp brings in
the data of every host-buffer entry point, by the runtime's pageable copy, by the pinned ring of four 8 MiB slots or by the
two-thread split of the pageable copy (FLO_UPLOAD_THREADS=2). A one-time probe of the host picks the route, so on one machine
the GPU suite sees one of them. The program is tests/native/stager_paths_test.cpp (its head names every check), built here
with g++ from stager.cpp unchanged and the deferred-execution stand-in for the runtime under tests/native/hipstub_streams
(late_runtime.cpp: streams as FIFOs of ops, pinned copies that read their source when they run, pageable copies that
snapshot it, events, gates, guard bytes, poison on free, allocation failures on demand, a lazy and an eager scheduling
policy). Built twice - AddressSanitizer with UBSan, and ThreadSanitizer - and each build runs twice: as it is, and with
FLO_UPLOAD_THREADS=2, which is a function-local static and so needs a process of its own. Stand-alone programs: nothing is
loaded into Python and nothing touches a GPU.

That the checks bite: each of the four waits was deleted once in a scratch copy of stager.cpp and the program run against it.
  * the slot-reuse `hipEventSynchronize(s->ev[k])` in upload_ring: "slot reuse" failed under both policies (both forms, the
    destinations held a later slot's bytes), and "table" under the lazy policy;
  * `hipStreamWaitEvent(s->aux_stream, s->aux_go, 0)`: "split aux_go" failed under the eager policy (the helper thread's
    half had been zeroed by the memset queued in front); the lazy policy cannot see it, it runs the second stream only when
    the first one waits for it;
  * `hipStreamWaitEvent(stream, s->aux_ev, 0)`: "split aux_ev" and "split aux_go" failed under the lazy policy (the helper's
    half never arrived: 15 728 704 of 20 971 585 bytes copied), and with them every upload of 16 MiB and more in "table" and
    "allocation"; the eager policy cannot see it;
  * the `hipEventSynchronize(s->ev[i])` of stager_destroy: "shutdown" failed under both policies (the model reported
    hipHostFree of a pinned block that queued copies still read, and the destinations received the poison byte).

The allocation check found the bug it was written for. On the commit before this test, ensure_ring returned at the first
failed hipHostMalloc or event creation and left slot[0] set, so the next large upload passed `if (s->slot[0]) return true`
with no workers and copied into a null slot: UBSan stopped the program at stager.cpp's `memcpy(j.dst, ...)` in
Stager::run ("null pointer passed as argument 1"), and without a sanitizer it ended with a segmentation fault. probe() had
the same exposure. ensure_ring now releases what it made and leaves no slot behind, and probe() falls back to the pageable
path when the ring cannot be made; the check passes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SANITIZERS = {"asan-ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "tsan": ["-fsanitize=thread"]}
REPORTS = ("AddressSanitizer", "ThreadSanitizer", "LeakSanitizer", "runtime error", "MODEL:", "FAIL [")


@pytest.fixture(scope="module", params=sorted(SANITIZERS))
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stager_paths") / ("stager_paths_test_" + request.param))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread"] + SANITIZERS[request.param] +
                   ["-I", os.path.join(NATIVE, "hipstub_streams"), "-I", os.path.join(ROOT, "flo_amd", "csrc"), "-o", exe,
                    os.path.join(NATIVE, "stager_paths_test.cpp"), os.path.join(NATIVE, "hipstub_streams", "late_runtime.cpp"),
                    os.path.join(ROOT, "flo_amd", "csrc", "stager.cpp")], check=True)
    return exe


def _run(exe, split):
    env = {k: v for k, v in os.environ.items() if k not in ("FLO_UPLOAD_THREADS", "FLO_UPLOAD_PATH", "FLO_SMALL_UPLOAD_MB")}
    if split:
        env["FLO_UPLOAD_THREADS"] = "2"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    print(r.stdout)
    for word in REPORTS:
        assert word not in r.stderr, r.stderr[-6000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("ok: direct, ring and split paths" if split else "ok: direct and ring paths"), last
    for policy in ("lazy", "eager"):
        ran = [x.split(",")[0] for x in r.stdout.splitlines() if x.endswith(" s") and ", %s: " % policy in x]
        assert ran == (["path", "table", "split", "allocation"] if split else
                       ["path", "small limit", "table", "slot reuse", "shutdown", "allocation", "worker pool"]), (policy, ran)


def test_direct_and_ring_paths_under_both_policies(program):
    _run(program, split=False)


def test_the_split_path_under_both_policies(program):
    _run(program, split=True)
