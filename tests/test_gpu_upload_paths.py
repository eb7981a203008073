"""Every consumer of the upload stager on BOTH of its large paths, against a route that does not use the stager.

flo_amd/csrc/stager.cpp brings in the data of every host-buffer entry point. An upload above 8 MiB takes the runtime's
pageable copy ("pageable-direct") or the pinned ring of four 8 MiB slots ("pinned-ring"), whichever a one-time probe of the
host found faster, so on one machine the rest of the suite and bench.py exercise one of the two. Here FLO_UPLOAD_PATH, which
a context reads at its first large upload, forces each in turn: every test makes a fresh Context per path, makes one large
call, and asserts that ctx.upload_path()[0] names the path intended (a test that silently ran the other path would prove
nothing; the names asserted are printed). Records must be byte-equal between the two contexts and equal to a reference
that never enters the stager: a Batch filled by one flo_batch_upload per clip (a plain hipMemcpyAsync from the caller's
memory), encoded, synced and fetched (upload_child.batch_route). tests/native/stager_paths_test.cpp is the CPU counterpart:
it sees what no test here can (the source may be reused when the call returns; allocation failures; the waits, with the
device as late as a gate makes it).

  consumer                                  upload                                  reference
  ctx.encode_batch, lossy and lossless      flo_encode_batch on up_stream           batch_route of the same clips
  ctx.encode_lossy / encode_lossless        encode_one -> batch_upload_all          batch_route of the one clip
  ctx.decode, ctx.decode_lossless_i32       flo_decode: one file of 10 MB           the CPU oracle's decode of the file; the
                                                                                    Corpus window of the whole file on the
                                                                                    OTHER path
  flo_amd.Corpus over six files, 20 MB      flo_corpus_create                       slices of each file's whole decode
  ctx.compare on host buffers               flo_compare: file and 9.2 MiB of PCM    Batch.fidelity of the uploaded clip
  ctx.analyze / ctx.analysis_metadata       analyze_impl, on the context's stream   Batch.analyze_all, analysis_metadata_all
                                                                                    and analysis_metadata of the uploaded clip

The encode cases' geometry is upload_child.GEOMETRY (its comment says where the ring's cuts fall). All inputs are noise
at amplitude 0.25, made once per session. The decode and corpus files are lossless files of such noise on the 16-bit grid
(bit depth 24 in the header, level 0; they do not compress). Their yardstick is the CPU oracle's decoder and not the input
itself: the reference codec's lossless frames do not hold noise exactly (its own decoder returns between a few in 100 000
and 98 % of the input's integers, by level and amplitude; the device reproduces the oracle's files and integers bit for bit), so "decodes to its
input" is not a property a noise file has here. Compressible PCM that does round-trip would need several times the samples
to pass 8 MiB of file.

The ring's reuse with the device late (test_analysis_above_40_mib_with_the_device_late): 40.4 MiB through a ring of 32 MiB
on the context's stream, four delays of 5000 us queued in front, with the pool fill off and under 0x7F. Four such delays
hold the first slot's copy for about 20 ms; the host needs about 1 ms to fill four slots at the 30 - 35 GB/s DESIGN.md
records for the ring, under 7 ms even at 5 GB/s, so the fifth slot's fill meets a copy that has not run. The call's wall
time late and quiet is printed; DESIGN.md, "Who waits for whom", has the figures of one MI355X session and what the same
test did on a throwaway build without upload_ring's hipEventSynchronize(s->ev[k]).

What is fixed per process (FLO_SMALL_UPLOAD_MB and FLO_UPLOAD_THREADS are function-local statics) runs in two fresh child
processes, one at a time (tests/upload_child.py, whose head describes both): "ring-everything" sends every upload of the
scenarios that reach stager_upload through the ring; "split" runs the encode geometry, the corpus and the 40 MiB analysis with
two upload threads, quiet and late. Their digests must equal this process's records. A child that runs into its time limit
ends the session: nothing more is started on the GPU."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import flo_amd
import normalize_recycled  # noqa: F401  (registers its scenario: the scenario list is the one the other modules see)
import recycled_scenarios as S
import upload_child as U
from gpu_util import ctx  # noqa: F401
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SR = U.SR
NAMES = {"ring": "pinned-ring", "direct": "pageable-direct"}
PATHS = ("ring", "direct")
SMALL = 8 * U.MiB   # kSmallUpload


@pytest.fixture(scope="module", autouse=True)
def switches_off_afterwards():
    yield
    flo_amd.debug_stream_delay(None)
    flo_amd.debug_pool_fill(None)


class on_path:
    """a fresh context whose first large upload will read FLO_UPLOAD_PATH=path; leaving the block asserts that it did"""

    def __init__(self, monkeypatch, path):
        self.mp, self.path = monkeypatch, path

    def __enter__(self):
        self.mp.setenv("FLO_UPLOAD_PATH", self.path)
        self.c = flo_amd.Context(0)
        assert self.c.upload_path()[0] == "not measured yet"
        return self.c

    def __exit__(self, et, ev, tb):
        try:
            if et is None:
                got = self.c.upload_path()[0]
                print("FLO_UPLOAD_PATH=%s: the context reports %r" % (self.path, got))
                assert got == NAMES[self.path], (self.path, got)
        finally:
            self.c.close()


_REF = {}


def reference(ctx, key):
    """records of the stager-free route, made once per session on the session's context"""
    if key not in _REF:
        if key in ("lossy", "lossless"):
            mode, q = (flo_amd.MODE_LOSSY, 0.55) if key == "lossy" else (flo_amd.MODE_LOSSLESS, 5)
            _REF[key] = U.batch_route(ctx, mode, U.geometry_clips(), q)["files"]
        elif key in ("one lossy", "one lossless"):
            mode, q = (flo_amd.MODE_LOSSY, 0.55) if key == "one lossy" else (flo_amd.MODE_LOSSLESS, 5)
            _REF[key] = U.batch_route(ctx, mode, [U.noise(U.ONE_CLIP, 980)], q, fidelity=True, analysis=True)
        elif key == "decode file":
            k, x = U.integer_clip(5_600_000, 940)
            _REF[key] = U.batch_route(ctx, flo_amd.MODE_LOSSLESS, [x], 0, bit_depth=24)["files"][0]
        elif key == "corpus files":
            _REF[key] = U.corpus_inputs(ctx)
        elif key == "analysis 40":
            _REF[key] = U.batch_route(ctx, flo_amd.MODE_LOSSLESS, [U.noise(U.ANALYSIS_CLIP, 990)], 0, analysis=True)
    return _REF[key]


def test_the_geometry_is_what_its_comment_says():
    g = U.GEOMETRY
    assert g[0] * 4 == SMALL and g[1] * 4 == SMALL + 4 and 0 in g and any(n % 2 for n in g[2:7])
    assert g[-1] * 4 > 36 * U.MiB and g[-1] * 4 > 4 * SMALL and sum(g[:-1]) * 4 <= 48 * U.MiB < sum(g) * 4   # a chunk of its own
    assert sum(g[:-1]) * 4 >= 16 * U.MiB                                        # the first chunk is one the split takes
    # lossless, the ring cuts the first chunk into [clip 0], [8 MiB of clip 1], [its last float, the small clips]; lossy, clip 1
    # loses its odd float and fills its slot exactly
    assert (g[1] // 2 * 2) * 4 == SMALL and sum(g[2:-1]) * 4 + 64 * len(g) < SMALL
    assert U.ONE_CLIP * 4 > SMALL and U.ANALYSIS_CLIP * 4 > 40 * U.MiB


# ---- the consumers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["lossy", "lossless"])
def test_encode_batch_on_both_paths(ctx, monkeypatch, key):
    mode, q = (flo_amd.MODE_LOSSY, 0.55) if key == "lossy" else (flo_amd.MODE_LOSSLESS, 5)
    want = reference(ctx, key)
    assert sum(len(f) for f in want) > SMALL
    for path in PATHS:
        with on_path(monkeypatch, path) as c:
            got = c.encode_batch(mode, U.geometry_clips(), SR, 2, q)
        assert len(got) == len(want)
        differing = [i for i in range(len(want)) if got[i] != want[i]]
        assert not differing, (key, path, "files differ from the Batch route's", differing,
                               S.first_difference([("file", got[differing[0]])], [("file", want[differing[0]])]))


@pytest.mark.parametrize("key", ["one lossy", "one lossless"])
def test_one_clip_encode_on_both_paths(ctx, monkeypatch, key):
    x = U.noise(U.ONE_CLIP, 980)
    want = reference(ctx, key)["files"][0]
    for path in PATHS:
        with on_path(monkeypatch, path) as c:
            got = c.encode_lossy(x, SR, 2, 0.55) if key == "one lossy" else c.encode_lossless(x, SR, 2, 16, 5)
        assert got == want, (key, path, S.first_difference([("file", got)], [("file", want)]))


def test_decode_of_a_file_above_the_limit_on_both_paths(ctx, monkeypatch):
    f = reference(ctx, "decode file")
    assert len(f) > SMALL and flo_amd.probe_container(f).bit_depth == 24, len(f)
    want = O.decode_lossless_i32(f)[0]            # the CPU oracle's decoder: see the module's docstring
    assert want.size == 5_600_000
    pcm, window = {}, {}
    for path in PATHS:
        with on_path(monkeypatch, path) as c:
            pcm[path] = np.array(c.decode(f))
            assert np.array_equal(c.decode_lossless_i32(f), want), (path, "the oracle's integers")
            corpus = flo_amd.Corpus([f], c)                       # (another upload of the file on this path)
            try:
                n = int(corpus.lengths[0])
                assert n == want.size // 2
                window[path] = U.corpus_windows(corpus, length=n, starts=(0,))[0][2].reshape(-1)
            finally:
                corpus.close()
    assert np.array_equal(pcm["ring"].view(np.uint32), pcm["direct"].view(np.uint32))
    assert np.array_equal(pcm["ring"].view(np.uint32), window["direct"].view(np.uint32)), "decode on the ring against the corpus window on the pageable path"
    assert np.array_equal(pcm["direct"].view(np.uint32), window["ring"].view(np.uint32)), "decode on the pageable path against the corpus window on the ring"


def test_corpus_on_both_paths(ctx, monkeypatch):
    files = reference(ctx, "corpus files")
    assert sum(len(f) for f in files) > 16 * U.MiB and {len(f) % 2 for f in files} == {0, 1}, [len(f) for f in files]
    whole = [np.array(ctx.decode(f)).reshape(-1, 2) for f in files]      # each below the limit: never a large upload
    for i, n in enumerate(U.CORPUS_CLIPS):
        o = O.decode_lossless_i32(files[i])[0]
        assert o.size == n and np.array_equal(ctx.decode_lossless_i32(files[i]), o), (i, "the oracle's integers")
    for path in PATHS:
        with on_path(monkeypatch, path) as c:
            corpus = flo_amd.Corpus(files, c)
            try:
                for f, s, w in U.corpus_windows(corpus):
                    assert np.array_equal(w.view(np.uint32), whole[f][s:s + w.shape[0]].view(np.uint32)), (path, f, s)
            finally:
                corpus.close()


def test_compare_on_host_buffers_on_both_paths(ctx, monkeypatch):
    x = U.noise(U.ONE_CLIP, 980)
    for key in ("one lossy", "one lossless"):
        ref = reference(ctx, key)
        for path in PATHS:
            with on_path(monkeypatch, path) as c:
                got = S.fidelity_raw([c.compare(x, ref["files"][0], blocks=True)])
            assert got == ref["fidelity"][0], (key, path, S.first_difference([("report", got)], [("report", ref["fidelity"][0])]))


def _analysis_record(c, x):
    return [("analyze", S.analysis_raw(c.analyze(x, SR, 2, 50))), ("analysis_metadata", c.analysis_metadata(x, SR, 2, 50))]


def _analysis_reference(ref):
    raw, meta = ref["analysis"][0]
    assert ref["analysis one clip"][0] == meta
    return [("analyze", raw), ("analysis_metadata", meta)]


def test_analysis_on_host_buffers_on_both_paths(ctx, monkeypatch):
    x = U.noise(U.ONE_CLIP, 980)
    want = _analysis_reference(reference(ctx, "one lossless"))
    for path in PATHS:
        with on_path(monkeypatch, path) as c:
            got = _analysis_record(c, x)
        assert S.first_difference(got, want) is None, (path, S.first_difference(got, want))


# ---- the ring's reuse with the device late --------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_analysis_above_40_mib_with_the_device_late(ctx, monkeypatch, path):
    """On the ring this is the suite's GPU check of upload_ring's hipEventSynchronize(s->ev[k]): the fifth slot's fill must
    wait for the first slot's copy, which sits behind 20 ms of delays. On a throwaway build without that wait this test
    was run once and failed for the path "ring" (and passed for "direct"): already the quiet call returned another analysis
    than the Batch route's, the host refilling slot 0 faster than the copy engine drains it ("Who waits for
    whom", has the report and the wall times). The CPU program's "slot reuse" check (tests/native/stager_paths_test.cpp)
    holds the same wait with the device held back by a gate."""
    x = U.noise(U.ANALYSIS_CLIP, 990)
    want = _analysis_reference(reference(ctx, "analysis 40"))
    with on_path(monkeypatch, path) as c:
        t0 = time.perf_counter()
        quiet = U.job_analysis(c, None)
        t_quiet = time.perf_counter() - t0
        assert S.first_difference(quiet, want) is None, (path, "quiet", S.first_difference(quiet, want))
        for fill in (None, 0x7F):
            flo_amd.debug_pool_fill(fill)
            try:
                late = []
                t0 = time.perf_counter()
                for call in (lambda: ("analyze", S.analysis_raw(c.analyze(x, SR, 2, 50))), lambda: ("analysis_metadata", c.analysis_metadata(x, SR, 2, 50))):
                    for _ in range(U.DELAYS_IN_FRONT):
                        flo_amd.debug_delay_enqueue(c.stream(), U.DELAY_US)
                    late.append(call())
                t_late = time.perf_counter() - t0
            finally:
                flo_amd.debug_pool_fill(None)
            print("%s, fill %s: two analysis calls of %.1f MiB: quiet %.1f ms, behind 4 x %d us each %.1f ms"
                  % (NAMES[path], "off" if fill is None else hex(fill), x.size * 4 / U.MiB, 1e3 * t_quiet, U.DELAY_US, 1e3 * t_late))
            assert S.first_difference(late, quiet) is None, (path, fill, S.first_difference(late, quiet))


# ---- what is fixed per process -------------------------------------------------------------------------------------------
CHILD_LIMIT = 120.0   # a hang guard: a child takes a few seconds (the import, then under a second of work)
_CHILD = {"failed": None}


def _child(which, env):
    assert _CHILD["failed"] is None, "not started: the child %r failed" % _CHILD["failed"]
    _CHILD["failed"] = which
    e = {k: v for k, v in os.environ.items() if k not in ("FLO_UPLOAD_PATH", "FLO_UPLOAD_THREADS", "FLO_SMALL_UPLOAD_MB")}
    e.update(env)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [U.__file__, which]
    t0 = time.perf_counter()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT, env=e)   # a fresh child process, one at a time
    except subprocess.TimeoutExpired:
        pytest.exit("the child %r ran into its limit of %.0f s: nothing more is started on the GPU" % (which, CHILD_LIMIT), returncode=1)
    took = time.perf_counter() - t0
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    print("%s: the child took %.2f s in all: %s" % (which, took, [{k: v for k, v in x.items() if "digests" not in k} for x in lines]))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    _CHILD["failed"] = None
    return lines


def _same_digests(got, want, who):
    assert list(got) == list(want), (who, "the records' labels differ")
    differing = [k for k in want if got[k] != want[k]]
    assert not differing, (who, "differs from this process's record", differing[:8])


def test_every_upload_through_the_ring_in_a_fresh_process(ctx):
    names = [n for n, _ in U.RING_SCENARIOS]
    want, seconds = {}, 0.0
    for n in names:
        run = next(s["run"] for s in S.SCENARIOS if s["name"] == n)
        run(ctx)                                 # (builds the scenario's cached inputs)
        t0 = time.perf_counter()
        want[n] = U.digests(run(ctx))
        seconds += time.perf_counter() - t0
    lines = _child("ring-everything", {"FLO_SMALL_UPLOAD_MB": "0", "FLO_UPLOAD_PATH": "ring"})
    assert lines[-1]["upload_path"] == "pinned-ring"
    print("the scenarios here, quiet and with their inputs made: %.2f s; in the child, inputs included: %.2f s"
          % (seconds, sum(x["seconds"] for x in lines[:-1])))
    assert [x["job"] for x in lines[:-1]] == names
    for x in lines[:-1]:
        _same_digests(x["digests"], want[x["job"]], x["job"])


def test_the_split_upload_in_a_fresh_process(ctx, monkeypatch):
    inputs = {"corpus files": reference(ctx, "corpus files")}
    want, delays = {}, {}
    with on_path(monkeypatch, "direct") as c:   # unsplit: FLO_UPLOAD_THREADS is not set in this process
        for name, fn in U.split_jobs():
            quiet = fn(c, inputs)
            late, delays[name], _ = U.run_late(c, fn, inputs)
            assert S.first_difference(late, quiet) is None, (name, "late here", S.first_difference(late, quiet))
            want[name] = U.digests(quiet)
    for key, name in (("lossy", "encode_batch lossy"), ("lossless", "encode_batch lossless")):
        assert want[name] == U.digests([("encode_batch %d" % i, f) for i, f in enumerate(reference(ctx, key))]), name
    lines = _child("split", {"FLO_UPLOAD_THREADS": "2", "FLO_UPLOAD_PATH": "direct"})
    assert lines[-1]["upload_path"] == "pageable-direct"
    assert [x["job"] for x in lines[:-1]] == [n for n, _ in U.split_jobs()]
    for x in lines[:-1]:
        _same_digests(x["digests"], want[x["job"]], (x["job"], "quiet"))
        _same_digests(x["late_digests"], want[x["job"]], (x["job"], "late"))
        # a split upload queues two delays of its own, behind aux_go on the second stream and behind aux_ev on the first
        assert x["delays"] == delays[x["job"]] + 2 * U.SPLIT_UPLOADS[x["job"]], (x["job"], "delays queued", x["delays"], delays[x["job"]])
