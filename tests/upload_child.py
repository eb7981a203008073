"""What is fixed per process in the upload stager: run by tests/test_gpu_upload_paths.py in a fresh process, one at a time.

    FLO_SMALL_UPLOAD_MB=0 FLO_UPLOAD_PATH=ring      python upload_child.py ring-everything
    FLO_UPLOAD_THREADS=2  FLO_UPLOAD_PATH=direct    python upload_child.py split

FLO_SMALL_UPLOAD_MB (stager_upload's small_limit) and FLO_UPLOAD_THREADS (upload_direct's `two`) are function-local
statics, read at the first upload of the process; the parent sets them in the child's environment.

ring-everything: with a small limit of 0 every upload, however small, goes through the pinned ring: many tiny segments per
slot, odd lengths, single bytes. Runs RING_SCENARIOS, the scenarios of tests/recycled_scenarios.py whose calls reach
stager_upload (the call site each one reaches is listed there), on one context.

split: with two upload threads every pageable upload of 16 MiB and more in two or more segments is split between the
calling thread and a helper thread on the stager's second stream. Runs SPLIT_JOBS quiet, then late: the library's delay
switch on at 400 us (so that the stager queues its own delays behind aux_go and aux_ev) and four delays of 5000 us in front
of every call on the context's stream. Reports how many delays the library queued per late job: a split upload queues
two more than the same upload unsplit, which is how the parent knows that the split engaged.

Prints one JSON line {"job": name, "seconds": s, "digests": {"NNN label": sha256}, ...} per record and a last line
{"import_seconds": s, "upload_path": name}. Exit status 0 only if everything ran and the upload path is the one asked for.
Also holds the inputs and jobs that the parent and the child must build alike. Not a test module; reads nothing outside the
repository."""
import functools
import json
import os
import sys
import time

T0 = time.perf_counter()
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

SR = 44100
MiB = 1 << 20
# The encode cases' clips, in interleaved floats of a stereo batch, chosen so that the ring's cuts fall where they can go
# wrong: exactly one slot (8 MiB); one float more, cut behind 8 MiB; five of odd and even counts that share a slot with that float;
# an empty clip; an odd count (a stereo lossy clip's trailing partial frame is not uploaded); 36 MiB and 17 floats, which
# wraps the ring of four slots inside one call and is a chunk of its own in flo_encode_batch (chunks hold 48 MiB).
GEOMETRY = [2_097_152, 2_097_153, 300_001, 300_002, 300_003, 300_004, 300_005, 0, 123_457, 9_437_184 + 17]
ONE_CLIP = 2_400_002        # one clip above 8 MiB (9.2 MiB), an even count: lossy and lossless upload all of it
ANALYSIS_CLIP = 10_600_000  # above 40 MiB: five slots' worth through a ring of four
CORPUS_CLIPS = [1_900_000 + 2 * i for i in range(6)]   # six lossless files of noise, about 3.3 MB each: 20 MB in all
DELAY_US, LIB_DELAY_US, DELAYS_IN_FRONT = 5000, 400, 4

# Scenarios of tests/recycled_scenarios.py whose calls reach stager_upload, with the call site each one reaches. The others
# bring their samples in through flo_batch_upload (a plain hipMemcpyAsync: the batch scenarios, the stage calls, resample,
# normalise, edit), hold none (fingerprint index), or use the stager's copy threads only (the streaming decoders and lossy
# streaming encoders: stager_memcpy_many). None was dropped for time.
RING_SCENARIOS = [
    ("one-shot lossy encodes", "encode_one -> batch_upload_all (batch.cpp)"),
    ("one-shot lossless encodes", "encode_one -> batch_upload_all (batch.cpp)"),
    ("one-shot decodes", "flo_decode / flo_decode_lossless_i32 (decode.cpp) and flo_compare (fidelity.cpp)"),
    ("analysis", "analyze_impl (analysis.cpp), on the context's stream"),
    ("corpus windows", "flo_corpus_create (corpus.cpp)"),
    ("streaming encoders", "stream_encode_chunks -> batch_upload_all (stream.cpp)"),
    ("rate-targeted encodes and free functions", "flo_encode_batch on up_stream (batch.cpp), flo_encode_batch_to_size (rate.cpp), "
                                                 "flo_encode_batch_ladder (ladder.cpp)"),
]


def digests(record):
    from concurrent_child import digests as d
    return d(record)


@functools.lru_cache(maxsize=None)
def noise(n, seed):
    """n interleaved floats of noise at amplitude 0.25, as recycled_scenarios.noise makes it"""
    import recycled_scenarios as S
    return S.noise(n, 1, seed, 0.25)


def geometry_clips():
    return [noise(n, 900 + i) for i, n in enumerate(GEOMETRY)]


@functools.lru_cache(maxsize=None)
def integer_clip(n, seed):
    """(integers k, noise on the 16-bit grid that quantises to exactly k): the lossless encoder truncates s * 32767 toward
    zero (f32_to_i32), so the floats lie half a step outside k, where no f32 rounding can move the result"""
    import numpy as np
    k = np.random.default_rng(seed).integers(-8191, 8192, n).astype(np.int32)
    x = ((k + np.where(k < 0, -0.5, 0.5)) / 32767.0).astype(np.float32)
    x.setflags(write=False)
    return k, x


def batch_route(ctx, mode, clips, quality_or_level, bit_depth=None, metas=None, fidelity=False, analysis=False):
    """the route that does not use the stager: a Batch, one flo_batch_upload per clip (a plain hipMemcpyAsync from the
    caller's memory), encode, sync, fetch. -> dict(files=..., fidelity=raw reports, analysis=[(raw, META)])"""
    import flo_amd
    import recycled_scenarios as S
    b = flo_amd.Batch(ctx, mode, [x.size for x in clips], SR, 2, quality_or_level)
    try:
        for i, x in enumerate(clips):
            b.upload(i, x)
        out = {}
        if analysis:
            out["analysis"] = list(zip([S.analysis_raw(a) for a in b.analyze_all(50)], b.analysis_metadata_all(50)))
            out["analysis one clip"] = [b.analysis_metadata(i, 50) for i in range(b.n_clips)]
        if bit_depth:
            b.set_bit_depth(bit_depth)
        b.encode(0)
        b.sync()
        out["files"] = [b.fetch(i, metas[i] if metas else b"") for i in range(b.n_clips)]
        if fidelity:
            out["fidelity"] = [S.fidelity_raw([r]) for r in b.fidelity(blocks=True)]
        return out
    finally:
        b.close()


def corpus_windows(corpus, length=4096, starts=None):
    """[(file, start, float32 array [length, channels])]: three windows inside each file, or those at `starts`"""
    import numpy as np
    import torch
    fi, st = [], []
    for f, n in enumerate(int(x) for x in corpus.lengths):
        for s in starts or (0, n // 2 + 1, n - length):
            fi.append(f)
            st.append(s)
    out = torch.full((len(fi), length, corpus.channels), 7.0, device="cuda:0")
    torch.cuda.synchronize()
    corpus.decode_windows(np.array(fi, np.uint32), np.array(st, np.uint64), length, out=out)
    corpus.sync()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    return [(f, s, got[i]) for i, (f, s) in enumerate(zip(fi, st))]


# ---- the jobs of the split child: (ctx, inputs) -> record; the parent runs the same functions ------------------------------
def job_encode_batch(mode):
    def run(ctx, inputs):
        import flo_amd
        files = ctx.encode_batch(mode, geometry_clips(), SR, 2, 0.55 if mode == flo_amd.MODE_LOSSY else 5)
        return [("encode_batch %d" % i, f) for i, f in enumerate(files)]
    return run


def job_analysis(ctx, inputs):
    import recycled_scenarios as S
    x = noise(ANALYSIS_CLIP, 990)
    return [("analyze", S.analysis_raw(ctx.analyze(x, SR, 2, 50))), ("analysis_metadata", ctx.analysis_metadata(x, SR, 2, 50))]


def job_corpus(ctx, inputs):
    import flo_amd
    c = flo_amd.Corpus(inputs["corpus files"], ctx)
    try:
        return [("window of file %d at %d" % (f, s), w.tobytes()) for f, s, w in corpus_windows(c)]
    finally:
        c.close()


def split_jobs():
    import flo_amd
    return [("encode_batch lossy", job_encode_batch(flo_amd.MODE_LOSSY)), ("encode_batch lossless", job_encode_batch(flo_amd.MODE_LOSSLESS)),
            ("analysis above 40 MiB", job_analysis), ("corpus of six files", job_corpus)]


# Uploads of a job that the split takes: 16 MiB and more in two or more segments. flo_encode_batch: the first chunk (nine
# clips, 22 MiB; the 36 MiB clip is a chunk and a segment of its own). flo_corpus_create: six files, 20 MB. The analysis
# uploads its clip as ONE segment, so it is never split: it is here for the ring's counterpart, the pageable copy of 40 MiB
# on the context's stream with the device late.
SPLIT_UPLOADS = {"encode_batch lossy": 1, "encode_batch lossless": 1, "analysis above 40 MiB": 0, "corpus of six files": 1}


def corpus_inputs(ctx):
    """six lossless files of noise made by the stager-free route, each with a META chunk one byte longer than the last, so
    that odd and even byte lengths both occur"""
    import flo_amd
    clips = [integer_clip(n, 950 + i)[1] for i, n in enumerate(CORPUS_CLIPS)]
    metas = [b"\x81\xa1t" + bytes([0xa0 + i]) + b"a" * i for i in range(len(clips))]   # MessagePack {"t": "a" * i}
    return batch_route(ctx, flo_amd.MODE_LOSSLESS, clips, 0, metas=metas)["files"]


def run_late(ctx, fn, inputs, fill=None):
    """fn with the device late: the library's switch on, four long delays in front on the context's stream.
    -> (record, delays the library queued, seconds)"""
    import flo_amd
    flo_amd.debug_pool_fill(fill)
    flo_amd.debug_stream_delay(LIB_DELAY_US)
    try:
        before = flo_amd.debug_stream_delays()
        for _ in range(DELAYS_IN_FRONT):
            flo_amd.debug_delay_enqueue(ctx.stream(), DELAY_US)
        t0 = time.perf_counter()
        rec = fn(ctx, inputs)
        seconds = time.perf_counter() - t0
        return rec, flo_amd.debug_stream_delays() - before - DELAYS_IN_FRONT, seconds
    finally:
        flo_amd.debug_stream_delay(None)
        flo_amd.debug_pool_fill(None)


def main(argv):
    which = argv[1]
    import flo_amd
    import normalize_recycled  # noqa: F401  (registers its scenario, as in the parent)
    import recycled_scenarios as S
    import_seconds = time.perf_counter() - T0
    ctx = flo_amd.Context(0)
    try:
        if which == "ring-everything":
            assert os.environ.get("FLO_SMALL_UPLOAD_MB") == "0" and os.environ.get("FLO_UPLOAD_PATH") == "ring"
            want = "pinned-ring"
            for name, _site in RING_SCENARIOS:
                run = next(s["run"] for s in S.SCENARIOS if s["name"] == name)
                t0 = time.perf_counter()
                rec = run(ctx)
                print(json.dumps({"job": name, "seconds": round(time.perf_counter() - t0, 3), "digests": digests(rec)}), flush=True)
        elif which == "split":
            assert os.environ.get("FLO_UPLOAD_THREADS") == "2" and os.environ.get("FLO_UPLOAD_PATH") == "direct"
            want = "pageable-direct"
            inputs = {"corpus files": corpus_inputs(ctx)}
            for name, fn in split_jobs():
                t0 = time.perf_counter()
                quiet = fn(ctx, inputs)
                seconds = time.perf_counter() - t0
                late, delays, late_seconds = run_late(ctx, fn, inputs)
                print(json.dumps({"job": name, "seconds": round(seconds, 3), "late_seconds": round(late_seconds, 3), "delays": delays,
                                  "digests": digests(quiet), "late_digests": digests(late)}), flush=True)
        else:
            raise SystemExit("usage: upload_child.py ring-everything | split")
        path = ctx.upload_path()[0]
        print(json.dumps({"import_seconds": round(import_seconds, 3), "upload_path": path}), flush=True)
        return 0 if path == want else 4
    finally:
        ctx.close()


if __name__ == "__main__":
    sys.exit(main(sys.argv))
