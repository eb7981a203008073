"""Results must not depend on when queued work runs: every scenario and every ordering contract, with the device late.

The library works across many streams (the context's, the upload and download streams of flo_encode_batch's pipeline, the
analysis' side streams, a caller's stream through the decode plan's events) and its host code relies on explicit waits in
front of every read-back and every release of a pool block. The other tests' kernels end long before the host's next
step, so a missing wait, fork, join or an early pool_free would go unseen. flo_debug_stream_delay makes the library
queue a delay (one sleeping wavefront: no memory access, nothing waited for) in front of every launch of its own and
behind every wait for an event on its own streams, so the device really is DELAY_US behind per launch, accumulating.

* the window test shows that the delay does what it is for: work behind it has not run when an unordered reader looks;
* every scenario of tests/recycled_scenarios.py runs quiet, then late under pool fill 0x7F and late under 0xFF: identical
  records. The fill makes a block that was released early and handed out again visibly different; the delay makes the early
  release possible;
* the ordering contracts of include/flo_hip.h, each late, with a delay on the caller's stream in front of the producer.

The expected values are the same calls' results with the delay off, which the per-feature tests pin to their models."""
import ctypes as C
import time

import numpy as np
import pytest

import flo_amd
import normalize_recycled  # noqa: F401  (registers the normalise scenario)
import recycled_scenarios as S
from gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

# Twice the smallest of 100, 200, 500, 1000, 2000 us at which the window and the stream query below held in 20 of 20
# consecutive tries on an MI355X: 200 us (at 100 us the host's own path to the reader is as long as the delay and the window
# held in 13 of 20). DESIGN.md, "Who waits for whom", has the measurement.
DELAY_US = 400

HIP_NOT_READY = 600   # hipErrorNotReady


@pytest.fixture(scope="module", autouse=True)
def switches_off_afterwards():
    """the switches are process-wide: left on they would reach every later test"""
    yield
    flo_amd.debug_stream_delay(None)
    flo_amd.debug_pool_fill(None)


class late:
    """the delay on (and a pool fill) for a block; .launches: the delays queued inside it"""

    def __init__(self, fill=0x7F, us=None):
        self.fill, self.us = fill, DELAY_US if us is None else us

    def __enter__(self):
        flo_amd.debug_pool_fill(self.fill)
        flo_amd.debug_stream_delay(self.us)
        self.n0, self.launches = flo_amd.debug_stream_delays(), 0
        return self

    def __exit__(self, *exc):
        self.launches = flo_amd.debug_stream_delays() - self.n0
        flo_amd.debug_stream_delay(None)
        flo_amd.debug_pool_fill(None)


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamQuery.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def _raw_upload(b, clips):
    """flo_batch_upload alone: Batch.upload waits for the copy, this does not (the arrays are the scenarios' cached inputs
    and outlive the call)"""
    for i, x in enumerate(clips):
        assert x.dtype == np.float32 and x.flags.c_contiguous and x.size == b.n_interleaved[i]
        b.ctx._chk(b._L.flo_batch_upload(b._h, i, x.ctypes.data))


def _raw_pcm(b):
    """every clip's PCM as it sits in the batch, by null-stream copies and with no flo_batch_sync of this batch"""
    hip, out = _hip(), []
    for i, n in enumerate(b.n_interleaved):
        buf = np.zeros(max(n, 1), np.float32)
        if n:
            assert hip.hipMemcpy(buf.ctypes.data, b._L.flo_batch_clip_device_data(b._h, i), n * 4, 2) == 0
        out.append(buf[:n].tobytes())
    return out


# ---- a. the switch ---------------------------------------------------------------------------------------------------
def test_the_switch_returns_the_previous_setting_and_the_counter_grows(ctx):
    import torch
    try:
        assert flo_amd.debug_stream_delay(None) is None            # off at the start (and left off by whoever used it)
        assert flo_amd.debug_stream_delay(100) is None
        assert flo_amd.debug_stream_delay(0) == 100
        assert flo_amd.debug_stream_delay(5000) == 0
        L = flo_amd._native.lib()
        for refused in (5001, -2, 1 << 20):
            assert L.flo_debug_stream_delay(refused) == 5000       # refused: the setting stays
        assert flo_amd.debug_stream_delay(None) == 5000
        assert L.flo_debug_stream_delay(-1) == -1
        with pytest.raises(ValueError):
            flo_amd.debug_stream_delay(5001)
        assert L.flo_debug_delay_enqueue(ctx.stream(), 5001) != 0 and L.flo_debug_delay_enqueue(ctx.stream(), -1) != 0
        # off: no delay is queued; on: one per launch at the least; the explicit call counts whatever the switch says
        x = S.music(3000, 2, 13)
        n0 = flo_amd.debug_stream_delays()
        ctx.resample(x, 44100, 48000, 2)
        assert flo_amd.debug_stream_delays() == n0
        flo_amd.debug_delay_enqueue(ctx.stream(), 0)
        assert flo_amd.debug_stream_delays() == n0 + 1
        flo_amd.debug_stream_delay(0)
        ctx.resample(x, 44100, 48000, 2)
        assert flo_amd.debug_stream_delays() >= n0 + 2
    finally:
        flo_amd.debug_stream_delay(None)
        torch.cuda.synchronize()


# ---- b. the delay opens a window -------------------------------------------------------------------------------------
READERS = 8   # twice the hardware queues a process has by default: not all of them can share the context's queue


def window_holds(ctx, us, readers=READERS):
    """(how many unordered readers saw zeros, every ordered one saw the fill): a fill behind a delay on the context's
    stream, read from another stream with no event between them. A read-only race made on purpose; it touches nothing of
    the library's. A process has a handful of hardware queues (four by default) and a reader whose stream shares the
    context's queue is ordered behind the fill by the hardware - measured: one torch stream in four alone in a process,
    two in four inside the suite - so each try reads from `readers` streams in turn, and the window is open when at least
    a quarter of them see the zeros."""
    import torch
    cs = torch.cuda.ExternalStream(ctx.stream())
    t = torch.zeros(4096, device="cuda:0")
    pin = torch.ones(4096).pin_memory()
    n_early, after = 0, True
    for other in [torch.cuda.Stream() for _ in range(readers)]:
        t.zero_()
        pin.fill_(1.0)
        torch.cuda.synchronize()
        flo_amd.debug_delay_enqueue(cs, us)
        with torch.cuda.stream(cs):
            t.fill_(1.0)
        with torch.cuda.stream(other):
            pin.copy_(t, non_blocking=True)
        other.synchronize()
        n_early += bool((pin == 0).all())
        cs.synchronize()
        with torch.cuda.stream(other):
            pin.copy_(t, non_blocking=True)
        other.synchronize()
        after = after and bool((pin == 1).all())
    return n_early, after


def stream_is_busy_behind_a_call(ctx, us):
    """hipStreamQuery on the context's stream right after an asynchronous library call has returned, the switch on"""
    cs = S.batch_clips()
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [x.size for x in cs], S.SR, 2, 0.55)
    try:
        S._upload(b, cs)
        flo_amd.debug_stream_delay(us)
        r = b.resample(48000)
        status = _hip().hipStreamQuery(ctx.stream())
        flo_amd.debug_stream_delay(None)
        r.close()
        return status == HIP_NOT_READY
    finally:
        flo_amd.debug_stream_delay(None)
        b.close()


def test_the_delay_opens_a_window(ctx):
    try:
        early, after = window_holds(ctx, DELAY_US)
        print("readers that saw the zeros: %d of %d" % (early, READERS))
        assert after, "the fill behind the delay never arrived"
        # The bound: a reader is ordered behind the fill only where its stream shares the context's hardware queue. With Q
        # queues dealt out evenly that is one reader in Q (Q = 4 by default: 6 of 8 see zeros); the runtime deals unevenly
        # when other streams exist (seen: up to one in two), and a process may run with Q = 2. A quarter of the readers is
        # asked for: what is left when the sharing is three times the even deal, and more than one reader's luck.
        assert early >= READERS // 4, "%d of %d readers on other streams saw the zeros: the delay opened no window" % (early, READERS)
        assert stream_is_busy_behind_a_call(ctx, DELAY_US), "the context's stream was idle right behind Batch.resample"
    finally:
        flo_amd.debug_stream_delay(None)


# ---- c. every recycled-memory scenario, run late -----------------------------------------------------------------------
def _flat(result):
    """a leftover's three records as one"""
    if isinstance(result, tuple):
        return [("%s: %s" % (tag, k), v) for tag, rec in zip(("fresh", "first", "again"), result) for k, v in rec]
    return result


def _fill_name(fill):
    return "off" if fill is None else hex(fill)


# the passes of the contracts below: the fill the issue names, and the fill off (under a fill every pool_alloc waits for the
# whole device, so a call that takes a block between the delay and its launches meets an idle device; off, nothing drains it)
FILLS = [0x7F, None]
FILL_IDS = ["fill 0x7f", "fill off"]


ALL = [(s["name"], s["run"]) for s in S.SCENARIOS] + [("A, B, A: " + s["name"], s["run"]) for s in S.LEFTOVERS]


@pytest.mark.parametrize("name", [n for n, _ in ALL])
def test_late(ctx, name):
    run = next(r for n, r in ALL if n == name)
    try:
        t0 = time.perf_counter()
        quiet = _flat(run(ctx))
        t_quiet = time.perf_counter() - t0
        # the fill off first: a fill makes every pool_alloc wait for the whole device, which drains the lag at each block a
        # call takes; without it nothing but the library's own waits stands between the host and the late device
        for fill in (None, 0x7F, 0xFF):
            t0 = time.perf_counter()
            with late(fill) as w:
                rec = _flat(run(ctx))
            print("%s: fill %s: %d launches delayed by %d us, %.2f s (quiet %.2f s)" % (name, _fill_name(fill), w.launches, DELAY_US, time.perf_counter() - t0, t_quiet))
            assert w.launches > 0, (name, "no delay was queued")
            diff = S.first_difference(quiet, rec)
            assert diff is None, (name, "late under fill %s against quiet" % _fill_name(fill), diff)
    finally:
        flo_amd.debug_stream_delay(None)
        flo_amd.debug_pool_fill(None)


# ---- d. the ordering contracts the header states ---------------------------------------------------------------------
def _corpus_calls(corpus):
    fi, st1, st2 = [], [], []
    for f, n in enumerate(int(x) for x in corpus.lengths):
        for s in (0, n // 2, n - 5, n + 7):
            fi.append(f)
            st1.append(s)
            st2.append(max(s - 300, 0) + 11)
    return np.array(fi, np.uint32), np.array(st1, np.uint64), np.array(st2, np.uint64)


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
def test_corpus_windows_on_a_late_caller_stream(ctx, fill):
    """flo_corpus_decode_windows: ordered behind what is queued on `stream`, later work on `stream` sees the result; a
    second call that reuses the corpus' scratch right behind the first must not disturb it"""
    import torch
    c = flo_amd.Corpus(S._corpus_files(), ctx)
    L = 1500
    try:
        fi, st1, st2 = _corpus_calls(c)
        want = []
        for st in (st1, st2):
            o = c.decode_windows(fi, st, L)
            c.sync()
            torch.cuda.synchronize()
            want.append(o.cpu().numpy())
        s = torch.cuda.Stream()
        with late(fill) as w, torch.cuda.stream(s):
            out1, out2 = torch.empty((len(fi), L, c.channels), device="cuda:0"), torch.empty((len(fi), L, c.channels), device="cuda:0")
            flo_amd.debug_delay_enqueue(s, DELAY_US)
            out1.fill_(7.0)          # the destination's earlier writer is late: the decode must land behind it
            out2.fill_(7.0)
            c.decode_windows(fi, st1, L, out=out1)
            y1 = out1 * 2.0          # no host synchronisation: ordered by the stream alone
            c.decode_windows(fi, st2, L, out=out2)
            y2 = out2 * 2.0
        s.synchronize()
        assert w.launches > 0
        for got, ref, tag in ((y1, want[0] * 2.0, "first call, read behind it"), (y2, want[1] * 2.0, "second call, read behind it"),
                              (out1, want[0], "first call"), (out2, want[1], "second call")):
            assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32)), tag
        c.sync()
    finally:
        flo_amd.debug_stream_delay(None)
        flo_amd.debug_pool_fill(None)
        c.close()


def _fed(ctx, files):
    decs = [flo_amd.StreamingDecoder(ctx) for _ in files]
    for d, f in zip(decs, files):
        d.feed(f)
    return decs


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
def test_streams_decode_on_a_late_caller_stream(ctx, fill):
    """flo_sdec_decode_ready with a caller's stream, lossy and lossless streams mixed: the same two-sided check"""
    import torch
    files = S._sdec_files_a()
    sets = (files, files[::-1])
    decs = []
    try:
        want = []
        for fs in sets:
            ds = _fed(ctx, fs)
            decs += ds
            r = flo_amd.decode_streams(ds)
            torch.cuda.synchronize()
            want.append((r.out.cpu().numpy(), r.offsets.copy()))
        s = torch.cuda.Stream()
        got = []
        with late(fill) as w, torch.cuda.stream(s):
            outs = [torch.empty(max(ref.size, 1), device="cuda:0") for ref, _ in want]
            fed = [_fed(ctx, fs) for fs in sets]   # (in front of the delay: under a fill every pool block taken waits for the device)
            decs += fed[0] + fed[1]
            flo_amd.debug_delay_enqueue(s, DELAY_US)
            for o in outs:
                o.fill_(7.0)
            for ds, o in zip(fed, outs):
                r = flo_amd.decode_streams(ds, out=o)
                got.append((r, r.out * 2.0))
        s.synchronize()
        assert w.launches > 0
        for (r, y), (ref, offs), tag in zip(got, want, ("first call", "second call")):
            assert np.array_equal(r.offsets, offs) and not r.status.any(), tag
            assert np.array_equal(y.cpu().numpy().view(np.uint32), (ref * 2.0).view(np.uint32)), tag + ", read behind it"
            assert np.array_equal(r.out.cpu().numpy().view(np.uint32), ref.view(np.uint32)), tag
    finally:
        flo_amd.debug_stream_delay(None)
        flo_amd.debug_pool_fill(None)
        for d in decs:
            d.close()


def _convert(b, which):
    if which == "resample":
        return b.resample(48000)
    return b.normalize(target_lufs=-16.0, limit=True)[0]


def _files(b):
    b.encode(0)
    b.sync()
    return [b.fetch(i) for i in range(b.n_clips)]


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("which", ["resample", "normalize"])
def test_a_conversion_is_ordered_by_a_sync_of_either_batch(ctx, which, fill):
    """flo_batch_resample / flo_batch_normalize only enqueue; flo_batch_sync on either batch orders the conversion"""
    first, second = S.batch_clips(), S.harsh_clips()
    lens = [x.size for x in first]

    def source(clips):
        b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, lens, S.SR, 2, 0.55)
        _raw_upload(b, clips)
        return b

    b = source(first)
    try:
        r = _convert(b, which)
        r.sync()
        want = _raw_pcm(r)
        r.close()
        _raw_upload(b, second)
        want_second = _files(b)
    finally:
        b.close()
    try:
        with late(fill) as w:
            # the source alone is synchronised, then the result is read
            b = source(first)
            r = _convert(b, which)
            b.sync()
            got = _raw_pcm(r)
            r.close()
            assert got == want, "the result, read after a sync of the source alone"
            # the result alone is synchronised, then the source is overwritten and encoded
            r = _convert(b, which)
            r.sync()
            _raw_upload(b, second)
            assert _files(b) == want_second, "the re-uploaded source's files"
            assert _raw_pcm(r) == want, "the result of the first source, after the source was overwritten"
            r.close()
            b.close()
            # the source is closed while the conversion is still queued
            b = source(first)
            r = _convert(b, which)
            b.close()
            got = [r.download_pcm(i).tobytes() for i in range(r.n_clips)]
            r.close()
            assert got == want, "the result, read after the source was closed behind the call"
        assert w.launches > 0
    finally:
        flo_amd.debug_stream_delay(None)
        flo_amd.debug_pool_fill(None)
        b.close()


def test_upload_encode_fetch_rounds(ctx):
    """Three rounds on one batch - uploads that nothing waits for, encode, sync, fetch, and the next round's uploads right
    behind - and flo_encode_batch over three chunks, whose pipeline (uploads on up_stream while the previous chunk encodes,
    downloads on down_stream) starts chunk k + 1's uploads as soon as chunk k's encode is queued and reuses both events of
    a chunk. (flo_batch_upload drops the batch's results, so on ONE batch the next uploads cannot start before the fetch:
    the overlap the pipeline has is flo_encode_batch's.)"""
    rounds = [S.batch_clips(), S.harsh_clips(), S.batch_clips(seed=90)]
    big = [S.noise(3_200_000, 2, 95 + i, 0.25) for i in range(3)]   # 25.6 MB each: two do not fit a chunk of 48 MB
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [x.size for x in rounds[0]], S.SR, 2, 0.55)
    try:
        want = []
        for clips in rounds:
            S._upload(b, clips)
            want.append(_files(b))
        want_big = ctx.encode_batch(flo_amd.MODE_LOSSY, big, S.SR, 2, 0.55)
        with late() as w:
            _raw_upload(b, rounds[0])
            for k in range(len(rounds)):
                got = _files(b)
                if k + 1 < len(rounds):
                    _raw_upload(b, rounds[k + 1])
                assert got == want[k], "round %d" % k
            got_big = ctx.encode_batch(flo_amd.MODE_LOSSY, big, S.SR, 2, 0.55)
        assert w.launches > 0
        assert [len(f) for f in got_big] == [len(f) for f in want_big]
        assert got_big == want_big, "flo_encode_batch over three chunks"
        # the fill off: under it each chunk's flo_batch_create and the pack buffer's pool_alloc wait for the whole device, which
        # all but serialises the three streams; off, chunk k + 1 uploads while chunk k encodes and chunk k - 1 comes down
        with late(None) as w:
            got_big = ctx.encode_batch(flo_amd.MODE_LOSSY, big, S.SR, 2, 0.55)
        assert w.launches > 0
        assert got_big == want_big, "flo_encode_batch over three chunks, the pool fill off"
    finally:
        flo_amd.debug_stream_delay(None)
        flo_amd.debug_pool_fill(None)
        b.close()


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
def test_decode_to_has_run_when_it_returns(ctx, fill):
    """Only this: with the library's own work late, Batch.decode_to has run when the call returns. The destination's
    earlier writer (a delayed fill on the caller's stream) is NOT late any more when the decode starts: flo_batch_decode
    takes no stream, so the caller orders the destination's earlier writers by waiting for its own stream (as for any
    pointer it hands over), which the test does. What the library owes is that a torch op behind the call, with no
    flo_batch_sync and no device synchronisation, sees the decoded values."""
    import torch
    cs = S.batch_clips()
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [x.size for x in cs], S.SR, 2, 0.55)
    try:
        S._upload(b, cs)
        b.encode(0)
        b.sync()
        n = sum(int(r["decoded_frames"]) for r in b.fidelity()) * b.channels
        dst = S._torch_full(n + 8, 7.0, torch.float32)
        offs = b.decode_to(dst.data_ptr(), dst.numel())
        torch.cuda.synchronize()
        want = dst.cpu().numpy()
        s = torch.cuda.Stream()
        with late(fill) as w, torch.cuda.stream(s):
            dst2 = torch.empty(n + 8, device="cuda:0")
            flo_amd.debug_delay_enqueue(s, DELAY_US)
            dst2.fill_(7.0)
            s.synchronize()
            assert b.decode_to(dst2.data_ptr(), dst2.numel()) == offs
            y = dst2 * 2.0
            got, got2 = dst2.cpu().numpy(), y.cpu().numpy()
        assert w.launches > 0
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(got2.view(np.uint32), (want * 2.0).view(np.uint32))
    finally:
        flo_amd.debug_stream_delay(None)
        flo_amd.debug_pool_fill(None)
        b.close()


def _analyse_behind_uploads(c, clips, fill=None, delayed=False):
    """analyze_all right behind uploads that nothing waits for -> (the record, whether the context's stream was still busy
    with them when analyze_all was called). The batch is made in front of the delay: its pool blocks are not what is
    under test."""
    b = flo_amd.Batch(c, flo_amd.MODE_LOSSY, [x.size for x in clips], S.SR, 2, 0.55)
    try:
        if not delayed:
            _raw_upload(b, clips)
            return [("analyze_all %d" % i, S.analysis_raw(a)) for i, a in enumerate(b.analyze_all(50))], False
        b.sync()
        with late(fill) as w:
            for _ in range(4):   # the uploads queue behind 4 D: late by more than the host needs to reach the fork
                flo_amd.debug_delay_enqueue(c.stream(), DELAY_US)
            _raw_upload(b, clips)
            busy = _hip().hipStreamQuery(c.stream()) == HIP_NOT_READY
            rec = [("analyze_all %d" % i, S.analysis_raw(a)) for i, a in enumerate(b.analyze_all(50))]
        return rec, busy, w.launches
    finally:
        flo_amd.debug_stream_delay(None)
        flo_amd.debug_pool_fill(None)
        b.close()


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("one_stream", [False, True])
def test_analyze_all_behind_uploads_nothing_waited_for(ctx, one_stream, fill):
    """The fork must wait for the late uploads and the read-back for all joins; with FLO_ANALYSIS_ONE_STREAM=1 (read when
    a context first analyses: a context of its own) everything runs on the context's stream.

    Which half each pass runs late: flo_batch_analyze_all takes its pool blocks before it records the fork, and under a
    fill each of them waits for the whole device, so under fill 0x7F the uploads have landed before any analysis work is
    queued and only the joins (delays behind the forks keep the side streams late) are run late. With the fill off nothing
    drains the device: the uploads are still queued when analyze_all is called - asserted, by hipStreamQuery - and a fork
    that waited for nothing would let the side streams read PCM that has not arrived."""
    import contextlib
    clips = S.batch_clips()
    c = ctx
    try:
        # (the variable is read at every analysis of a context that has no side streams yet: it stays set for both passes)
        with S.env("FLO_ANALYSIS_ONE_STREAM", "1") if one_stream else contextlib.nullcontext():
            if one_stream:
                c = flo_amd.Context(0)
            want, _ = _analyse_behind_uploads(c, clips)
            got, busy, launches = _analyse_behind_uploads(c, clips, fill, delayed=True)
        print("%s, fill %s: the stream was %s behind the uploads; %d delays" % ("one stream" if one_stream else "four streams", _fill_name(fill),
                                                                              "busy" if busy else "idle", launches))
        assert busy, "the uploads were not late when analyze_all was called"
        # four delays in front of the uploads and one in front of the launch; the four-stream form adds one behind each of
        # the three forks and one behind the joins, which also tells which form ran
        assert launches == 5 if one_stream else launches == 9, launches
        assert S.first_difference(want, got) is None, S.first_difference(want, got)
    finally:
        flo_amd.debug_stream_delay(None)
        flo_amd.debug_pool_fill(None)
        if c is not ctx:
            c.close()


_QUIET = {}


def _unrelated(ctx):
    """the scenario run behind every early close: one-shot lossy encodes (it takes blocks of many sizes from the pool)"""
    return S.lossy_encodes(ctx)


def _busy(ctx):
    return _hip().hipStreamQuery(ctx.stream()) == HIP_NOT_READY


# Each returns (the context's stream was busy right before the close, it was idle right behind it, what the object had
# produced for the caller). "idle right behind the close" is the host-side view of the wait in front of pool_free: every
# destroy releases its blocks in the call, so a destroy that did not wait would return with the stream still busy.
def _close_batch(ctx):
    cs = S.batch_clips()
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [x.size for x in cs], S.SR, 2, 0.55)
    _raw_upload(b, cs)
    b.encode(0)
    busy = _busy(ctx)
    b.close()
    return busy, not _busy(ctx), b""


def _close_ladder(ctx):
    cs = S.batch_clips()
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [x.size for x in cs], S.SR, 2, 0.55)
    try:
        _raw_upload(b, cs)
        lad = b.encode_ladder(S.LADDER5)
        busy = _busy(ctx)
        lad.close()
        return busy, not _busy(ctx), b""
    finally:
        b.close()


def _close_corpus(ctx):
    import torch
    c = flo_amd.Corpus(S._corpus_files(), ctx)
    fi, st1, _ = _corpus_calls(c)
    out = c.decode_windows(fi, st1, 1500)
    busy = _busy(ctx)
    c.close()
    idle = not _busy(ctx)
    torch.cuda.synchronize()
    return busy, idle, out.cpu().numpy().tobytes()


def _close_decoders(ctx):
    import torch
    ds = _fed(ctx, S._sdec_files_a())
    r = flo_amd.decode_streams(ds)
    busy = _busy(ctx)
    ds[0].close()
    idle = not _busy(ctx)
    ds[1].close()
    torch.cuda.synchronize()
    return busy, idle, r.out.cpu().numpy().tobytes()


def _close_index(ctx):
    ix = flo_amd.FingerprintIndex(S._fingerprints(300, 7), ctx)
    i, s = ix.topk_self(16)
    busy = _busy(ctx)
    ix.close()
    return busy, not _busy(ctx), S._b(i) + S._b(s)


# Ladder and FingerprintIndex have no asynchronous call: encode_ladder and the searches are complete on return, so nothing
# of theirs can be queued when they are closed and their destroys' waits cannot be run late by any caller.
QUEUES_WORK = dict(Batch=True, Ladder=False, Corpus=True, StreamingDecoder=True, FingerprintIndex=False)


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("what", ["Batch", "Ladder", "Corpus", "StreamingDecoder", "FingerprintIndex"])
def test_closing_an_object_with_work_queued(ctx, what, fill):
    """The object goes right behind its last call, with the device late.

    * What can see a destroy that does not wait in front of pool_free: the context's stream is busy right before the close
      (asserted for the objects that have an asynchronous call) and must be idle right behind it, and what the object had
      written for the caller must be what it writes quiet.
    * Then, as the issue words the early-free test, an unrelated scenario takes the blocks again and must give the quiet
      record. Under fill 0x7F the first block it takes waits for the whole device, and with the fill off the reuse is
      ordered by the one context stream, so this half alone could not fail; it is kept as the check that a late close
      leaves the pool and the context in order."""
    close = dict(Batch=_close_batch, Ladder=_close_ladder, Corpus=_close_corpus, StreamingDecoder=_close_decoders,
                 FingerprintIndex=_close_index)[what]
    try:
        if "quiet" not in _QUIET:
            _QUIET["quiet"] = _unrelated(ctx)
        if what not in _QUIET:
            _QUIET[what] = close(ctx)[2]
        with late(fill) as w:
            busy, idle, made = close(ctx)
            rec = _unrelated(ctx)
        print("%s, fill %s: busy before the close %s, idle behind it %s" % (what, _fill_name(fill), busy, idle))
        assert w.launches > 0
        if QUEUES_WORK[what]:
            assert busy, "nothing was queued when the object was closed"
        assert idle, "the context's stream was still busy when the close returned: its blocks went back to the pool in use"
        assert made == _QUIET[what], "what the closed object had written for the caller"
        diff = S.first_difference(_QUIET["quiet"], rec)
        assert diff is None, (what, diff)
    finally:
        flo_amd.debug_stream_delay(None)
        flo_amd.debug_pool_fill(None)

