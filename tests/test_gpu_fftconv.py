"""Partitioned FFT convolution on the device (flo_batch_convolve_fft, flo_convolve_fft and their Python faces) against
tests/fftconv_model.py under its yardstick: per output block and channel s_b = sum over p of ||segment b-p|| ||partition p||,
r = max over blocks of max|err| / s_b with err against the exact f64 convolution.

1. Per job, r_device <= max(3 r_model(job), floor): the floor is the largest r_model of the module's cases, computed in this
   process; the factor 3 stands for another butterfly order (radix-2 Stockham over B complex points and a real-FFT split,
   against scipy's pocketfft), FMA contraction in the accumulation and twiddle rounding. A wrong index, partition or twiddle
   costs three orders or more. Blocks of zero scale must be zero.
2. Bit for bit the same output for a job in the batch, alone through flo_convolve_fft, at another place in the list, and
   under a FLO_CONV_FFT_GROUP_BYTES that gives several groups and cuts a job.
3. A NaN planted in one clip changes no bit of any other job, nor of that job's blocks out of its reach.
4. Sources are unchanged. 5. method="auto" picks by crossover_taps. 6. Errors carry their message and leave no batch.
7. A filtered lossy batch goes on to encode, analyze_all and convolve. 8. The CLI.

No source is longer than 3 * lane_blocks * B + 5 frames, except one job of N = 20000, K = 16384. The module also runs the A
of tests/fftconv_recycled.py under every pool fill (the A, B, A sequence itself runs in tests/test_gpu_recycled_memory.py and
tests/test_gpu_late_streams.py, which find it registered because pytest imports this module first).

Seen on the device (B = 512, lane_blocks = 8; the floor, the largest r_model of the module, is 6.72e-8): the largest
r_device / r_model of a case is 1.43 (C 2, Ch 1), 1.39 (3, 1), 1.63 (3, 3), 1.72 (8, 1), 1.37 (8, 8), and 3.33 (1, 1) and 3.82
(2, 2) in the two cases with the sweeps, on jobs whose r_model lies far below the floor, so that the floor is their bound;
every job is inside max(3 r_model, floor).
Recorded once: a scratch build in which the cosine of twiddle k = 37 is multiplied by 1 + 2^-16 fails assertion 1 in all
seven cases, first at the K = 1 job of each: r_device 7.7e-8 to 1.0e-7 against max(3 * 1.9e-8 .. 2.4e-8, 6.72e-8)."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import fftconv_model as M
import fftconv_recycled
import flo_amd
import recycled_scenarios as S
from flo_amd import _native
from gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu
F32 = np.float32
RATE = 48000
CASES = [(1, 1), (2, 1), (2, 2), (3, 1), (3, 3), (8, 1), (8, 8)]
GEO = flo_amd.conv_fft_geometry(2, 1)
B, LB = GEO["block_frames"], GEO["lane_blocks"]


@functools.lru_cache(maxsize=None)
def _case(ch, ir_ch):
    """(src, irs, jobs, [(r_model, exact, scales) per job]) of one case: built once, never written"""
    src, irs, jobs = M.device_case(ch, ir_ch, B, LB, sweeps=(ch, ir_ch) in ((1, 1), (2, 2)), big=(ch, ir_ch) == (2, 1))
    ref = []
    for g in jobs:
        x, h = src[g["clip"]], irs[g["ir"]]
        exact, s = M.exact_clip(x, ch, h, ir_ch, g), M.scales(x, ch, h, ir_ch, g, B)
        r, zero_ok = M.ratio(M.model_clip(x, ch, h, ir_ch, g, B), exact, s, B)
        assert zero_ok and r <= M.R_CAP
        ref.append((r, exact, s))
    return src, irs, jobs, ref


@functools.lru_cache(maxsize=None)
def _floor():
    return max(r for c in CASES for r, _, _ in _case(*c)[3])


def _batch_of(ctx, clips, rate, ch, mode=flo_amd.MODE_LOSSLESS, q=0):
    b = flo_amd.Batch(ctx, mode, [x.size for x in clips], rate, ch, q)
    for i, x in enumerate(clips):
        ctx._chk(ctx._L.flo_batch_upload(b._h, i, np.ascontiguousarray(x, F32).ctypes.data))
    b.sync()
    return b


def _c_jobs(jobs):
    arr = (_native.ConvJob * max(len(jobs), 1))()
    for k, g in enumerate(jobs):
        arr[k] = _native.ConvJob(g["frames"], g["skip"], g["ir_start"], g["clip"], g["ir"], g["taps"], g["reserved"])
    return arr


def _raw(ctx, src, irs, jobs):
    """flo_batch_convolve_fft through the C ABI: (rc, handle)"""
    h = C.c_void_p(0xDEAD)
    rc = ctx._L.flo_batch_convolve_fft(src._h if src is not None else None, irs._h if irs is not None else None, len(jobs), _c_jobs(jobs), C.byref(h))
    return rc, h


def _run(ctx, src, irs, jobs):
    """every output clip of the list as downloaded arrays"""
    rc, h = _raw(ctx, src, irs, jobs)
    ctx._chk(rc)
    out = flo_amd.Batch(ctx, src._made[0], [g["frames"] * src.channels for g in jobs], src.sample_rate, src.channels, src._made[1], _handle=h)
    try:
        return [out.download_pcm(i) for i in range(out.n_clips)]
    finally:
        out.close()


def _raw_alone(ctx, x, h, rate, ch, ir_ch, g):
    x, h = np.ascontiguousarray(x, F32), np.ascontiguousarray(h, F32)
    out, n = C.c_void_p(0xDEAD), C.c_size_t(7)
    rc = ctx._L.flo_convolve_fft(ctx._h, x.ctypes.data, x.size, h.ctypes.data, h.size, rate, ch, ir_ch, _c_jobs([g]), C.byref(out), C.byref(n))
    return rc, out, n


def _alone(ctx, x, h, rate, ch, ir_ch, g):
    rc, out, n = _raw_alone(ctx, x, h, rate, ch, ir_ch, g)
    ctx._chk(rc)
    res = np.frombuffer(C.string_at(out.value, n.value * 4), F32).copy() if n.value else np.zeros(0, F32)
    ctx._L.flo_free(out)
    return res


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


class _GroupBytes:
    """FLO_CONV_FFT_GROUP_BYTES for the calls inside (the library reads it per call)"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("FLO_CONV_FFT_GROUP_BYTES")
        os.environ["FLO_CONV_FFT_GROUP_BYTES"] = str(self.value)

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["FLO_CONV_FFT_GROUP_BYTES"]
        else:
            os.environ["FLO_CONV_FFT_GROUP_BYTES"] = self.old


def test_the_cases_reach_what_they_claim():
    for ch, ir_ch in CASES:
        src, irs, jobs, _ = _case(ch, ir_ch)
        assert max(x.size // ch for x in src[:6]) <= 3 * LB * B + 5
        K = {M.taps_of(g["taps"], irs[g["ir"]].size // ir_ch, g["ir_start"]) for g in jobs}
        assert K >= {0, 1, B - 1, B, B + 1, 2 * B + 70, (LB + 1) * B + 1}
        assert {g["frames"] for g in jobs} >= {0, 1, B, B + 1, 3 * LB * B + 5}
        assert {src[g["clip"]].size // ch for g in jobs} >= {0, 1}
    assert any(g["frames"] == 20000 for g in _case(2, 1)[2])
    assert len(_case(1, 1)[2]) > 4 * B and len(_case(2, 2)[2]) > 4 * B   # the sweeps: every impulse position, every unit tap


@pytest.mark.parametrize("ch,ir_ch", CASES)
def test_batch_alone_elsewhere_and_grouped(ctx, ch, ir_ch):
    src, irs, jobs, ref = _case(ch, ir_ch)
    floor = _floor()
    lossy = ch == 2   # the source batch is a lossy one there
    a = _batch_of(ctx, src, RATE, ch, flo_amd.MODE_LOSSY if lossy else flo_amd.MODE_LOSSLESS, 0.55 if lossy else 0)
    b = _batch_of(ctx, irs, RATE, ir_ch)
    try:
        got = _run(ctx, a, b, jobs)
        worst = 0.0
        for k, g in enumerate(jobs):
            r_model, exact, s = ref[k]
            assert got[k].size == g["frames"] * ch
            r, zero_ok = M.ratio(got[k], exact, s, B)
            worst = max(worst, r / max(r_model, 1e-30) if r_model else 0.0)
            assert zero_ok, (ch, ir_ch, k, g, "a block of zero scale is not zero")
            assert r <= max(3 * r_model, floor), (ch, ir_ch, k, g, r, r_model, floor)
        print("C %d, Ch %d: largest r_device / r_model %.2f, floor %.2e" % (ch, ir_ch, worst, floor))
        # at another place in the list
        back = _run(ctx, a, b, jobs[::-1])[::-1]
        for k in range(len(jobs)):
            assert np.array_equal(_bits(back[k]), _bits(got[k])), (ch, ir_ch, "reversed list", k, jobs[k])
        # several groups and a cut job: a cap of lane_blocks + 2 segments
        cap_segs = LB + 2
        segs = [M.stored_segments(src[g["clip"]].size // ch, g["frames"], M.taps_of(g["taps"], irs[g["ir"]].size // ir_ch, g["ir_start"]), g["skip"], B)
                for g in jobs]
        assert max(segs) > 2 * cap_segs and sum(segs) > 3 * cap_segs   # the longest job is cut; three groups at least
        with _GroupBytes(cap_segs * ch * B * 8):
            grouped = _run(ctx, a, b, jobs)
        for k in range(len(jobs)):
            assert np.array_equal(_bits(grouped[k]), _bits(got[k])), (ch, ir_ch, "grouped", k, jobs[k])
        # alone (of the sweeps every 37th)
        plain = min(len(jobs), 31)
        for k in list(range(plain)) + list(range(plain, len(jobs), 37)):
            g = jobs[k]
            alone = _alone(ctx, src[g["clip"]], irs[g["ir"]], RATE, ch, ir_ch, dict(g, clip=0, ir=0))
            assert np.array_equal(_bits(alone), _bits(got[k])), (ch, ir_ch, "alone", k, g)
        for clips, batch in ((src, a), (irs, b)):   # the sources are unchanged
            for i, x in enumerate(clips):
                assert np.array_equal(_bits(batch.download_pcm(i)), _bits(x)), (ch, ir_ch, i)
    finally:
        a.close()
        b.close()


def test_a_unit_tap_moves_the_source(ctx):
    """h = [0 .. 0, 1] at every position 0 .. 2B: the output is the clip d frames later, to the yardstick's floor"""
    src, irs, jobs, _ = _case(1, 1)
    sweep = [g for g in jobs if g["ir"] == 2 and g["clip"] == 1]
    assert len(sweep) == 2 * B + 1
    a, b = _batch_of(ctx, src, RATE, 1), _batch_of(ctx, irs, RATE, 1)
    try:
        got = _run(ctx, a, b, sweep)
    finally:
        a.close()
        b.close()
    x = src[1].astype(np.float64)
    seen = set()
    for g, y in zip(sweep, got):
        d = 2 * B - g["ir_start"]           # the tap's position
        seen.add(d)
        t = np.arange(g["frames"]) + g["skip"] - d
        want = np.where((t >= 0) & (t < x.size), x[np.clip(t, 0, x.size - 1)], 0.0)
        # r <= max(3 r_model, floor) <= 3 floor, and s_b <= 0.3 sqrt(2B) * 1: a segment of samples below 0.3, one unit tap
        assert np.abs(y - want).max() <= 3 * _floor() * 0.3 * np.sqrt(2 * B), (d, float(np.abs(y - want).max()))
    assert seen >= set(range(2 * B + 1))


def test_a_nan_stays_within_its_reach(ctx):
    ch, ir_ch = 2, 1
    src, irs, jobs, _ = _case(ch, ir_ch)
    jobs = [g for g in jobs if g["frames"] != 20000]
    a, b = _batch_of(ctx, src, RATE, ch), _batch_of(ctx, irs, RATE, ir_ch)
    frame = 2 * LB * B + B // 2 + 3
    bad = np.array(src[0])
    bad[frame * ch + 1] = np.nan            # clip 0, channel 1
    c = _batch_of(ctx, [bad] + list(src[1:]), RATE, ch)
    try:
        clean, dirty = _run(ctx, a, b, jobs), _run(ctx, c, b, jobs)
    finally:
        for x in (a, b, c):
            x.close()
    touched = 0
    for k, g in enumerate(jobs):
        if g["clip"] != 0:
            assert np.array_equal(_bits(clean[k]), _bits(dirty[k])), ("another clip's job", k, g)
            continue
        T = g["frames"]
        K = M.taps_of(g["taps"], irs[g["ir"]].size // ir_ch, g["ir_start"])
        nb = -(-T // B)
        reach = set(M.reached_blocks(frame, g["skip"], src[0].size // ch, K, B, nb)) if K else set()
        x, y = clean[k].reshape(T, ch), dirty[k].reshape(T, ch)
        assert np.array_equal(_bits(x[:, 0]), _bits(y[:, 0])), ("the other channel", k, g)
        for blk in range(nb):
            if blk not in reach:
                assert np.array_equal(_bits(x[blk * B:(blk + 1) * B]), _bits(y[blk * B:(blk + 1) * B])), ("out of reach", k, g, blk)
        touched += bool(np.isnan(y).any())
    assert touched >= 3   # the planted value does arrive where the definition sends it


def test_auto_picks_by_the_crossover(ctx):
    cross = GEO["crossover_taps"]
    x = M.noise(3000, 2, 21)
    short, long_ = M.decay(cross - 1, 1, 22), M.decay(cross, 1, 23)
    a, b = _batch_of(ctx, [x], RATE, 2), _batch_of(ctx, [short, long_], RATE, 1)
    try:
        def run(ir, method):
            out = a.convolve(b, ir=ir, mode="full", method=method)
            try:
                return out.download_pcm(0)
            finally:
                out.close()
        for ir, fft in ((0, False), (1, True)):
            direct, by_fft, auto = run(ir, "direct"), run(ir, "fft"), run(ir, "auto")
            assert not np.array_equal(_bits(direct), _bits(by_fft))
            assert np.array_equal(_bits(auto), _bits(by_fft if fft else direct)), ir
            assert np.array_equal(_bits(run(ir, "direct")), _bits(a.convolve(b, ir=ir, mode="full").download_pcm(0)))   # the default
        assert np.array_equal(_bits(ctx.convolve(x, long_, RATE, 2, 1, mode="full", method="auto")), _bits(run(1, "fft")))
        assert np.array_equal(_bits(flo_amd.convolve(x, short, RATE, 2, 1, mode="full", method="auto")), _bits(run(0, "direct")))
        with pytest.raises(flo_amd.FloError, match="unknown method"):
            a.convolve(b, method="overlap-add")
    finally:
        a.close()
        b.close()


def test_taps_beyond_the_direct_limit(ctx):
    """K above FLO_CONV_MAX_TAPS: the direct path refuses, this one runs (a sparse response keeps the exact sum cheap)"""
    K = 65536 + 300
    h = np.zeros(K, F32)
    at = [0, 1, 4097, 65535, 65536, K - 1]
    h[at] = [0.5, -0.25, 0.125, 0.3, -0.2, 0.1]
    x = M.noise(700, 1, 31)
    g = M.job(0, 0, 700 + K - 1)
    got = _alone(ctx, x, h, RATE, 1, 1, g)
    want = np.zeros(700 + K - 1)
    for p in at:
        want[p:p + 700] += float(h[p]) * x.astype(np.float64)
    s = M.scales(x, 1, h, 1, g, B)
    r_model, model_ok = M.ratio(M.model_clip(x, 1, h, 1, g, B), want.reshape(-1, 1), s, B)
    r, zero_ok = M.ratio(got, want.reshape(-1, 1), s, B)
    assert model_ok and r_model <= M.R_CAP and zero_ok and r <= max(3 * r_model, _floor()), (r, r_model)
    with pytest.raises(flo_amd.FloError, match="FLO_CONV_MAX_TAPS"):
        ctx.convolve(x, h, RATE, 1)


def test_errors_leave_no_batch_and_a_usable_context(ctx):
    clips = [np.arange(20, dtype=F32), np.arange(8, dtype=F32)]
    big = 1 << 64
    src = _batch_of(ctx, clips, RATE, 2)
    irs = _batch_of(ctx, [np.ones(3, F32), np.zeros(0, F32), np.zeros(M.MAX_TAPS + 1, F32)], RATE, 1)
    wide = _batch_of(ctx, [np.zeros(6, F32)], RATE, 3)
    many = _batch_of(ctx, [np.zeros(18, F32)], RATE, 9)
    slow = _batch_of(ctx, [np.zeros(4, F32)], 44100, 1)
    empty = flo_amd.Batch(ctx, flo_amd.MODE_LOSSLESS, [8], RATE, 2, 0)
    empty_ir = flo_amd.Batch(ctx, flo_amd.MODE_LOSSLESS, [8], RATE, 1, 0)
    other_ctx = flo_amd.Context(0)
    try:
        foreign = _batch_of(other_ctx, [np.zeros(4, F32)], RATE, 1)
        most = (2 ** 64 - 1) // 8 // 2
        cases = [(src, irs, [M.job(2, 0, 4)], "clip 2"), (src, irs, [M.job(0, 3, 4)], "ir 3"), (src, irs, [M.job(0, 0, 4, reserved=1)], "reserved"),
                 (src, irs, [M.job(0, 2, 4)], "FLO_CONV_FFT_MAX_TAPS 1048576"), (src, irs, [M.job(0, 0, big - 3, skip=3)], "frames + skip"),
                 (src, irs, [M.job(0, 0, most + 1)], "frames "), (src, irs, [M.job(0, 0, 4), M.job(0, 0, 1 << 45)], "tiles"),
                 (src, None, [], "irs is NULL"), (None, irs, [], "src is NULL"), (src, wide, [M.job(0, 0, 4)], "ir_channels"),
                 (many, irs, [M.job(0, 0, 4)], "channels"), (src, slow, [M.job(0, 0, 4)], "resample"), (src, slow, [M.job(0, 0, 4)], "sample_rate"),
                 (src, foreign, [M.job(0, 0, 4)], "context")]
        for a, b, jobs, word in cases:
            rc, h = _raw(ctx, a, b, jobs)
            msg = ctx._L.flo_last_error(ctx._h).decode()
            assert rc == 1 and word in msg and msg.startswith("flo_batch_convolve_fft: "), (word, rc, msg)
            assert not h.value, word
            if a is src and b is irs and len(jobs) == 1 and jobs[0]["clip"] == 0 and jobs[0]["ir"] == 0:   # the same refusal through flo_convolve_fft
                rc, out, n = _raw_alone(ctx, clips[0], np.ones(3, F32), RATE, 2, 1, jobs[0])
                msg = ctx._L.flo_last_error(ctx._h).decode()
                assert rc == 1 and word.strip() in msg and msg.startswith("flo_convolve_fft: ") and not out.value and n.value == 0, (word, msg)
        for g, word in ((M.job(1, 0, 4), "clip 1"), (M.job(0, 1, 4), "ir 1")):   # flo_convolve_fft has one clip and one response
            rc, out, n = _raw_alone(ctx, clips[0], np.ones(3, F32), RATE, 2, 1, g)
            msg = ctx._L.flo_last_error(ctx._h).decode()
            assert rc == 1 and msg.startswith("flo_convolve_fft: " + word) and not out.value, msg
        rc, h = _raw(ctx, None, None, [])   # no batch: no context to carry a message
        assert rc == 1 and not h.value
        for a, b in ((empty, irs), (src, empty_ir)):   # a batch that a job names holds no PCM yet: FLO_ERR_STATE
            rc, h = _raw(ctx, a, b, [M.job(0, 0, 4)])
            assert rc != 0 and rc != 1 and "no PCM" in ctx._L.flo_last_error(ctx._h).decode() and not h.value
            rc, h = _raw(ctx, a, b, [])
            assert rc == 0
            ctx._L.flo_batch_destroy(h)
        with pytest.raises(flo_amd.FloError, match="no PCM"):
            empty.convolve(irs, method="fft")
        ok = _run(ctx, src, irs, [M.job(0, 0, 4, skip=1), M.job(1, 1, 3), M.job(1, 0, 5, ir_start=9)])   # the context still works
        assert np.abs(ok[0] - np.array([2, 4, 6, 9, 12, 15, 18, 21], F32)).max() < 1e-4 and not ok[1].any() and not ok[2].any()
        foreign.close()
    finally:
        other_ctx.close()
        for b in (src, irs, wide, many, slow, empty, empty_ir):
            b.close()


def _same_analysis(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y, equal_nan=True), k
        elif isinstance(x, float):
            assert x == y or (math.isnan(x) and math.isnan(y)), (k, x, y)
        else:
            assert x == y, (k, x, y)


def test_the_result_is_a_first_class_batch(ctx):
    """a filtered lossy batch against a batch of the same samples uploaded the usual way: the same files (so the padding
    behind the clips, pcm_written and the plan are right), the same analysis, the same convolved audio by either path"""
    rng = np.random.default_rng(34)
    sr, ch = 44100, 2
    lens = (6000, 1, 0, 2500, 1024)
    clips = [(rng.uniform(-0.5, 0.5, n * ch) * np.repeat(np.sin(np.arange(n) / 300.0) ** 2 + 0.05, ch)).astype(F32) for n in lens]
    irs = [M.decay(2 * B + 9, 1, 35), M.decay(300, 1, 36)]
    jobs = [M.job(0, 0, 6000, skip=31), M.job(0, 1, 6299), M.job(1, 1, 10), M.job(2, 0, 0), M.job(3, 1, 2500, ir_start=1, taps=200), M.job(4, 0, 1100, skip=3),
            M.job(2, 1, 700)]
    src = _batch_of(ctx, clips, sr, ch, flo_amd.MODE_LOSSY, 0.55)
    resp = _batch_of(ctx, irs, sr, 1)
    try:
        out = src.convolve(resp, jobs, method="fft")
        samples = [out.download_pcm(i) for i in range(out.n_clips)]
        up = _batch_of(ctx, samples, sr, ch, flo_amd.MODE_LOSSY, 0.55)
        try:
            assert out.n_interleaved == up.n_interleaved and out.channels == ch and out.sample_rate == sr
            for x, y in zip(out.analyze_all(), up.analyze_all()):
                _same_analysis(x, y)
            for method in ("direct", "fft"):
                ra, rb = out.convolve(resp, mode="full", ir=1, taps=40, method=method), up.convolve(resp, mode="full", ir=1, taps=40, method=method)
                try:
                    for i in range(ra.n_clips):
                        assert np.array_equal(_bits(ra.download_pcm(i)), _bits(rb.download_pcm(i))), (method, i)
                finally:
                    ra.close()
                    rb.close()
            out.encode()
            up.encode()
            out.sync()
            up.sync()
            for i in range(out.n_clips):
                assert out.fetch(i) == up.fetch(i), i
        finally:
            out.close()
            up.close()
    finally:
        src.close()
        resp.close()


def test_cli_convolve_takes_the_method(ctx, tmp_path):
    from flo_amd import cli
    from flo_amd.wav import read_wav_bytes, write_wav_bytes
    cross = GEO["crossover_taps"]
    rng = np.random.default_rng(3)
    a, h = rng.uniform(-0.2, 0.2, 2 * 6000).astype(F32), M.decay(cross + 5, 1, 8)
    wa, wh, outp = (tmp_path / n for n in ("a.wav", "h.wav", "out.wav"))
    wa.write_bytes(write_wav_bytes(a, RATE, 2))
    wh.write_bytes(write_wav_bytes(h, RATE, 1))
    sa, sh = (np.ascontiguousarray(read_wav_bytes(p.read_bytes())[0], F32) for p in (wa, wh))
    for tail, mode in ((False, "head"), (True, "full")):
        want = {m: ctx.convolve(sa, sh, RATE, 2, 1, mode=mode, method=m) for m in ("direct", "fft")}
        assert not np.array_equal(_bits(want["direct"]), _bits(want["fft"]))
        for method, key in ((None, "direct"), ("direct", "direct"), ("fft", "fft"), ("auto", "fft")):
            assert cli.main(["convolve", str(wa), str(wh), str(outp)] + (["--tail"] if tail else []) + (["--method", method] if method else [])) == 0
            got, rate, ch = read_wav_bytes(outp.read_bytes())
            assert (rate, ch) == (RATE, 2) and np.array_equal(_bits(got), _bits(want[key])), (mode, method)


def test_the_scenario_under_every_fill(ctx):
    """A of tests/fftconv_recycled.py with the switch off and under every fill, in the shape of test_fill"""
    assert "fftconv" in [s["name"] for s in S.LEFTOVERS]
    records = []
    try:
        for fill in S.FILLS:
            flo_amd.debug_pool_fill(fill)
            records.append(fftconv_recycled.fftconv_a(ctx))
    finally:
        flo_amd.debug_pool_fill(None)
    for fill, rec in zip(S.FILLS[1:], records[1:]):
        diff = S.first_difference(records[0], rec)
        assert diff is None, ("fftconv", "fill %s against the switch off" % ("off" if fill is None else hex(fill)), diff)
