"""FIR filtering and convolution on the device (flo_batch_convolve, flo_convolve and their Python faces) against
tests/convolve_model.py, bit for bit: uint32 views are compared, samples that are NaN on both sides match by position. Every
output clip is checked in its batch and alone through flo_convolve. No source clip is longer than 3 tile_frames + 5 frames
(flo_conv_geometry), and long responses are kept to a handful of jobs: the model's work for one test, the sum of K * T * C
over the jobs, stays near 1e8. The module also runs the A of tests/convolve_recycled.py under every pool fill (the A, B, A
sequence itself runs in tests/test_gpu_recycled_memory.py and tests/test_gpu_late_streams.py, which find it registered
because pytest imports this module first)."""
import ctypes as C
import math

import numpy as np
import pytest

import convolve_model as M
import convolve_recycled
import mix_model
import flo_amd
import recycled_scenarios as S
from flo_amd import _native
from gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu
F32 = np.float32
RATE = 48000


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
    """flo_batch_convolve through the C ABI: (rc, handle)"""
    h = C.c_void_p(0xDEAD)
    rc = ctx._L.flo_batch_convolve(src._h if src is not None else None, irs._h if irs is not None else None, len(jobs), _c_jobs(jobs), C.byref(h))
    return rc, h


def _conv_batch(ctx, src, irs, jobs):
    rc, h = _raw(ctx, src, irs, jobs)
    ctx._chk(rc)
    return flo_amd.Batch(ctx, src._made[0], [g["frames"] * src.channels for g in jobs], src.sample_rate, src.channels, src._made[1], _handle=h)


def _raw_alone(ctx, x, h, rate, ch, ir_ch, g):
    x, h = np.ascontiguousarray(x, F32), np.ascontiguousarray(h, F32)
    out, n = C.c_void_p(0xDEAD), C.c_size_t(7)
    rc = ctx._L.flo_convolve(ctx._h, x.ctypes.data, x.size, h.ctypes.data, h.size, rate, ch, ir_ch, _c_jobs([g]), C.byref(out), C.byref(n))
    return rc, out, n


def _alone(ctx, x, h, rate, ch, ir_ch, g):
    rc, out, n = _raw_alone(ctx, x, h, rate, ch, ir_ch, g)
    ctx._chk(rc)
    res = np.frombuffer(C.string_at(out.value, n.value * 4), F32).copy() if n.value else np.zeros(0, F32)
    ctx._L.flo_free(out)
    return res


def _download_all(b):
    return [b.download_pcm(i) for i in range(b.n_clips)]


def test_the_model_has_the_geometry_in_force():
    for ch, ir_ch in ((1, 1), (2, 1), (2, 2), (3, 1), (3, 3), (8, 1), (8, 8)):
        assert flo_amd.conv_geometry(ch, ir_ch) == dict(tile_frames=M.TILE, tap_chunk=M.CHUNK, lane_outputs=M.LANE)


@pytest.mark.parametrize("ch,ir_ch", [(1, 1), (2, 1), (2, 2), (3, 1), (3, 3), (8, 1), (8, 8)])
def test_batch_and_alone_equal_the_model(ctx, ch, ir_ch):
    src, irs, jobs = M.device_case(ch, ir_ch)
    assert M.case_paths(src, irs, jobs, ch, ir_ch) >= M.expected_paths(ch, ir_ch)
    assert max(x.size // ch for x in src) <= 3 * M.TILE + 5 and M.work(src, irs, jobs, ch, ir_ch) < 2e8
    want = M.convolve(src, ch, irs, ir_ch, jobs, strict=True)
    lossy = ch == 2   # the source batch is a lossy one there
    a = _batch_of(ctx, src, RATE, ch, flo_amd.MODE_LOSSY if lossy else flo_amd.MODE_LOSSLESS, 0.55 if lossy else 0)
    b = _batch_of(ctx, irs, RATE, ir_ch)
    try:
        out = _conv_batch(ctx, a, b, jobs)
        try:
            got = _download_all(out)
            assert out.n_interleaved == [g["frames"] * ch for g in jobs]
        finally:
            out.close()
        for k, g in enumerate(jobs):
            assert M.same(got[k], want[k]) is None, (ch, ir_ch, "batch", k, g, M.same(got[k], want[k]))
        for k, g in enumerate(jobs):
            alone = _alone(ctx, src[g["clip"]], irs[g["ir"]], RATE, ch, ir_ch, dict(g, clip=0, ir=0))
            assert M.same(alone, want[k]) is None, (ch, ir_ch, "alone", k, g, M.same(alone, want[k]))
        for clips, batch in ((src, a), (irs, b)):   # the sources are unchanged
            for i, x in enumerate(clips):
                assert np.array_equal(batch.download_pcm(i).view(np.uint32), x.view(np.uint32)), (ch, ir_ch, i)
    finally:
        a.close()
        b.close()


def test_a_batch_as_its_own_response(ctx):
    """irs == src: clips of one batch filtered by clips of the same batch"""
    ch = 2
    clips = [M.noise(M.TILE + 7, ch, 70, M.SOURCE_EDGES), (M.noise(M.CHUNK + 5, ch, 71) * F32(0.25)).astype(F32), M.noise(3, ch, 72)]
    jobs = [M.job(0, 1, M.TILE + 7), M.job(0, 2, M.TILE + 9, skip=1), M.job(1, 1, 2 * M.CHUNK + 9), M.job(2, 0, 40, taps=M.LANE + 1), M.job(0, 0, 50, taps=20)]
    want = M.convolve(clips, ch, clips, ch, jobs, strict=True)
    b = _batch_of(ctx, clips, RATE, ch)
    try:
        out = _conv_batch(ctx, b, b, jobs)
        try:
            for k, y in enumerate(_download_all(out)):
                assert M.same(y, want[k]) is None, (k, M.same(y, want[k]))
        finally:
            out.close()
        for i, x in enumerate(clips):
            assert np.array_equal(b.download_pcm(i).view(np.uint32), x.view(np.uint32)), i
    finally:
        b.close()


def test_denormals_stay_inside_the_flush_allowance(ctx):
    """One clip of denormals under taps of |h| <= 1. Held only to |got - want| <= K * 2^-126: what a device that flushes
    denormal inputs or results to zero may lose per FMA."""
    ch, K = 2, M.CHUNK + 9
    x = (mix_model.plain(M.TILE + 9, ch, 5) * F32(2.0 ** -130)).astype(F32)
    assert ((np.abs(x) < 2.0 ** -126) & (x != 0)).all()
    h = np.random.default_rng(6).uniform(-1, 1, K).astype(F32)
    g = M.job(0, 0, M.TILE + 9, skip=4)
    want, _ = M.convolve_clip(x, ch, h, 1, g)
    got = _alone(ctx, x, h, RATE, ch, 1, g)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert (err <= K * 2.0 ** -126).all(), float(err.max())


def test_filter_equals_design_upload_and_convolve(ctx):
    ch = 2
    clips = [mix_model.plain(n, ch, 80 + i) for i, n in enumerate((M.TILE + 300, 0, 1, 700))]
    b = _batch_of(ctx, clips, RATE, ch)
    try:
        for kind, lo, hi, taps, beta in (("lowpass", None, 4000.0, 255, 9.0), ("bandstop", 900.0, 1100.0, 101, 6.0), ("highpass", 80.0, None, 31, 9.0)):
            table = flo_amd.fir_design(kind, RATE, lo, hi, taps, beta)
            assert table.dtype == F32 and table.size == taps
            out = b.filter(kind, lo, hi, taps, beta)
            irs = _batch_of(ctx, [table], RATE, 1)
            by_hand = b.convolve(irs, mode="centered")
            try:
                for i, x in enumerate(clips):
                    want, _ = M.convolve_clip(x, ch, table, 1, M.mode_job("centered", x.size // ch, taps))
                    assert M.same(out.download_pcm(i), by_hand.download_pcm(i)) is None, (kind, i)
                    assert M.same(out.download_pcm(i), want) is None, (kind, i, M.same(out.download_pcm(i), want))
            finally:
                out.close()
                by_hand.close()
                irs.close()
        one = flo_amd.fir_filter(clips[3], RATE, ch, "lowpass", f_hi=4000.0)
        want, _ = M.convolve_clip(clips[3], ch, flo_amd.fir_design("lowpass", RATE, f_hi=4000.0), 1, M.mode_job("centered", 700, 255))
        assert M.same(one, want) is None
    finally:
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
    """a filtered lossy batch against a batch of the model's output uploaded the usual way: the same files (so the padding
    behind the clips, pcm_written and the plan are right), the same analysis, the same resampled, normalised, edited and
    mixed audio"""
    rng = np.random.default_rng(34)
    sr, ch = 44100, 2
    lens = (6000, 1, 0, 2500, 1024)
    clips = [(rng.uniform(-0.5, 0.5, n * ch) * np.repeat(np.sin(np.arange(n) / 300.0) ** 2 + 0.05, ch)).astype(F32) for n in lens]
    irs = [flo_amd.fir_design("lowpass", sr, f_hi=5000.0, taps=63), (rng.uniform(-0.2, 0.2, 300) * np.exp(-np.arange(300) / 60.0)).astype(F32)]
    jobs = [M.job(0, 0, 6000, skip=31), M.job(0, 1, 6299), M.job(1, 1, 10), M.job(2, 0, 0), M.job(3, 1, 2500, ir_start=1, taps=200), M.job(4, 0, 1100, skip=3),
            M.job(2, 1, 700)]
    src = _batch_of(ctx, clips, sr, ch, flo_amd.MODE_LOSSY, 0.55)
    resp = _batch_of(ctx, irs, sr, 1)
    try:
        out = src.convolve(resp, jobs)
        want = M.convolve(clips, ch, irs, 1, jobs, strict=True)
        up = _batch_of(ctx, want, sr, ch, flo_amd.MODE_LOSSY, 0.55)
        try:
            assert out.n_interleaved == up.n_interleaved and out.channels == ch and out.sample_rate == sr
            for a, b in zip(out.analyze_all(), up.analyze_all()):
                _same_analysis(a, b)
            steps = {"resample": lambda s: s.resample(48000), "normalize": lambda s: s.normalize(target_lufs=-20.0)[0],
                     "edit": lambda s: s.edit([dict(clip=0, start=7, frames=3000, pad_head=2, fade_in=9), dict(clip=4)]),
                     "mix": lambda s: s.mix([dict(out=0, clip=0, gain=0.7), dict(out=0, clip=1, at=100, gain=0.3)]),
                     "convolve": lambda s: s.convolve(resp, mode="full", ir=1, taps=40)}
            for which, step in steps.items():
                ra, rb = step(out), step(up)
                try:
                    for i in range(ra.n_clips):
                        assert M.same(ra.download_pcm(i), rb.download_pcm(i)) is None, (which, i)
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


def test_errors_leave_no_batch_and_a_usable_context(ctx):
    clips = [np.arange(20, dtype=F32), np.arange(8, dtype=F32)]
    big = 1 << 64
    src = _batch_of(ctx, clips, RATE, 2)
    irs = _batch_of(ctx, [np.ones(3, F32), np.zeros(0, F32)], RATE, 1)
    wide = _batch_of(ctx, [np.zeros(6, F32)], RATE, 3)
    many = _batch_of(ctx, [np.zeros(18, F32)], RATE, 9)
    slow = _batch_of(ctx, [np.zeros(4, F32)], 44100, 1)
    empty = flo_amd.Batch(ctx, flo_amd.MODE_LOSSLESS, [8], RATE, 2, 0)
    empty_ir = flo_amd.Batch(ctx, flo_amd.MODE_LOSSLESS, [8], RATE, 1, 0)
    other_ctx = flo_amd.Context(0)
    try:
        foreign = _batch_of(other_ctx, [np.zeros(4, F32)], RATE, 1)
        most = (2 ** 64 - 1) // 8 // 2
        cases = [(src, irs, [M.job(2, 0, 4)], "clip 2"), (src, irs, [M.job(0, 2, 4)], "ir 2"), (src, irs, [M.job(0, 0, 4, reserved=1)], "reserved"),
                 (src, irs, [M.job(0, 0, big - 3, skip=3)], "frames + skip"), (src, irs, [M.job(0, 0, most + 1)], "frames "),
                 (src, irs, [M.job(0, 0, 4), M.job(0, 0, 1 << 45)], "tiles"), (src, None, [], "irs is NULL"), (None, irs, [], "src is NULL"),
                 (src, wide, [M.job(0, 0, 4)], "ir_channels"), (many, irs, [M.job(0, 0, 4)], "channels"), (src, slow, [M.job(0, 0, 4)], "resample"),
                 (src, slow, [M.job(0, 0, 4)], "sample_rate"), (src, foreign, [M.job(0, 0, 4)], "context")]
        for a, b, jobs, word in cases:
            rc, h = _raw(ctx, a, b, jobs)
            msg = ctx._L.flo_last_error(ctx._h).decode()
            assert rc == 1 and word in msg and msg.startswith("flo_batch_convolve: "), (word, rc, msg)
            assert not h.value, word
            if a is src and b is irs and len(jobs) == 1 and jobs[0]["clip"] == 0 and jobs[0]["ir"] == 0:   # the same refusal through flo_convolve
                rc, out, n = _raw_alone(ctx, clips[0], np.ones(3, F32), RATE, 2, 1, jobs[0])
                msg = ctx._L.flo_last_error(ctx._h).decode()
                assert rc == 1 and word.strip() in msg and msg.startswith("flo_convolve: ") and not out.value and n.value == 0, (word, msg)
        for g, word in ((M.job(1, 0, 4), "clip 1"), (M.job(0, 1, 4), "ir 1")):   # flo_convolve has one clip and one response
            rc, out, n = _raw_alone(ctx, clips[0], np.ones(3, F32), RATE, 2, 1, g)
            msg = ctx._L.flo_last_error(ctx._h).decode()
            assert rc == 1 and msg.startswith("flo_convolve: " + word) and not out.value, msg
        rc, out, n = _raw_alone(ctx, clips[0], np.ones(6, F32), RATE, 2, 3, M.job(0, 0, 4))
        assert rc == 1 and "ir_channels" in ctx._L.flo_last_error(ctx._h).decode() and not out.value
        rc, h = _raw(ctx, None, None, [])   # no batch: no context to carry a message
        assert rc == 1 and not h.value
        # a batch that a job names holds no PCM yet: FLO_ERR_STATE; with no job it does not matter
        for a, b in ((empty, irs), (src, empty_ir)):
            rc, h = _raw(ctx, a, b, [M.job(0, 0, 4)])
            assert rc != 0 and rc != 1 and "no PCM" in ctx._L.flo_last_error(ctx._h).decode() and not h.value
            rc, h = _raw(ctx, a, b, [])
            assert rc == 0
            ctx._L.flo_batch_destroy(h)
        with pytest.raises(flo_amd.FloError, match="no PCM"):
            empty.convolve(irs)
        ok = _conv_batch(ctx, src, irs, [M.job(0, 0, 4, skip=1), M.job(1, 1, 3), M.job(1, 0, 5, ir_start=9)])   # the context still works
        assert ok.download_pcm(0).tolist() == [2, 4, 6, 9, 12, 15, 18, 21] and not ok.download_pcm(1).view(np.uint32).any()
        assert not ok.download_pcm(2).view(np.uint32).any()
        ok.close()
        foreign.close()
    finally:
        other_ctx.close()
        for b in (src, irs, wide, many, slow, empty, empty_ir):
            b.close()


def test_python_faces_modes_and_defaults(ctx):
    rng = np.random.default_rng(5)
    x = rng.uniform(-0.9, 0.9, 3000 * 2).astype(F32)
    odd = rng.uniform(-0.1, 0.1, 1001).astype(F32)   # an odd count: the partial frame is not part of the clip
    h0, h1 = rng.uniform(-0.3, 0.3, 9).astype(F32), rng.uniform(-0.3, 0.3, 40).astype(F32)
    b = _batch_of(ctx, [x, odd, np.zeros(0, F32)], RATE, 2)
    irs = _batch_of(ctx, [h0, h1, np.zeros(0, F32)], RATE, 1)
    try:
        for mode in ("head", "full", "centered"):
            for ir, taps in ((0, None), ([1, 0, 1], None), (1, 5), (2, None)):
                out = b.convolve(irs, ir=ir, mode=mode, taps=taps)
                try:
                    for i, clip in enumerate((x, odd, np.zeros(0, F32))):
                        j = ir[i] if isinstance(ir, list) else ir
                        k = min((h0, h1, np.zeros(0, F32))[j].size, M.ALL if taps is None else taps)
                        g = M.mode_job(mode, clip.size // 2, k, taps=M.ALL if taps is None else taps)
                        want, _ = M.convolve_clip(clip, 2, (h0, h1, np.zeros(0, F32))[j], 1, g)
                        assert out.n_interleaved[i] == want.size and M.same(out.download_pcm(i), want) is None, (mode, ir, taps, i)
                finally:
                    out.close()
        out = b.convolve(irs, [dict(clip=0, ir=1, skip=3, frames=100, ir_start=2, taps=7), _native.ConvJob(5, 0, 0, 1, 0, M.ALL, 0), dict(clip=1)])
        try:
            assert out.n_interleaved == [200, 10, 1000]
            want = M.convolve([x, odd], 2, [h0, h1], 1, [M.job(0, 1, 100, 3, 2, 7), M.job(1, 0, 5), M.job(1, 0, 500)])
            for k in range(3):
                assert M.same(out.download_pcm(k), want[k]) is None, k
        finally:
            out.close()
        none = b.convolve(irs, [])
        assert none.n_clips == 0
        none.close()
        with pytest.raises(flo_amd.FloError, match="unknown keys"):
            b.convolve(irs, [dict(clip=0, gain=3)])
        with pytest.raises(flo_amd.FloError, match="unknown mode"):
            b.convolve(irs, mode="tail")
    finally:
        b.close()
        irs.close()
    one = ctx.convolve(x, h1, RATE, 2, 1, mode="full")
    assert one.size == 3039 * 2 and M.same(one, M.convolve_clip(x, 2, h1, 1, M.mode_job("full", 3000, 40))[0]) is None
    assert M.same(flo_amd.convolve(x, [1.0], RATE, 2), x) is None      # h = [1] reproduces the source (no -0.0 in it)
    assert M.same(ctx.convolve(x, h0, RATE, 2, 1, dict(frames=50, skip=2)), M.convolve_clip(x, 2, h0, 1, M.job(0, 0, 50, 2))[0]) is None
    assert ctx.convolve(np.zeros(0, F32), h0, RATE, 2).size == 0 and not ctx.convolve(x, np.zeros(0, F32), RATE, 2).view(np.uint32).any()


def test_cli_filter_and_convolve(ctx, tmp_path, capsys):
    from flo_amd import cli
    from flo_amd.wav import read_wav_bytes, write_wav_bytes
    rng = np.random.default_rng(3)
    a, h = rng.uniform(-0.2, 0.2, 2 * 6000).astype(F32), (rng.uniform(-0.2, 0.2, 500) * np.exp(-np.arange(500) / 80.0)).astype(F32)
    wa, wh, outp, slow, wide = (tmp_path / n for n in ("a.wav", "h.wav", "out.wav", "slow.wav", "wide.wav"))
    wa.write_bytes(write_wav_bytes(a, RATE, 2))
    wh.write_bytes(write_wav_bytes(h, RATE, 1))
    slow.write_bytes(write_wav_bytes(h, 44100, 1))
    wide.write_bytes(write_wav_bytes(a, RATE, 2))
    sa, sh = (np.ascontiguousarray(read_wav_bytes(p.read_bytes())[0], F32) for p in (wa, wh))
    assert cli.main(["filter", str(wa), str(outp), "--bandpass", "300,3400", "--taps", "127"]) == 0
    got, rate, ch = read_wav_bytes(outp.read_bytes())
    table = flo_amd.fir_design("bandpass", RATE, 300.0, 3400.0, 127)
    want, _ = M.convolve_clip(sa, 2, table, 1, M.mode_job("centered", 6000, 127))
    assert (rate, ch) == (RATE, 2) and M.same(np.ascontiguousarray(got, F32), want) is None
    for tail, mode in ((False, "head"), (True, "full")):
        assert cli.main(["convolve", str(wa), str(wh), str(outp)] + (["--tail"] if tail else [])) == 0
        got, rate, ch = read_wav_bytes(outp.read_bytes())
        want, _ = M.convolve_clip(sa, 2, sh, 1, M.mode_job(mode, 6000, 500))
        assert (rate, ch) == (RATE, 2) and M.same(np.ascontiguousarray(got, F32), want) is None, mode
    assert cli.main(["convolve", str(wa), str(slow), str(outp)]) != 0
    assert "resample" in capsys.readouterr().err
    assert cli.main(["convolve", str(wh), str(wide), str(outp)]) != 0   # a stereo response on a mono input
    assert "edit" in capsys.readouterr().err
    assert cli.main(["filter", str(wa), str(outp), "--lowpass", "30000"]) != 0
    assert "f_hi" in capsys.readouterr().err


def test_the_scenario_under_every_fill(ctx):
    """A of tests/convolve_recycled.py with the switch off and under every fill, in the shape of test_fill"""
    assert "convolve" in [s["name"] for s in S.LEFTOVERS]
    records = []
    try:
        for fill in S.FILLS:
            flo_amd.debug_pool_fill(fill)
            records.append(convolve_recycled.convolve_a(ctx))
    finally:
        flo_amd.debug_pool_fill(None)
    for fill, rec in zip(S.FILLS[1:], records[1:]):
        diff = S.first_difference(records[0], rec)
        assert diff is None, ("convolve", "fill %s against the switch off" % ("off" if fill is None else hex(fill)), diff)
