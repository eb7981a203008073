"""Loudness normalisation and true-peak limiting on the device (flo_batch_true_peak, flo_batch_normalize, flo_normalize and
their Python faces) against tests/normalize_model.py, bit for bit: every output sample (-0.0, NaN positions and infinities
included), every true peak and every report. The model takes what the device measured of the source clip - integrated
loudness and sample peak, from the batched analysis, which has tests of its own - and restates everything behind it.
Every clip is checked in its mixed batch and alone through flo_normalize. The cases are normalize_model.cases()."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import flo_amd
import normalize_model as M
import normalize_recycled
from flo_amd import _native
from gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu


def _opts(case):
    return _native.NormalizeOpts(case["target"], case["ceiling"], case["max_gain_db"], case["mode"], case["lookahead_frames"])


def _batch_of(ctx, clips, rate, ch, mode=flo_amd.MODE_LOSSLESS, q=0):
    b = flo_amd.Batch(ctx, mode, [x.size for x in clips], rate, ch, q)
    for i, x in enumerate(clips):
        ctx._chk(ctx._L.flo_batch_upload(b._h, i, x.ctypes.data))
    b.sync()
    return b


def _normalize_batch(ctx, b, opts):
    """flo_batch_normalize through the C ABI: (the new Batch, the raw reports)"""
    h = C.c_void_p()
    reps = (_native.NormalizeReport * max(b.n_clips, 1))()
    ctx._chk(ctx._L.flo_batch_normalize(b._h, C.byref(opts), C.byref(h), reps))
    lens = [n // b.channels * b.channels for n in b.n_interleaved]
    return flo_amd.Batch(ctx, b._made[0], lens, b.sample_rate, b.channels, b._made[1], _handle=h), reps


def _normalize_alone(ctx, x, rate, ch, opts):
    out, rep = C.c_void_p(), _native.NormalizeReport()
    ctx._chk(ctx._L.flo_normalize(ctx._h, x.ctypes.data, x.size, rate, ch, C.byref(opts), C.byref(out), C.byref(rep)))
    n = x.size // ch * ch
    res = np.frombuffer(C.string_at(out.value, n * 4), np.float32).copy() if n else np.zeros(0, np.float32)
    ctx._L.flo_free(out)
    return res, rep


def _f64_same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _check_report(got, want, tag):
    assert got.status == want["status"], (tag, got.status, want["status"])
    assert np.float32(got.input_true_peak).view(np.uint32) == np.float32(want["input_true_peak"]).view(np.uint32), (tag, got.input_true_peak, want["input_true_peak"])
    assert np.float32(got.gain).view(np.uint32) == np.float32(want["gain"]).view(np.uint32), (tag, got.gain, want["gain"])
    for k in ("input_lufs", "input_true_peak_dbtp", "gain_db", "ceiling_reduction_db"):
        assert _f64_same(getattr(got, k), want[k]), (tag, k, getattr(got, k), want[k])
    assert (got.limited_frames, got.min_gain_q24) == (want["limited_frames"], want["min_gain_q24"]), (tag, got.limited_frames, got.min_gain_q24, want)


def _first_difference(got, want):
    d = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    return None if not d.size else "%d of %d samples differ, the first at %d: %r against %r" % (d.size, got.size, d[0], got[d[0]], want[d[0]])


@pytest.mark.parametrize("case", M.cases(), ids=lambda c: c["name"])
def test_batch_and_alone_equal_the_model(ctx, case):
    rate, ch = case["rate"], case["ch"]
    clips = [x for _, x in case["clips"]]
    opts = _opts(case)
    src = _batch_of(ctx, clips, rate, ch)
    try:
        measured = src.analyze_all()
        peaks = src.true_peaks(linear=True)
        out, reps = _normalize_batch(ctx, src, opts)
        try:
            limited = 0
            for i, (name, x) in enumerate(case["clips"]):
                tag = (case["name"], name)
                want, rep, _ = M.normalize(x, ch, rate, measured[i]["integrated_lufs"], measured[i]["sample_peak_dbfs"], case["target"], case["ceiling"],
                                           case["mode"], case["lookahead_frames"], case["max_gain_db"])
                assert peaks[i].view(np.uint32) == M.true_peak(x, ch).view(np.uint32), (tag, peaks[i], M.true_peak(x, ch))
                got = out.download_pcm(i)
                assert got.size == want.size and _first_difference(got, want) is None, (tag, "batch", _first_difference(got, want))
                _check_report(reps[i], rep, tag)
                alone, arep = _normalize_alone(ctx, x, rate, ch, opts)
                assert _first_difference(alone, want) is None, (tag, "alone", _first_difference(alone, want))
                _check_report(arep, rep, tag + ("alone",))
                limited += rep["limited_frames"]
                # the source is unchanged
                assert np.array_equal(src.download_pcm(i).view(np.uint32), x.view(np.uint32)), tag
            if case["mode"] == M.LIMIT and case["name"] not in ("skip_bound",):
                assert limited > 0, (case["name"], "no frame of the case was limited")
        finally:
            out.close()
    finally:
        src.close()


@pytest.mark.parametrize("rate,ch", M.RESAMPLER_SHAPES)
def test_true_peaks_are_the_resampler_at_four_times_the_rate(ctx, rate, ch):
    """max(max |x|, max |Batch.resample(4 rate)|), on the device itself: the envelope is that conversion's output"""
    clips = M.resampler_clips(rate, ch)
    b = _batch_of(ctx, clips, rate, ch)
    try:
        lin = b.true_peaks(linear=True)
        db = b.true_peaks()
        up = b.resample(4 * rate)
        try:
            for i, x in enumerate(clips):
                y = up.download_pcm(i)
                want = np.float32(max(np.abs(x).max(initial=0), np.abs(y).max(initial=0)))
                assert lin[i].view(np.uint32) == want.view(np.uint32), (i, lin[i], want)
                assert lin[i].view(np.uint32) == M.true_peak(x, ch).view(np.uint32)
                assert db[i] == (20.0 * math.log10(float(want)) if want > 1e-9 else -150.0)
        finally:
            up.close()
    finally:
        b.close()
    assert ctx.true_peak(clips[-1], rate, ch) == db[-1] == flo_amd.true_peak(clips[-1], rate, ch)


def test_long_path_equals_short_path(ctx):
    """tiles that take the short path give the same bits as the long path: the whole case again with FLO_NORM_NO_SKIP set"""
    by = {c["name"]: c for c in M.cases()}
    for name in ("skip_bound", "gain_x2", "ragged_64"):
        case = by[name]
        clips = [x for _, x in case["clips"]]
        src = _batch_of(ctx, clips, case["rate"], case["ch"])
        try:
            runs = []
            for env in (None, "1"):
                if env is None:
                    os.environ.pop("FLO_NORM_NO_SKIP", None)
                else:
                    os.environ["FLO_NORM_NO_SKIP"] = env
                try:
                    out, reps = _normalize_batch(ctx, src, _opts(case))
                finally:
                    os.environ.pop("FLO_NORM_NO_SKIP", None)
                runs.append(([out.download_pcm(i) for i in range(out.n_clips)], [bytes(r) for r in reps][:out.n_clips]))
                out.close()
            for i, (a, b) in enumerate(zip(runs[0][0], runs[1][0])):
                assert _first_difference(a, b) is None, (name, i, _first_difference(a, b))
            assert runs[0][1] == runs[1][1], name
        finally:
            src.close()


def test_results_do_not_depend_on_recycled_memory(ctx):
    """the work lists, the start values of the peak and report words and the halo reads: the same bytes whatever the pool's
    blocks held before (0x7F: a huge positive number and a large count; 0xFF: NaN and the largest unsigned)"""
    import recycled_scenarios as S
    records = []
    try:
        for fill in (None, 0x7F, 0xFF):
            flo_amd.debug_pool_fill(fill)
            records.append(normalize_recycled.normalise(ctx))
    finally:
        flo_amd.debug_pool_fill(None)
    for rec in records[1:]:
        assert S.first_difference(records[0], rec) is None, S.first_difference(records[0], rec)
    assert normalize_recycled.NAME in [s["name"] for s in S.SCENARIOS]


def test_python_faces_and_an_empty_batch(ctx):
    rng = np.random.default_rng(5)
    clips = [rng.uniform(-0.9, 0.9, 3000 * 2).astype(np.float32), rng.uniform(-0.1, 0.1, 1001).astype(np.float32)]   # (an odd count: a partial frame)
    outs, reports = flo_amd.normalize_many(clips, 48000, 2, ctx=ctx, target_lufs=-3.0, limit=True)
    assert [o.size for o in outs] == [6000, 1000] and len(reports) == 2
    one, rep = ctx.normalize(clips[0], 48000, 2, target_lufs=-3.0, limit=True)
    assert _first_difference(one, outs[0]) is None and rep == reports[0]
    assert abs(rep["input_lufs"] + rep["gain_db"] + 3.0) < 1e-5 and rep["status"] == "" and rep["limited_frames"] > 0
    assert np.abs(one).max() <= float(M.ceiling(-1.0)) * (1 + 2.0 ** -22)
    # another look-ahead, in milliseconds
    two, rep2 = ctx.normalize(clips[0], 48000, 2, target_lufs=-3.0, limit=True, lookahead_ms=0.25)
    want, wrep, _ = M.normalize(clips[0], 2, 48000, rep["input_lufs"], -1.0, -3.0, -1.0, M.LIMIT, 12)
    assert _first_difference(two, want) is None and rep2["limited_frames"] == wrep["limited_frames"]
    with pytest.raises(flo_amd.FloError, match="lookahead_frames"):
        ctx.normalize(clips[0], 48000, 2, limit=True, lookahead_ms=50.0)
    with pytest.raises(flo_amd.FloError, match="ceiling_dbtp"):
        ctx.normalize(clips[0], 48000, 2, ceiling_dbtp=float("nan"))
    empty = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [], 44100, 2, 0.55)
    try:
        out, reports = empty.normalize()
        assert out.n_clips == 0 and reports == [] and empty.true_peaks().size == 0
        out.close()
    finally:
        empty.close()
    fresh = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [100], 44100, 2, 0.55)
    try:
        with pytest.raises(flo_amd.FloError, match="no PCM"):
            fresh.normalize()
    finally:
        fresh.close()


def test_encode_of_the_normalised_batch(ctx):
    """upload -> normalise -> encode never leaves the device: the files equal encode_lossy of the model's output"""
    rng = np.random.default_rng(9)
    sr, ch = 44100, 2
    clips = [(rng.uniform(-0.4, 0.4, n * ch) * np.repeat(np.sin(np.arange(n) / 900.0) ** 2, ch)).astype(np.float32) for n in (30000, 5000)]
    clips[0][20000:20040] = 0.99
    src = _batch_of(ctx, clips, sr, ch, flo_amd.MODE_LOSSY, 0.55)
    try:
        measured = src.analyze_all()
        out, reports = src.normalize(target_lufs=-6.0, limit=True)
        try:
            assert sum(r["limited_frames"] for r in reports) > 0
            out.encode()
            out.sync()
            for i, x in enumerate(clips):
                want, _, _ = M.normalize(x, ch, sr, measured[i]["integrated_lufs"], measured[i]["sample_peak_dbfs"], -6.0, -1.0, M.LIMIT)
                assert out.fetch(i) == ctx.encode_lossy(want, sr, ch, 0.55), i
        finally:
            out.close()
    finally:
        src.close()


def test_cli_normalize_and_encode_lufs(ctx, tmp_path, capsys):
    from flo_amd import cli
    from flo_amd.wav import read_wav_bytes, write_wav_bytes
    rng = np.random.default_rng(3)
    x = rng.uniform(-0.2, 0.2, 2 * 24000).astype(np.float32)
    wav, outp, flo = tmp_path / "in.wav", tmp_path / "out.wav", tmp_path / "out.flo"
    wav.write_bytes(write_wav_bytes(x, 48000, 2))
    src = read_wav_bytes(wav.read_bytes())[0]
    assert cli.main(["normalize", str(wav), str(outp), "--lufs", "-16", "--ceiling", "-2", "--limit"]) == 0
    got, sr, ch = read_wav_bytes(outp.read_bytes())
    want, rep = ctx.normalize(src, 48000, 2, target_lufs=-16.0, ceiling_dbtp=-2.0, limit=True)
    assert (sr, ch) == (48000, 2) and _first_difference(np.ascontiguousarray(got, np.float32), want) is None
    assert "Gain:" in capsys.readouterr().out
    # encode --lufs: the file holds the normalised audio (lossless at 16 bits: quantised), and META describes it
    assert cli.main(["encode", str(wav), str(flo), "--lufs", "-16"]) == 0
    data = flo.read_bytes()
    assert cli.flo_info(data)["crc_valid"]
    level, _ = ctx.normalize(src, 48000, 2, target_lufs=-16.0)
    pcm = flo_amd.decode(data)
    assert pcm.size >= level.size and float(np.abs(pcm[:level.size] - level).max()) <= 1.0 / 32767 + 1e-6
