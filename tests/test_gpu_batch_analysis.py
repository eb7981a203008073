"""The analysis metadata of every clip of a batch in one device pass (flo_batch_analyze_all / Batch.analyze_all,
flo_batch_analysis_metadata_all, flo_amd.encode*_many): field for field, peak for peak and byte for byte what the per-clip
path gives, in groups or not, and for odd-length lossy clips what the reference gives."""
import ctypes as C

import numpy as np
import pytest

import flo_amd
import signals
from flo_amd import meta
from gpu_util import ctx  # noqa: F401
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FIELDS = ("hash", "duration_ms", "sample_rate", "channels", "frequency_peaks", "energy_profile", "avg_loudness",
          "integrated_lufs", "length_ms", "loudness_range_lu", "true_peak_dbtp", "sample_peak_dbfs", "sum_squares")


def _bits(v):
    if isinstance(v, (float, np.floating)):
        return np.array(v, np.float64 if isinstance(v, float) else type(v)).tobytes()
    return v


def _same(a, b):
    assert a["peaks"].size == b["peaks"].size
    assert np.array_equal(a["peaks"].view(np.uint32), b["peaks"].view(np.uint32))
    for k in FIELDS:
        assert _bits(a[k]) == _bits(b[k]), (k, a[k], b[k])


def _clips(sr, ch):
    rng = np.random.default_rng(sr + ch)
    frames = [1, 200, 65536, 65537, int(12.3 * sr), 40 * sr]
    frames += [f // ch for f in (253, 254, 255, 509, 510, 511, 1021, 1022)]   # 9 + 4 n around the hash's 1 KiB chunks
    out = [signals.music_like(sr, f, ch, seed=i) for i, f in enumerate(frames)]
    out.append(np.zeros(3000 * ch, np.float32))                                         # silence
    out.append(np.array([0.1, np.nan, -np.inf, 0.2] * (700 * ch), np.float32))         # NaN and inf
    out.append(rng.uniform(-4, 4, 30000 * ch).astype(np.float32))                       # loud noise
    out.append(np.zeros(0, np.float32))                                                  # empty
    return out


def _batch(ctx, clips, sr, ch, mode=flo_amd.MODE_LOSSLESS, q=5):
    b = flo_amd.Batch(ctx, mode, [c.size for c in clips], sr, ch, q)
    for i, c in enumerate(clips):
        b.upload(i, c)
    return b


@pytest.mark.parametrize("sr,ch", [(44100, 2), (16000, 1), (96000, 6), (8000, 2)])
def test_every_clip_equals_the_per_clip_path(ctx, sr, ch):
    clips = _clips(sr, ch)
    b = _batch(ctx, clips, sr, ch)
    try:
        got = b.analyze_all(50)
        metas = b.analysis_metadata_all(50)
        assert len(got) == len(metas) == len(clips)
        for i, c in enumerate(clips):
            _same(got[i], ctx.analyze(c, sr, ch, 50))
            m = O.analysis_metadata(c, sr, ch, 50)
            assert metas[i] == b.analysis_metadata(i, 50) == m, i
    finally:
        b.close()


def test_other_peak_rates(ctx):
    sr, ch = 44100, 2
    clips = [signals.music_like(sr, f, ch, seed=f) for f in (1, 200, 50000, 65537, 100000)]
    b = _batch(ctx, clips, sr, ch)
    try:
        for pps in (1, 10, 200, 44100):
            got, metas = b.analyze_all(pps), b.analysis_metadata_all(pps)
            for i, c in enumerate(clips):
                _same(got[i], ctx.analyze(c, sr, ch, pps))
                assert metas[i] == O.analysis_metadata(c, sr, ch, pps), (pps, i)
    finally:
        b.close()


def test_groups_give_the_same_results(ctx, monkeypatch):
    sr, ch = 44100, 2
    clips = _clips(sr, ch)
    b = _batch(ctx, clips, sr, ch)
    try:
        one = b.analyze_all(50)
        ctx.profile_enable(True)
        ctx.profile_reset()
        monkeypatch.setenv("FLO_BATCH_ANALYSIS_GROUP_BYTES", str(400_000))   # read per call
        many = b.analyze_all(50)
        metas = b.analysis_metadata_all(50)
        _, n_groups = ctx.profile_query("analysis_batch")
        assert n_groups >= 2 * 3    # two calls, three groups at least each
        for i, c in enumerate(clips):
            _same(many[i], one[i])
            assert metas[i] == O.analysis_metadata(c, sr, ch, 50)
    finally:
        ctx.profile_enable(False)
        b.close()


def test_odd_length_lossy_clips_are_analysed_over_all_samples(ctx):
    sr = 44100
    for ch in (2, 3):
        clips = [signals.music_like(sr, f, ch, seed=f).ravel()[: f * ch - k] for f, k in ((5000, 1), (70001, ch - 1), (20000, 0))]
        clips = [np.ascontiguousarray(c) + np.float32(0.01) for c in clips]   # (no zero in the tails)
        b = _batch(ctx, clips, sr, ch, flo_amd.MODE_LOSSY, 0.55)
        try:
            metas = b.analysis_metadata_all(50)
            got = b.analyze_all(50)
            for i, c in enumerate(clips):   # reading a clip back does not drop its kept tail
                assert np.array_equal(b.download_pcm(i)[: c.size // ch * ch], c[: c.size // ch * ch])
            assert b.analysis_metadata_all(50) == metas
            differs = 0
            for i, c in enumerate(clips):
                want = O.analysis_metadata(c, sr, ch, 50)
                assert metas[i] == want, (ch, i)
                _same(got[i], ctx.analyze(c, sr, ch, 50))
                differs += b.analysis_metadata(i, 50) != want   # the per-clip path reads zeros where the tail was
            assert differs == 2
        finally:
            b.close()


def test_free_functions_many(ctx):
    sr, ch = 44100, 2
    clips = [signals.music_like(sr, f, ch, seed=f) for f in (3000, 40000, 70000)]
    files = flo_amd.encode_many(clips, sr, ch, 16)
    for c, f in zip(clips, files):
        assert f == O.encode_lossless(c, sr, ch, 16, 5, meta=O.analysis_metadata(c, sr, ch, 50))
    for many, one in ((flo_amd.encode_lossy_many(clips, sr, ch, 16, 2), lambda c: flo_amd.encode_lossy(c, sr, ch, 16, 2)),
                      (flo_amd.encode_with_bitrate_many(clips, sr, ch, 16, 192), lambda c: flo_amd.encode_with_bitrate(c, sr, ch, 16, 192))):
        for c, f in zip(clips, many):
            assert f == one(c)
            m = O.analysis_metadata(c, sr, ch, 50)
            assert f[-len(m):] == m
    # an odd-length lossy clip: the reference's META (the caller's samples), the encoder's audio (whole frames)
    odd = np.ascontiguousarray(clips[1][:-1])
    f = flo_amd.encode_lossy_many([odd], sr, ch, 16, 2)[0]
    m = O.analysis_metadata(odd, sr, ch, 50)
    assert f[-len(m):] == m
    g = flo_amd.encode_lossy(odd, sr, ch, 16, 2)
    mg = int.from_bytes(g[62:70], "little")
    assert f[:62] + f[70:-len(m)] == g[:62] + g[70:len(g) - mg]
    user = meta.pack_fields(dict(title="Song", album="LP"))
    order = ["title", "album", "length_ms", "waveform_data", "spectrum_fingerprint", "loudness_profile"]
    for md in (user, [user] * len(clips)):
        for c, f in zip(clips, flo_amd.encode_with_bitrate_many(clips, sr, ch, 16, 192, metadata=md)):
            assert f == flo_amd.encode_with_bitrate(c, sr, ch, 16, 192, metadata=user)
            assert list(meta.unpack(f[len(f) - int.from_bytes(f[62:70], "little"):])) == order
    assert flo_amd.encode_many([], sr, ch, 16) == []


def test_scale_one_launch_group_per_clip_group(ctx):
    sr, ch, n = 44100, 2, 1250
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [10 * sr * ch] * n, sr, ch, 0.55)
    try:
        b.fill_synthetic(seed=7)
        ctx.profile_enable(True)
        ctx.profile_reset()
        got = b.analyze_all(50)
        _, launches = ctx.profile_query("analysis_batch")
        assert launches == 1     # 1250 x ~460 KB of scratch: one group under the default cap
        ctx.profile_enable(False)
        metas = b.analysis_metadata_all(50)
        for i in np.random.default_rng(5).choice(n, 16, replace=False):
            i = int(i)
            assert metas[i] == b.analysis_metadata(i, 50)
            _same(got[i], ctx.analyze(b.download_pcm(i), sr, ch, 50))
    finally:
        ctx.profile_enable(False)
        b.close()


def test_bad_arguments_fail_cleanly(ctx):
    sr, ch = 16000, 1
    clips = [signals.music_like(sr, f, ch, seed=f) for f in (100, 20000)]
    b = _batch(ctx, clips, sr, ch)
    L = b._L
    try:
        off = (C.c_uint64 * 3)()
        an = (flo_amd._native.Analysis * 2)()
        pk = np.zeros(4, np.float32)
        assert L.flo_batch_analyze_all(b._h, 0, an, pk.ctypes.data, pk.size, off) == 1
        assert L.flo_last_error(ctx._h)
        assert L.flo_batch_analyze_all(b._h, 50, an, pk.ctypes.data, pk.size, None) == 1
        assert L.flo_batch_analyze_all(b._h, 50, None, pk.ctypes.data, pk.size, off) == 1
        assert L.flo_batch_analyze_all(b._h, 50, an, pk.ctypes.data, pk.size, off) == 1   # 4 < 5 + 63 peaks
        assert b"too small" in L.flo_last_error(ctx._h)
        out = C.c_void_p()
        assert L.flo_batch_analysis_metadata_all(b._h, 0, C.byref(out), off) == 1
        assert L.flo_batch_analysis_metadata_all(b._h, 50, None, off) == 1
        assert L.flo_batch_analysis_metadata_all(b._h, 50, C.byref(out), None) == 1
        with pytest.raises(flo_amd.FloError):
            b.analyze_all(0)
        # nothing was left broken
        for i, a in enumerate(b.analyze_all(50)):
            _same(a, ctx.analyze(clips[i], sr, ch, 50))
    finally:
        b.close()
