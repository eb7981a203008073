"""Trimming, fades, padding and channel remixing on the device (flo_batch_edit, flo_batch_active_range, flo_edit and their
Python faces) against tests/edit_model.py, bit for bit: uint32 views are compared, samples that are NaN on both sides match
by position. Every output clip is checked in its batch and alone through flo_edit. No clip is longer than 3F + 5 frames,
F = flo_edit_tile_frames; the one long cut (fades of 2^24 - 1) is cut from a short source."""
import ctypes as C
import math

import numpy as np
import pytest

import edit_model as M
import edit_recycled
import flo_amd
from flo_amd import _native
from gpu_util import ctx  # noqa: F401

gpu = pytest.mark.gpu   # every test but the registry's own: that one runs wherever this module's tests are selected


@pytest.fixture(scope="module", autouse=True)
def scenario_in_place():
    """the edit scenario moves in front of the last one when this module's tests begin (tests/edit_recycled.py says why)"""
    edit_recycled.take_place()
    yield


def test_the_scenario_stands_in_front_of_the_last_one():
    import recycled_scenarios as S
    names = [s["name"] for s in S.SCENARIOS]
    assert names.count(edit_recycled.NAME) == 1 and names[-2] == edit_recycled.NAME and names[-1].startswith("rate-targeted")
    assert S.EXEMPT["flo_edit_tile_frames"] == "host arithmetic"
    covers = next(s["covers"] for s in S.SCENARIOS if s["name"] == edit_recycled.NAME)
    assert covers == ["flo_batch_edit", "flo_batch_active_range", "flo_edit"]
F32 = np.float32


def _batch_of(ctx, clips, rate, ch, mode=flo_amd.MODE_LOSSLESS, q=0):
    b = flo_amd.Batch(ctx, mode, [x.size for x in clips], rate, ch, q)
    for i, x in enumerate(clips):
        ctx._chk(ctx._L.flo_batch_upload(b._h, i, np.ascontiguousarray(x, F32).ctypes.data))
    b.sync()
    return b


def _c_segs(segs):
    arr = (_native.EditSegment * max(len(segs), 1))()
    for k, g in enumerate(segs):
        arr[k] = _native.EditSegment(g["start"], g["frames"], g["clip"], g["pad_head"], g["pad_tail"], g["fade_in"], g["fade_out"], g.get("reserved", 0))
    return arr


def _c_matrix(matrix):
    return None if matrix is None else np.ascontiguousarray(matrix, F32).reshape(-1)


def _edit_batch(ctx, b, segs, cout, matrix):
    """flo_batch_edit through the C ABI: the new Batch"""
    h, m = C.c_void_p(), _c_matrix(matrix)
    ctx._chk(ctx._L.flo_batch_edit(b._h, len(segs), _c_segs(segs), cout, m.ctypes.data if m is not None else None, C.byref(h)))
    return flo_amd.Batch(ctx, b._made[0], [M.out_frames(g) * cout for g in segs], b.sample_rate, cout, b._made[1], _handle=h)


def _edit_alone(ctx, x, rate, cin, g, cout, matrix):
    out, n, m = C.c_void_p(), C.c_size_t(), _c_matrix(matrix)
    ctx._chk(ctx._L.flo_edit(ctx._h, x.ctypes.data, x.size, rate, cin, _c_segs([dict(g, clip=0)]), cout, m.ctypes.data if m is not None else None,
                             C.byref(out), C.byref(n)))
    res = np.frombuffer(C.string_at(out.value, n.value * 4), F32).copy() if n.value else np.zeros(0, F32)
    ctx._L.flo_free(out)
    return res


def _download_all(b):
    return [b.download_pcm(i) for i in range(b.n_clips)]


@pytest.fixture(scope="module")
def wanted():
    """the model's output of every form's cuts, computed once"""
    memo = {}

    def get(name):
        if name not in memo:
            cin, cout, matrix, clips, segs = M.form_case(name)
            memo[name] = [M.edit(clips[g["clip"]], cin, g, cout, matrix) for g in segs]
        return memo[name]
    return get


@gpu
@pytest.mark.parametrize("name", [f[0] for f in M.FORMS])
def test_batch_and_alone_equal_the_model(ctx, wanted, name):
    cin, cout, matrix, clips, segs = M.form_case(name)
    want = wanted(name)
    src = _batch_of(ctx, clips, 48000, cin)
    try:
        out = _edit_batch(ctx, src, segs, cout, matrix)
        try:
            got = _download_all(out)
        finally:
            out.close()
        for k, g in enumerate(segs):
            assert M.same(got[k], want[k]) is None, (name, "batch", k, g, M.same(got[k], want[k]))
        for k, g in enumerate(segs):
            alone = _edit_alone(ctx, clips[g["clip"]], 48000, cin, g, cout, matrix)
            assert M.same(alone, want[k]) is None, (name, "alone", k, g, M.same(alone, want[k]))
        for i, x in enumerate(clips):   # the source is unchanged
            assert np.array_equal(src.download_pcm(i).view(np.uint32), x.view(np.uint32)), (name, i)
    finally:
        src.close()


@gpu
@pytest.mark.parametrize("name", ["2to2_copy", "3to3_copy", "2to1", "1to2", "3to2"])
def test_fades(ctx, name):
    _, cin, cout, matrix = next(f for f in M.FORMS if f[0] == name)
    F = M.tile_frames(cin, cout)
    clips, segs = M.fade_case(F, cin)
    plain = [dict(g, fade_in=0, fade_out=0) for g in segs]
    src = _batch_of(ctx, clips, 44100, cin)
    try:
        out, ref = _edit_batch(ctx, src, segs, cout, matrix), _edit_batch(ctx, src, plain, cout, matrix)
        try:
            got, unfaded = _download_all(out), _download_all(ref)
        finally:
            out.close()
            ref.close()
        crossing = 0
        for k, g in enumerate(segs):
            x = clips[g["clip"]]
            want = M.edit(x, cin, g, cout, matrix)
            assert M.same(got[k], want) is None, (name, k, g, M.same(got[k], want))
            alone = _edit_alone(ctx, x, 44100, cin, g, cout, matrix)
            assert M.same(alone, want) is None, (name, "alone", k, g, M.same(alone, want))
            # outside any fade the samples are the unfaded result's, bit for bit; past the source's end they stay +0.0
            n = M.avail(g, x.size // cin)
            _, on = M.weights(g, g["frames"])
            keep = np.ones(M.out_frames(g), bool)
            keep[g["pad_head"]:g["pad_head"] + g["frames"]] = ~on
            a, b = got[k].reshape(-1, cout)[keep], unfaded[k].reshape(-1, cout)[keep]
            assert M.same(a, b) is None, (name, "outside the fades", k, g)
            past = got[k].reshape(-1, cout)[g["pad_head"] + n:]
            assert not past.view(np.uint32).any(), (name, "past the source", k, g)
            classes = M.tile_classes(g, x.size // cin, F)
            crossing += sum(1 for c0, c1 in zip(classes, classes[1:]) if c0 & M.FADED and c1 & M.FADED)
        assert crossing >= 3, "no fade of the case crosses a tile boundary"
    finally:
        src.close()


@gpu
def test_the_longest_fade(ctx):
    """fade_in = fade_out = 2^24 - 1 on a cut that long, cut from a short source: the weights of the largest u and v"""
    F = M.tile_frames(1, 1)
    x = M.noise(3 * F + 5, 1, 11, F)
    frames = M.MAX_FADE - 1
    segs = [M.seg(0, 0, frames, fade_in=frames, fade_out=frames), M.seg(0, 0, frames, fade_in=0, fade_out=frames)]
    src = _batch_of(ctx, [x], 48000, 1)
    try:
        out = _edit_batch(ctx, src, segs, 1, None)
        try:
            for k, g in enumerate(segs):
                got = out.download_pcm(k)
                want = M.edit(x, 1, g, 1, None)
                assert M.same(got, want) is None, (k, M.same(got, want))
        finally:
            out.close()
        for bad in (M.seg(0, 0, frames + 1, fade_in=frames + 1), M.seg(0, 0, frames + 1, fade_out=frames + 1)):
            with pytest.raises(flo_amd.FloError, match="fade_"):
                _edit_batch(ctx, src, [bad], 1, None)
    finally:
        src.close()


def _active_clips(ch, F):
    t = M.threshold(-60.0)
    n = 2 * F + 5
    clips = [np.zeros(n * ch, F32)]
    for c in range(ch):
        for f in (0, F - 1, F, n - 1):
            x = np.zeros(n * ch, F32)
            x[f * ch + c] = F32(0.5)
            clips.append(x)
    at, above = np.zeros(n * ch, F32), np.zeros(n * ch, F32)
    at[(F + 3) * ch] = t
    at[7 * ch + ch - 1] = -t
    above[(F + 3) * ch + ch - 1] = np.nextafter(t, F32(1))
    above[5 * ch] = -np.nextafter(t, F32(1))
    nan = np.zeros(n * ch, F32)
    nan[(F - 2) * ch] = F32(np.nan)
    rng = np.random.default_rng(3)
    noise = (rng.standard_normal(n * ch) * 0.1).astype(F32)
    noise[:40 * ch] = 0
    noise[-(F + 9) * ch:] = 0
    clips += [at, above, nan, np.full(n * ch, -0.0, F32), np.zeros(0, F32), np.full(3 * ch, 1e-3, F32), noise, np.full(ch, F32(np.inf))]
    return clips


@gpu
@pytest.mark.parametrize("ch", [1, 2, 3])
def test_active_ranges(ctx, ch):
    F = M.tile_frames(ch, ch)
    clips = _active_clips(ch, F)
    b = _batch_of(ctx, clips, 48000, ch)
    try:
        for db, thr in ((-60.0, M.threshold(-60.0)), (None, F32(0.0)), (None, F32(np.inf)), (None, F32(0.25))):
            first, end = np.zeros(len(clips), np.uint64), np.zeros(len(clips), np.uint64)
            ctx._chk(ctx._L.flo_batch_active_range(b._h, float(thr), first.ctypes.data, end.ctypes.data))
            want = [M.active_range(x, ch, thr) for x in clips]
            assert list(zip(first.tolist(), end.tolist())) == want, (ch, thr)
            if db is not None:
                assert b.active_ranges(db).tolist() == [list(w) for w in want]
        assert any(w != (0, 0) for w in [M.active_range(x, ch, np.inf) for x in clips])   # the NaN clip is active under +inf
        for i, x in enumerate(clips):   # one clip at a time
            r = flo_amd.active_range_many([x], 48000, ch, -60.0, ctx=ctx)
            assert tuple(r[0].tolist()) == M.active_range(x, ch, M.threshold(-60.0)), (ch, i)
        for bad in (-1.0, float("nan")):
            first = np.zeros(len(clips), np.uint64)
            assert ctx._L.flo_batch_active_range(b._h, bad, first.ctypes.data, first.ctypes.data) == 1
            assert "threshold" in ctx._L.flo_last_error(ctx._h).decode()
    finally:
        b.close()


@gpu
def test_trim_silence(ctx):
    rate, ch = 48000, 2
    F = M.tile_frames(ch, ch)
    rng = np.random.default_rng(21)
    clips = []
    for head, body, tail in ((300, 2 * F, 500), (0, F + 7, 1), (5, 3, 0), (F, 0, 5), (0, 0, 0), (F - 1, F + 2, F + 1)):
        t = np.arange(body)
        tone = (0.4 * np.sin(t * 0.05))[:, None] * np.array([1.0, -0.5])
        tone += rng.standard_normal((body, ch)) * 0.01 + 0.02
        x = np.concatenate([np.zeros((head, ch)), tone, np.zeros((tail, ch))]).astype(F32).reshape(-1)
        clips.append(x)
    b = _batch_of(ctx, clips, rate, ch)
    try:
        for kw in (dict(), dict(pre_ms=1.0, post_ms=2.5, fade_ms=4.0), dict(threshold_db=-30.0, pre_ms=100.0, post_ms=100.0, fade_ms=1e4)):
            out, ranges = b.trim_silence(**kw)
            try:
                thr = M.threshold(kw.get("threshold_db", -60.0))
                for i, x in enumerate(clips):
                    first, end = M.active_range(x, ch, thr)
                    assert tuple(ranges[i].tolist()) == (first, end), (kw, i)
                    g = M.trim_segment(0, first, end, x.size // ch, rate, kw.get("pre_ms", 0.0), kw.get("post_ms", 0.0), kw.get("fade_ms", 0.0))
                    want = M.edit(x, ch, g, ch, None)
                    got = out.download_pcm(i)
                    assert M.same(got, want) is None, (kw, i, g, M.same(got, want))
                assert out.n_interleaved[4] == 0 and out.n_interleaved[0] > 0
            finally:
                out.close()
        outs, ranges2 = flo_amd.trim_silence_many(clips, rate, ch, ctx=ctx, pre_ms=1.0, post_ms=2.5, fade_ms=4.0)
        g = M.trim_segment(0, *M.active_range(clips[0], ch, M.threshold(-60.0)), clips[0].size // ch, rate, 1.0, 2.5, 4.0)
        assert M.same(outs[0], M.edit(clips[0], ch, g, ch, None)) is None and ranges2.shape == (len(clips), 2)
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


@gpu
@pytest.mark.parametrize("kind", ["lossy to_mono", "lossless crop"])
def test_the_result_is_a_first_class_batch(ctx, kind):
    """the edited batch against a batch of the model's output uploaded the usual way: the same files (so the padding behind
    the clips, pcm_written and the plan are right), the same analysis, the same resampled and normalised audio"""
    rng = np.random.default_rng(33)
    sr = 44100
    lens = (9000, 1, 0, 2500, 1024)
    clips = [(rng.uniform(-0.5, 0.5, n * 2) * np.repeat(np.sin(np.arange(n) / 300.0) ** 2 + 0.05, 2)).astype(F32) for n in lens]
    if kind == "lossy to_mono":
        mode, q, cout = flo_amd.MODE_LOSSY, 0.55, 1
        matrix = np.array([[1.0 / 2] * 2], F32)
        segs = [M.seg(i, 0, n) for i, n in enumerate(lens)]
    else:
        mode, q, cout, matrix = flo_amd.MODE_LOSSLESS, 5, 2, None
        segs = [M.seg(0, 1001, 5000, fade_in=64, fade_out=64), M.seg(3, 3, 2000, 5, 7), M.seg(1, 0, 1), M.seg(4, 1000, 100), M.seg(0, 3, 2048)]
    src = _batch_of(ctx, clips, sr, 2, mode, q)
    try:
        out = src.to_mono() if kind == "lossy to_mono" else src.edit(segs)
        want = [M.edit(clips[g["clip"]], 2, g, cout, matrix) for g in segs]
        up = _batch_of(ctx, want, sr, cout, mode, q)
        try:
            assert out.n_interleaved == up.n_interleaved and out.channels == cout
            for a, b in zip(out.analyze_all(), up.analyze_all()):
                _same_analysis(a, b)
            for which in ("resample", "normalize"):
                ra = out.resample(48000) if which == "resample" else out.normalize(target_lufs=-20.0)[0]
                rb = up.resample(48000) if which == "resample" else up.normalize(target_lufs=-20.0)[0]
                try:
                    for i in range(ra.n_clips):
                        assert M.same(ra.download_pcm(i), rb.download_pcm(i)) is None, (kind, which, i)
                finally:
                    ra.close()
                    rb.close()
            out.encode()
            up.encode()
            out.sync()
            up.sync()
            for i in range(out.n_clips):
                assert out.fetch(i) == up.fetch(i), (kind, i)
        finally:
            out.close()
            up.close()
    finally:
        src.close()


@gpu
def test_a_chain_of_derived_batches_keeps_its_work_and_its_bit_depth(ctx):
    """resample -> normalise -> to_mono, each source closed as soon as its successor exists and the test itself waiting for
    nothing before the encode: each batch lives on the work block its own launch was queued with, the bit depth of 24 passes
    through all three, and the empty and the one-frame clip stand in every prefix. Every file equals the file of the same
    clip taken alone through the one-clip calls"""
    rng = np.random.default_rng(41)
    lens = (0, 1, 4097)
    clips = [(rng.uniform(-0.4, 0.4, n * 2) * np.repeat(np.sin(np.arange(n) / 200.0) ** 2 + 0.05, 2)).astype(F32) for n in lens]
    mono = np.array([[1.0 / 2] * 2], F32)
    want = []
    for x in clips:
        y = flo_amd.resample(x, 48000, 44100, 2)
        z = flo_amd.remix(flo_amd.normalize(y, 44100, 2)[0], 44100, 2, mono)
        want.append(flo_amd.default_context().encode_lossless(z, 44100, 1, bit_depth=24))
    b = _batch_of(ctx, clips, 48000, 2, flo_amd.MODE_LOSSLESS, 5)
    try:
        b.set_bit_depth(24)
        for step in (lambda s: s.resample(44100), lambda s: s.normalize()[0], lambda s: s.to_mono()):
            nxt = step(b)
            b.close()
            b = nxt
        b.encode()
        b.sync()
        assert b.channels == 1 and b.sample_rate == 44100
        for i in range(len(lens)):
            assert b.fetch(i) == want[i], i
    finally:
        b.close()


@gpu
def test_errors_leave_no_batch_and_a_usable_context(ctx):
    clips = [np.arange(20, dtype=F32), np.arange(8, dtype=F32)]
    nan_m, big = np.array([[0.5, np.nan]], F32), np.full((9, 9), 0.1, F32)
    most = (2 ** 64 - 1) // 8 // 2
    src = _batch_of(ctx, clips, 48000, 2)
    try:
        cases = [([M.seg(2, 0, 1)], 2, None, "clip"), ([M.seg(0, 0, 1, reserved=1)], 2, None, "reserved"),
                 ([M.seg(0, 0, 4, fade_in=5)], 2, None, "fade_in"), ([M.seg(0, 0, 4, fade_out=5)], 2, None, "fade_out"),
                 ([M.seg(0, 0, 1 << 24, fade_in=1 << 24)], 2, None, "fade_in"), ([M.seg(0, 0, 4)], 1, None, "matrix"),
                 ([M.seg(0, 0, 4)], 1, nan_m, "matrix"), ([M.seg(0, 0, 4)], 9, big[:, :2], "out_channels"),
                 ([M.seg(0, 0, most + 1)], 2, None, "frames"), ([M.seg(0, 0, most, pad_tail=1)], 2, None, "frames")]
        for segs, cout, matrix, word in cases:
            h, m = C.c_void_p(0xDEAD), _c_matrix(matrix)
            rc = ctx._L.flo_batch_edit(src._h, len(segs), _c_segs(segs), cout, m.ctypes.data if m is not None else None, C.byref(h))
            msg = ctx._L.flo_last_error(ctx._h).decode()
            assert rc == 1 and word in msg and msg.startswith("flo_batch_edit: "), (word, rc, msg)
            assert not h.value, word
            assert M.refusal([10, 4], 2, False, segs, cout, matrix) == word
            out, n = C.c_void_p(0xDEAD), C.c_size_t(7)
            rc = ctx._L.flo_edit(ctx._h, clips[0].ctypes.data, clips[0].size, 48000, 2, _c_segs(segs), cout, m.ctypes.data if m is not None else None,
                                 C.byref(out), C.byref(n))
            if word != "clip":   # (flo_edit has one clip; the test's segments name it)
                assert rc == 1 and word in ctx._L.flo_last_error(ctx._h).decode() and not out.value and n.value == 0, word
            else:
                assert rc == 1 and not out.value
        # in_channels above 8 with a matrix; out_channels above 8 for a lossy batch
        nine = _batch_of(ctx, [np.zeros(18, F32)], 48000, 9)
        try:
            h, m = C.c_void_p(), _c_matrix(big[:2])
            assert ctx._L.flo_batch_edit(nine._h, 1, _c_segs([M.seg(0, 0, 2)]), 2, m.ctypes.data, C.byref(h)) == 1
            assert "in_channels" in ctx._L.flo_last_error(ctx._h).decode() and not h.value
            ok = _edit_batch(ctx, nine, [M.seg(0, 0, 2, 1, 1)], 9, None)   # a lossless copy of nine channels is fine
            assert ok.download_pcm(0).size == 36
            ok.close()
        finally:
            nine.close()
        lossy8 = _batch_of(ctx, [np.zeros(16, F32)], 48000, 8, flo_amd.MODE_LOSSY, 0.5)
        try:
            h = C.c_void_p()
            assert ctx._L.flo_batch_edit(lossy8._h, 1, _c_segs([M.seg(0, 0, 2)]), 9, None, C.byref(h)) == 1
            assert "out_channels" in ctx._L.flo_last_error(ctx._h).decode() and not h.value
        finally:
            lossy8.close()
        # the context still works, and so does the source batch
        out = _edit_batch(ctx, src, [M.seg(1, 1, 2, 1, 1)], 2, None)
        assert out.download_pcm(0).tolist() == [0, 0, 2, 3, 4, 5, 0, 0]
        out.close()
    finally:
        src.close()


@gpu
def test_python_faces_empty_batches_and_states(ctx):
    rng = np.random.default_rng(5)
    x = rng.uniform(-0.9, 0.9, 3000 * 2).astype(F32)
    odd = rng.uniform(-0.1, 0.1, 1001).astype(F32)   # an odd count: the partial frame is not part of the clip
    g = M.seg(0, 100, 500, 3, 4, 50, 60)
    one = ctx.edit(x, 48000, 2, dict(start=100, frames=500, pad_head=3, pad_tail=4, fade_in=50, fade_out=60))
    assert M.same(one, M.edit(x, 2, g, 2, None)) is None
    assert M.same(ctx.edit(x, 48000, 2), x) is None
    swap = [[0, 1], [1, 0]]
    outs = flo_amd.edit_many([x, odd], 48000, 2, [dict(clip=1), dict(clip=0, start=2990)], matrix=swap, ctx=ctx)
    assert M.same(outs[0], M.edit(odd, 2, M.seg(0, 0, 500), 2, swap)) is None and outs[1].size == 20
    both = flo_amd.remix_many([x, odd], 48000, 2, [[0.5, 0.5]], ctx=ctx)
    assert M.same(both[1], M.edit(odd, 2, M.seg(0, 0, 500), 1, [[0.5, 0.5]])) is None
    b = _batch_of(ctx, [x, odd], 48000, 2)
    try:
        mono = b.to_mono()
        assert mono.channels == 1 and mono.n_interleaved == [3000, 500]
        assert M.same(mono.download_pcm(0), M.edit(x, 2, M.seg(0, 0, 3000), 1, np.array([[0.5, 0.5]], F32))) is None
        mono.close()
        none = b.edit([])
        assert none.n_clips == 0 and none.active_ranges().shape == (0, 2)
        none.close()
    finally:
        b.close()
    empty = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [], 44100, 2, 0.55)
    try:
        out = empty.edit([])
        assert out.n_clips == 0 and empty.active_ranges().shape == (0, 2)
        out.close()
        out, ranges = empty.trim_silence()
        assert out.n_clips == 0 and ranges.shape == (0, 2)
        out.close()
    finally:
        empty.close()
    fresh = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [100], 44100, 2, 0.55)
    try:
        with pytest.raises(flo_amd.FloError, match="no PCM"):
            fresh.edit([dict(clip=0)])
        with pytest.raises(flo_amd.FloError, match="no PCM"):
            fresh.active_ranges()
    finally:
        fresh.close()


@gpu
def test_cli_edit_and_encode(ctx, tmp_path, capsys):
    from flo_amd import cli
    from flo_amd.wav import read_wav_bytes, write_wav_bytes
    rng = np.random.default_rng(3)
    sr = 48000
    body = rng.uniform(-0.2, 0.2, 2 * 24000).astype(F32)
    x = np.concatenate([np.zeros(2 * 4800, F32), body, np.zeros(2 * 2400, F32)])
    wav, outp, flo = tmp_path / "in.wav", tmp_path / "out.wav", tmp_path / "out.flo"
    wav.write_bytes(write_wav_bytes(x, sr, 2))
    src = np.ascontiguousarray(read_wav_bytes(wav.read_bytes())[0], F32)
    assert cli.main(["edit", str(wav), str(outp), "--mono", "--trim-silence", "-60", "--pre-ms", "10", "--fade-in", "5", "--fade-out", "20",
                     "--pad-tail", "0.25"]) == 0
    got, rate, ch = read_wav_bytes(outp.read_bytes())
    first, end = M.active_range(src, 2, M.threshold(-60.0))
    g = M.seg(0, first - 480, end - first + 480, 0, 12000, 240, 960)
    want = M.edit(src, 2, g, 1, np.array([[0.5, 0.5]], F32))
    assert (rate, ch) == (sr, 1) and M.same(np.ascontiguousarray(got, F32), want) is None
    assert "Active range" in capsys.readouterr().out
    assert cli.main(["edit", str(wav), str(outp), "--start", "0.1", "--duration", "0.5", "--channels", "2", "--matrix", "0,1,1,0"]) == 0
    got, rate, ch = read_wav_bytes(outp.read_bytes())
    assert ch == 2 and M.same(np.ascontiguousarray(got, F32), M.edit(src, 2, M.seg(0, 4800, 24000), 2, [[0, 1], [1, 0]])) is None
    # encode --mono --trim-silence: the file holds the edited audio (lossless at 16 bits: quantised)
    assert cli.main(["encode", str(wav), str(flo), "--mono", "--trim-silence", "-60"]) == 0
    data = flo.read_bytes()
    info = cli.flo_info(data)
    assert info["crc_valid"] and info["channels"] == 1 and info["total_samples"] == end - first
    level = M.edit(src, 2, M.seg(0, first, end - first), 1, np.array([[0.5, 0.5]], F32))
    pcm = flo_amd.decode(data)
    assert pcm.size >= level.size and float(np.abs(pcm[:level.size] - level).max()) <= 1.0 / 32767 + 1e-6
