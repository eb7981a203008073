"""Mixing and concatenation on the device (flo_batch_mix, flo_mix and their Python faces) against tests/mix_model.py, bit for
bit: uint32 views are compared, samples that are NaN on both sides match by position. Every output clip is checked in its
batch and alone through flo_mix. No clip is longer than 3F + 5 frames, F = flo_edit_tile_frames(C, C); the one long part
(fades of 2^24 - 1) is cut from a short source. The module also runs the A of tests/mix_recycled.py under every pool fill
(the A, B, A sequence itself runs in tests/test_gpu_recycled_memory.py and tests/test_gpu_late_streams.py, which find it
registered because pytest imports this module first)."""
import ctypes as C
import math

import numpy as np
import pytest

import mix_model as M
import mix_recycled
import flo_amd
import recycled_scenarios as S
from flo_amd import _native
from gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu
F32 = np.float32


def _batch_of(ctx, clips, rate, ch, mode=flo_amd.MODE_LOSSLESS, q=0):
    b = flo_amd.Batch(ctx, mode, [x.size for x in clips], rate, ch, q)
    for i, x in enumerate(clips):
        ctx._chk(ctx._L.flo_batch_upload(b._h, i, np.ascontiguousarray(x, F32).ctypes.data))
    b.sync()
    return b


def _c_parts(parts):
    arr = (_native.MixPart * max(len(parts), 1))()
    for k, g in enumerate(parts):
        arr[k] = _native.MixPart(g["start"], g["frames"], g["at"], g["out"], g["batch"], g["clip"], g["fade_in"], g["fade_out"], g["gain"])
    return arr


def _raw_mix(ctx, srcs, parts, T):
    """flo_batch_mix through the C ABI: (rc, handle)"""
    hs = (C.c_void_p * max(len(srcs), 1))(*[b._h.value if b is not None else None for b in srcs])
    frames = (C.c_uint64 * max(len(T), 1))(*T)
    h = C.c_void_p(0xDEAD)
    rc = ctx._L.flo_batch_mix(hs, len(srcs), len(T), frames, len(parts), _c_parts(parts), C.byref(h))
    return rc, h


def _mix_batch(ctx, srcs, parts, T):
    rc, h = _raw_mix(ctx, srcs, parts, T)
    ctx._chk(rc)
    b = srcs[0]
    return flo_amd.Batch(ctx, b._made[0], [t * b.channels for t in T], b.sample_rate, b.channels, b._made[1], _handle=h)


def _raw_alone(ctx, clips, rate, ch, parts, T):
    clips = [np.ascontiguousarray(x, F32) for x in clips]
    ptrs = (C.c_void_p * max(len(clips), 1))(*[x.ctypes.data for x in clips])
    lens = (C.c_size_t * max(len(clips), 1))(*[x.size for x in clips])
    out, n = C.c_void_p(0xDEAD), C.c_size_t(7)
    rc = ctx._L.flo_mix(ctx._h, len(clips), ptrs, lens, rate, ch, len(parts), _c_parts(parts), T, C.byref(out), C.byref(n))
    return rc, out, n


def _mix_alone(ctx, clips, rate, ch, parts, T):
    rc, out, n = _raw_alone(ctx, clips, rate, ch, parts, T)
    ctx._chk(rc)
    res = np.frombuffer(C.string_at(out.value, n.value * 4), F32).copy() if n.value else np.zeros(0, F32)
    ctx._L.flo_free(out)
    return res


def _download_all(b):
    return [b.download_pcm(i) for i in range(b.n_clips)]


@pytest.mark.parametrize("ch", [1, 2, 3, 8])
def test_batch_and_alone_equal_the_model(ctx, ch):
    sources, parts, T = M.device_case(ch)
    want = M.mix(sources, ch, parts, T, strict=True)
    a = _batch_of(ctx, sources[0], 48000, ch)
    b = _batch_of(ctx, sources[1], 48000, ch, flo_amd.MODE_LOSSY, 0.55)
    try:
        out = _mix_batch(ctx, [a, b], parts, T)
        try:
            got = _download_all(out)
            assert out.n_interleaved == [t * ch for t in T]
        finally:
            out.close()
        for k in range(len(T)):
            assert M.same(got[k], want[k]) is None, (ch, "batch", k, [g for g in parts if g["out"] == k][:4], M.same(got[k], want[k]))
        for k in range(len(T)):
            clips, mine = M.alone(sources, [g for g in parts if g["out"] == k])
            alone = _mix_alone(ctx, clips, 48000, ch, mine, T[k])
            assert M.same(alone, want[k]) is None, (ch, "alone", k, mine[:4], M.same(alone, want[k]))
        for src, batch in ((sources[0], a), (sources[1], b)):   # the sources are unchanged
            for i, x in enumerate(src):
                assert np.array_equal(batch.download_pcm(i).view(np.uint32), x.view(np.uint32)), (ch, i)
    finally:
        a.close()
        b.close()


def test_denormals_stay_inside_the_flush_allowance(ctx):
    """One clip of denormals through a two-part mix. Held only to |got - want| <= P * 2^-126, P the parts live on the sample:
    what a device that flushes denormal inputs, coefficients or results to zero may lose per FMA."""
    ch = 2
    F = M.tile_frames(ch)
    x = (M.plain(F + 9, ch, 5) * F32(2.0 ** -130)).astype(F32)
    assert ((np.abs(x) < 2.0 ** -126) & (x != 0)).all()
    parts = [M.part(0, 0, 0, 0, F + 9, 0, 1.0), M.part(0, 0, 0, 3, F, 5, 0.5, 4, 4)]
    T = F + 9
    counts = np.zeros(T, np.int64)
    want = M.mix_clip([[x]], ch, parts, T, counts=counts)
    src = _batch_of(ctx, [x], 48000, ch)
    try:
        out = _mix_batch(ctx, [src], parts, [T])
        try:
            got = out.download_pcm(0)
        finally:
            out.close()
    finally:
        src.close()
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).reshape(T, ch)
    assert counts.max() == 2 and (err <= counts[:, None] * 2.0 ** -126).all(), float(err.max())


@pytest.mark.parametrize("ms", [0.0, 2.0])
def test_concat_equals_the_model(ctx, ms):
    ch, rate = 2, 48000
    F = M.tile_frames(ch)
    clips = [M.plain(n, ch, 40 + i) for i, n in enumerate((F + 7, 50, 0, F - 60, 1, 300))]
    groups = [[0, 1, 2, 3], [], [4], [5, 0], [1, 4, 1], [3, 3]]
    frames = [x.size // ch for x in clips]
    b = _batch_of(ctx, clips, rate, ch)
    try:
        out = b.concat(groups, crossfade_ms=ms)
        try:
            got = _download_all(out)
        finally:
            out.close()
        for k, g in enumerate(groups):
            parts, T = flo_amd.concat_parts(frames, rate, ms, clips=g)
            want = M.mix_clip([clips], ch, parts, T, strict=True)
            assert got[k].size == T * ch and M.same(got[k], want) is None, (ms, k, M.same(got[k], want))
            if ms == 0.0:   # gapless: the clips one after another, bit for bit (no -0.0 in them)
                joined = np.concatenate([clips[i] for i in g] + [np.zeros(0, F32)])
                assert M.same(got[k], joined) is None, k
            else:
                assert T == max(sum(frames[i] for i in g) - sum(min(96, frames[i], frames[j]) for i, j in zip(g, g[1:])), 0)
        alone = ctx.mix([clips[5], clips[0]], rate, ch, *flo_amd.concat_parts([frames[5], frames[0]], rate, ms))
        assert M.same(alone, got[3]) is None
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
    """a mixed lossy batch against a batch of the model's output uploaded the usual way: the same files (so the padding
    behind the clips, pcm_written and the plan are right), the same analysis, the same resampled, normalised and edited audio"""
    rng = np.random.default_rng(33)
    sr, ch = 44100, 2
    lens = (6000, 1, 0, 2500, 1024)
    clips = [(rng.uniform(-0.5, 0.5, n * ch) * np.repeat(np.sin(np.arange(n) / 300.0) ** 2 + 0.05, ch)).astype(F32) for n in lens]
    bed = [(rng.uniform(-0.05, 0.05, 6100 * ch)).astype(F32)]
    parts = [M.part(0, 0, 0, 0, 6000, 100, 1.0, 64, 64), M.part(0, 0, 1, 500, 5600, 0, 0.5), M.part(1, 3, 0, 3, 2000, 5), M.part(1, 4, 0, 0, 1024, 1500, -0.5, 0, 200),
             M.part(3, 1, 0, 0, 1, 0), M.part(4, 0, 1, 0, 4096, 0, 0.25)]
    T = [6149, 2600, 0, 1, 4096, 700]
    src = _batch_of(ctx, clips, sr, ch, flo_amd.MODE_LOSSY, 0.55)
    other = _batch_of(ctx, bed, sr, ch)
    try:
        out = src.mix(parts, T, others=(other,))
        want = M.mix([clips, bed], ch, parts, T, strict=True)
        up = _batch_of(ctx, want, sr, ch, flo_amd.MODE_LOSSY, 0.55)
        try:
            assert out.n_interleaved == up.n_interleaved and out.channels == ch and out.sample_rate == sr
            for a, b in zip(out.analyze_all(), up.analyze_all()):
                _same_analysis(a, b)
            steps = {"resample": lambda s: s.resample(48000), "normalize": lambda s: s.normalize(target_lufs=-20.0)[0],
                     "edit": lambda s: s.edit([dict(clip=0, start=7, frames=3000, pad_head=2, fade_in=9), dict(clip=4)])}
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
        other.close()


def test_errors_leave_no_batch_and_a_usable_context(ctx):
    clips = [np.arange(20, dtype=F32), np.arange(8, dtype=F32)]
    big = 1 << 64
    src = _batch_of(ctx, clips, 48000, 2)
    mono = _batch_of(ctx, [np.zeros(4, F32)], 48000, 1)
    slow = _batch_of(ctx, [np.zeros(4, F32)], 44100, 2)
    empty = flo_amd.Batch(ctx, flo_amd.MODE_LOSSLESS, [8], 48000, 2, 0)
    other_ctx = flo_amd.Context(0)
    try:
        foreign = _batch_of(other_ctx, [np.zeros(4, F32)], 48000, 2)
        most = (2 ** 64 - 1) // 8 // 2
        cases = [([src], [4], [M.part(1, 0, 0, 0, 1)], "out "), ([src], [4, 4], [M.part(1, 0, 0, 0, 1), M.part(0, 0, 0, 0, 1)], "out must not decrease"),
                 ([src], [4], [M.part(0, 0, 1, 0, 1)], "batch"), ([src], [4], [M.part(0, 2, 0, 0, 1)], "clip"),
                 ([src, src], [4], [M.part(0, 2, 1, 0, 1)], "clip"),
                 ([src], [4], [M.part(0, 0, 0, 0, 4, fade_in=5)], "fade_in"), ([src], [4], [M.part(0, 0, 0, 0, 4, fade_out=5)], "fade_out"),
                 ([src], [4], [M.part(0, 0, 0, 0, 1 << 24, fade_in=1 << 24)], "fade_in"), ([src], [4], [M.part(0, 0, 0, 0, 1 << 24, fade_out=1 << 24)], "fade_out"),
                 ([src], [4], [M.part(0, 0, 0, 0, 4, gain=float("nan"))], "gain"), ([src], [4], [M.part(0, 0, 0, 0, 4, gain=float("inf"))], "gain"),
                 ([src], [4], [M.part(0, 0, 0, 0, big - 3, at=3)], "at + frames"), ([src], [4], [M.part(0, 0, 0, 5, big - 5)], "start + frames"),
                 ([src], [most + 1], [], "out_frames"), ([src], [4, 1 << 45], [], "tiles"),
                 ([src, None], [4], [], "source 1 is NULL"), ([src, mono], [4], [], "channels"), ([src, slow], [4], [], "sample_rate"),
                 ([src, foreign], [4], [], "context")]
        for srcs, T, parts, word in cases:
            rc, h = _raw_mix(ctx, srcs, parts, T)
            msg = ctx._L.flo_last_error(ctx._h).decode()
            assert rc == 1 and word in msg and msg.startswith("flo_batch_mix: "), (word, rc, msg)
            assert not h.value, word
            if srcs == [src] and len(T) == 1 and word != "batch":   # the same refusal through flo_mix
                rc, out, n = _raw_alone(ctx, clips, 48000, 2, parts, T[0])
                msg = ctx._L.flo_last_error(ctx._h).decode()
                assert rc == 1 and word.strip() in msg and msg.startswith("flo_mix: ") and not out.value and n.value == 0, (word, msg)
        for parts, word in (([M.part(0, 0, 1, 0, 1)], "batch"), ([M.part(1, 0, 0, 0, 1)], "out")):   # flo_mix has one source and one output
            rc, out, n = _raw_alone(ctx, clips, 48000, 2, parts, 4)
            msg = ctx._L.flo_last_error(ctx._h).decode()
            assert rc == 1 and msg.startswith("flo_mix: " + word) and not out.value, msg
        rc, h = _raw_mix(ctx, [], [], [4])   # no source: no context to carry a message
        assert rc == 1 and not h.value
        # a source that a part names holds no PCM yet: FLO_ERR_STATE; unnamed, it does not matter
        rc, h = _raw_mix(ctx, [src, empty], [M.part(0, 0, 1, 0, 1)], [4])
        assert rc != 0 and "no PCM" in ctx._L.flo_last_error(ctx._h).decode() and not h.value
        with pytest.raises(flo_amd.FloError, match="no PCM"):
            empty.mix([dict(out=0, clip=0)])
        ok = _mix_batch(ctx, [src, empty], [M.part(0, 1, 0, 1, 2, 1)], [4])
        assert ok.download_pcm(0).tolist() == [0, 0, 2, 3, 4, 5, 0, 0]
        ok.close()
        foreign.close()
    finally:
        other_ctx.close()
        for b in (src, mono, slow, empty):
            b.close()


def test_python_faces_empty_batches_and_defaults(ctx):
    rng = np.random.default_rng(5)
    x = rng.uniform(-0.9, 0.9, 3000 * 2).astype(F32)
    odd = rng.uniform(-0.1, 0.1, 1001).astype(F32)   # an odd count: the partial frame is not part of the clip
    b = _batch_of(ctx, [x, odd], 48000, 2)
    try:
        out = b.mix([dict(out=0, clip=0), dict(out=0, clip=1, at=2900, gain=0.5), dict(out=2, clip=1, start=10, fade_in=20, fade_out=30)])
        try:
            assert out.n_clips == 3 and out.n_interleaved == [3400 * 2, 0, 490 * 2]
            parts = [M.part(0, 0, 0, 0, 3000), M.part(0, 1, 0, 0, 500, 2900, 0.5), M.part(2, 1, 0, 10, 490, 0, 1.0, 20, 30)]
            want = M.mix([[x, odd]], 2, parts, [3400, 0, 490], strict=True)
            for k in range(3):
                assert M.same(out.download_pcm(k), want[k]) is None, k
            again = out.mix([_native.MixPart(0, 100, 5, 0, 0, 2, 0, 0, -1.0)], [200], others=(b,))   # a mixed batch as a source
            assert M.same(again.download_pcm(0), M.mix_clip([want], 2, [M.part(0, 2, 0, 0, 100, 5, -1.0)], 200)) is None
            again.close()
        finally:
            out.close()
        none = b.mix([])
        assert none.n_clips == 0
        none.close()
        silent = b.mix([], [5, 0])
        assert silent.download_pcm(0).tolist() == [0.0] * 10 and not silent.download_pcm(0).view(np.uint32).any()
        silent.close()
        with pytest.raises(flo_amd.FloError, match="unknown keys"):
            b.mix([dict(out=0, clip=0, fade=3)])
    finally:
        b.close()
    one = ctx.mix([x, odd], 48000, 2, [dict(out=0, clip=0, frames=100), dict(out=0, clip=1, at=50, gain=-1.0)])
    assert one.size == 550 * 2
    assert M.same(one, M.mix_clip([[x, odd]], 2, [M.part(0, 0, 0, 0, 100), M.part(0, 1, 0, 0, 500, 50, -1.0)], 550)) is None
    assert ctx.mix([], 48000, 2, []).size == 0 and ctx.mix([], 48000, 2, [], 3).tolist() == [0.0] * 6
    both = flo_amd.concat([x, odd], 48000, 2)
    assert M.same(both, np.concatenate([x, odd[:1000]])) is None
    assert M.same(flo_amd.mix([x], 48000, 2, [dict(out=0, clip=0)]), x) is None
    empty = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [], 44100, 2, 0.55)
    try:
        out = empty.mix([], [7])
        assert out.n_clips == 1 and not out.download_pcm(0).view(np.uint32).any()
        out.close()
        out = empty.concat([])
        assert out.n_clips == 0
        out.close()
    finally:
        empty.close()


def test_cli_mix_and_concat(ctx, tmp_path, capsys):
    from flo_amd import cli
    from flo_amd.wav import read_wav_bytes, write_wav_bytes
    rng = np.random.default_rng(3)
    sr = 48000
    a, b = rng.uniform(-0.2, 0.2, 2 * 6000).astype(F32), rng.uniform(-0.2, 0.2, 2 * 2500).astype(F32)
    wa, wb, outp, mono = tmp_path / "a.wav", tmp_path / "b.wav", tmp_path / "out.wav", tmp_path / "m.wav"
    wa.write_bytes(write_wav_bytes(a, sr, 2))
    wb.write_bytes(write_wav_bytes(b, sr, 2))
    mono.write_bytes(write_wav_bytes(a[::2].copy(), sr, 1))
    sa, sb = (np.ascontiguousarray(read_wav_bytes(p.read_bytes())[0], F32) for p in (wa, wb))
    assert cli.main(["mix", str(wa), str(wb), "--out", str(outp), "--gains", "1,0.5", "--at-ms", "0,100"]) == 0
    got, rate, ch = read_wav_bytes(outp.read_bytes())
    want = M.mix_clip([[sa, sb]], 2, [M.part(0, 0, 0, 0, 6000), M.part(0, 1, 0, 0, 2500, 4800, 0.5)], 7300)
    assert (rate, ch) == (sr, 2) and M.same(np.ascontiguousarray(got, F32), want) is None
    assert cli.main(["concat", str(wa), str(wb), "--out", str(outp), "--crossfade-ms", "10"]) == 0
    got, rate, ch = read_wav_bytes(outp.read_bytes())
    parts, T = flo_amd.concat_parts([6000, 2500], sr, 10.0)
    assert T == 8020 and M.same(np.ascontiguousarray(got, F32), M.mix_clip([[sa, sb]], 2, parts, T)) is None
    assert cli.main(["concat", str(wa), str(mono), "--out", str(outp)]) != 0
    assert "resample" in capsys.readouterr().err


def test_the_scenario_under_every_fill(ctx):
    """A of tests/mix_recycled.py with the switch off and under every fill, in the shape of test_fill"""
    assert "mix" in [s["name"] for s in S.LEFTOVERS]
    records = []
    try:
        for fill in S.FILLS:
            flo_amd.debug_pool_fill(fill)
            records.append(mix_recycled.mix_a(ctx))
    finally:
        flo_amd.debug_pool_fill(None)
    for fill, rec in zip(S.FILLS[1:], records[1:]):
        diff = S.first_difference(records[0], rec)
        assert diff is None, ("mix", "fill %s against the switch off" % ("off" if fill is None else hex(fill)), diff)
