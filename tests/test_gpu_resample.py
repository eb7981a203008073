"""Sample-rate conversion on the device (flo_batch_resample, flo_resample and their Python / CLI faces).

The reference of every output is a numpy f64 dot product over the table flo_resample_filter returned, with the f32 inputs
as given: y[j] = sum_k h[p][k] x[i + k - T/2 + 1], i = floor(j M / L), p = (j M) mod L, x zero outside the clip. The bound
per output is the standard one for T products and T - 1 additions in f32 in any order, with or without FMA,
    |y - y_ref| <= (T + 1) 2^-24 sum_k |h_k x_k| + T 2^-126
(the second term allows flushed denormals); no other tolerance is used. Every output of every clip is compared."""
import math
import os

import numpy as np
import pytest

import flo_amd
from conftest import EXAMPLES
from flo_amd import cli
from flo_amd.wav import read_wav_bytes
from gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

PAIRS = [(48000, 44100), (44100, 48000), (96000, 44100), (8000, 44100), (44100, 8000), (44100, 22050), (22050, 44100)]
CASES = [(a, b, ch) for a, b in PAIRS for ch in (1, 2)] + [(48000, 44100, 6)]
ERR_ARG = 1


def _n_in_for(n_out, L, M):
    """the fewest input frames that give at least n_out output frames (exactly n_out wherever some n_in gives it: always
    when M >= L; an upsampler's counts skip values, and the next count above is taken)"""
    if n_out == 0:
        return 0
    n = ((n_out - 1) * M) // L + 1   # the smallest n with ceil(n L / M) >= n_out
    assert -((-n * L) // M) >= n_out and (n == 1 or -((-(n - 1) * L) // M) < n_out)
    return n


def _lengths(info):
    L, M, T, tile = info["L"], info["M"], info["taps"], info["tile_outputs"]
    return [_n_in_for(n, L, M) for n in (0, 1, 2, T // 2, tile - 1, tile, tile + 1, 2 * tile + 17)]


def _clips(info, ch, seed):
    """per length: uniform noise in [-1, 1]; a unit impulse at the first input frame; one at the last"""
    rng = np.random.default_rng(seed)
    clips = []
    for n in _lengths(info):
        clips.append(rng.uniform(-1.0, 1.0, n * ch).astype(np.float32))
        first, last = np.zeros(n * ch, np.float32), np.zeros(n * ch, np.float32)
        if n:
            first[:ch] = 1.0
            last[-ch:] = 1.0
        clips += [first, last]
    return clips


def _reference(x, ch, info, table):
    """(y_ref, bound) of one interleaved clip, f64, shaped [n_out * ch]"""
    L, M, T = info["L"], info["M"], info["taps"]
    n_in = x.size // ch
    n_out = -((-n_in * L) // M)
    h = table.astype(np.float64)
    y, bound = np.zeros((n_out, ch)), np.zeros((n_out, ch))
    xp = np.zeros((n_in + 2 * T + M + 2, ch))
    xp[T:T + n_in] = x.reshape(n_in, ch).astype(np.float64)
    step = max(1, (1 << 22) // T)
    for j0 in range(0, n_out, step):
        j = np.arange(j0, min(n_out, j0 + step), dtype=np.int64)
        i, p = (j * M) // L, (j * M) % L
        idx = (i - T // 2 + 1 + T)[:, None] + np.arange(T)[None, :]
        for c in range(ch):
            prod = h[p] * xp[idx, c]
            y[j, c] = prod.sum(axis=1)
            bound[j, c] = (T + 1) * 2.0 ** -24 * np.abs(prod).sum(axis=1) + T * 2.0 ** -126
    return y.reshape(-1), bound.reshape(-1)


_made = {}


def _case(ctx, in_rate, out_rate, ch):
    """the mixed batch of a case, converted once: (info, table, clips, outputs of the batch)"""
    key = (in_rate, out_rate, ch)
    if key not in _made:
        info, table = flo_amd.resample_filter(in_rate, out_rate)
        clips = _clips(info, ch, seed=in_rate * 7 + out_rate + ch)
        b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [c.size for c in clips], in_rate, ch, 0.5)
        try:
            for i, c in enumerate(clips):
                b.upload(i, c)
            r = b.resample(out_rate)
            try:
                assert r.sample_rate == out_rate and r.channels == ch and r.n_clips == len(clips)
                outs = [r.download_pcm(i) for i in range(r.n_clips)]
            finally:
                r.close()
            for i, c in enumerate(clips):   # the source batch is unchanged
                assert np.array_equal(b.download_pcm(i).view(np.uint32), c.view(np.uint32)), (key, i)
        finally:
            b.close()
        _made[key] = (info, table, clips, outs)
    return _made[key]


@pytest.mark.parametrize("in_rate,out_rate,ch", CASES)
def test_every_output_against_the_f64_reference(ctx, in_rate, out_rate, ch):
    info, table, clips, outs = _case(ctx, in_rate, out_rate, ch)
    L, M = info["L"], info["M"]
    worst = 0.0
    for i, (x, y) in enumerate(zip(clips, outs)):
        n_in = x.size // ch
        assert y.size == -((-n_in * L) // M) * ch, (i, n_in, y.size)
        if not y.size:
            continue
        ref, bound = _reference(x, ch, info, table)
        err = np.abs(y.astype(np.float64) - ref)
        worst = max(worst, float((err / bound).max()))
        bad = np.flatnonzero(err > bound)
        assert bad.size == 0, (in_rate, out_rate, ch, "clip", i, "n_in", n_in, "first bad output", int(bad[0]) // ch,
                               float(err[bad[0]]), float(bound[bad[0]]))
    print(f"{in_rate}->{out_rate} x{ch}: tile {info['tile_outputs']}, taps {info['taps']}, worst |y - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("in_rate,out_rate,ch", CASES)
def test_a_clip_does_not_depend_on_its_batch(ctx, in_rate, out_rate, ch):
    info, table, clips, outs = _case(ctx, in_rate, out_rate, ch)
    for i, (x, y) in enumerate(zip(clips, outs)):
        alone = ctx.resample(x, in_rate, out_rate, ch)
        assert alone.dtype == np.float32 and np.array_equal(alone.view(np.uint32), y.view(np.uint32)), (in_rate, out_rate, ch, i)
    many = flo_amd.resample_many(clips[:6], in_rate, out_rate, ch, ctx=ctx)   # a lossless batch, other neighbours
    for i in range(6):
        assert np.array_equal(many[i].view(np.uint32), outs[i].view(np.uint32)), (in_rate, out_rate, ch, i)


@pytest.mark.parametrize("mode", [flo_amd.MODE_LOSSY, flo_amd.MODE_LOSSLESS])
def test_equal_rates_copy_bit_for_bit(ctx, mode):
    rng = np.random.default_rng(5)
    clips = [rng.uniform(-1, 1, n * 2).astype(np.float32) for n in (0, 1, 1023, 5000)]
    clips[2][7] = np.float32(-0.0)
    clips[3][11] = np.float32(1e-42)   # a denormal stays a denormal
    b = flo_amd.Batch(ctx, mode, [c.size for c in clips], 48000, 2, 0.5 if mode == flo_amd.MODE_LOSSY else 5)
    try:
        for i, c in enumerate(clips):
            b.upload(i, c)
        r = b.resample(48000)
        try:
            for i, c in enumerate(clips):
                assert np.array_equal(r.download_pcm(i).view(np.uint32), c.view(np.uint32)), i
        finally:
            r.close()
    finally:
        b.close()
    assert np.array_equal(ctx.resample(clips[3], 48000, 48000, 2).view(np.uint32), clips[3].view(np.uint32))


def _device_floats(batch, clip, n):
    import ctypes as C
    out = np.empty(n, np.float32)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data, batch._L.flo_batch_clip_device_data(batch._h, clip), n * 4, 2) == 0
    return out


@pytest.mark.parametrize("mode", [flo_amd.MODE_LOSSY, flo_amd.MODE_LOSSLESS])
def test_the_result_is_a_proper_batch(ctx, mode):
    """resampled 48 kHz stereo encodes to the files the one-shot encoders make of the new batch's PCM at 44100"""
    info, _ = flo_amd.resample_filter(48000, 44100)
    L, M, tile = info["L"], info["M"], info["tile_outputs"]
    rng = np.random.default_rng(9)
    lens = [_n_in_for(tile + 3, L, M), _n_in_for(5, L, M)]
    t = [np.arange(n) / 48000.0 for n in lens]
    clips = [np.stack([0.4 * np.sin(2 * np.pi * 440 * x) + 0.01 * rng.uniform(-1, 1, x.size),
                       0.3 * np.sin(2 * np.pi * 1000 * x)], axis=1).astype(np.float32).reshape(-1) for x in t]
    lossy = mode == flo_amd.MODE_LOSSY
    b = flo_amd.Batch(ctx, mode, [c.size for c in clips], 48000, 2, 0.55 if lossy else 5)
    try:
        for i, c in enumerate(clips):
            b.upload(i, c)
        r = b.resample(44100)
        try:
            assert [n // 2 for n in r.n_interleaved] == [tile + 3, 5]
            pcm = [r.download_pcm(i) for i in range(2)]
            if lossy:   # the zero tail a lossy batch relies on: up to hops * 1024 frames behind the clip
                for i, n in enumerate(r.n_interleaved):
                    hops = (n // 2 + 1024 + 1023) // 1024
                    whole = _device_floats(r, i, hops * 1024 * 2)
                    assert np.array_equal(whole[:n].view(np.uint32), pcm[i].view(np.uint32)) and not whole[n:].any(), i
            r.encode()
            r.sync()
            for i in range(2):
                own = ctx.encode_lossy(pcm[i], 44100, 2, 0.55) if lossy else ctx.encode_lossless(pcm[i], 44100, 2, 16, 5)
                assert r.fetch(i) == own, (mode, i)
                assert flo_amd.probe_container(own).sample_rate == 44100
        finally:
            r.close()
        for i, c in enumerate(clips):
            assert np.array_equal(b.download_pcm(i).view(np.uint32), c.view(np.uint32)), i
    finally:
        b.close()


def test_partial_trailing_frame_is_not_carried_over(ctx):
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, 2 * 400 + 1).astype(np.float32)
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [x.size], 48000, 2, 0.5)
    try:
        b.upload(0, x)
        r = b.resample(44100)
        try:
            assert r.n_interleaved == [flo_amd.resample_out_frames(48000, 44100, 400) * 2]
            assert np.array_equal(r.download_pcm(0).view(np.uint32), ctx.resample(x[:-1], 48000, 44100, 2).view(np.uint32))
        finally:
            r.close()
    finally:
        b.close()


def test_errors(ctx):
    import ctypes as C
    L = ctx._L
    x = np.zeros(64, np.float32)
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [x.size], 44100, 2, 0.5)
    empty = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [], 44100, 2, 0.5)
    try:
        b.upload(0, x)
        h = C.c_void_p()
        for rate, word in ((44101, "L"), (0, "out_rate"), (400000, "out_rate"), (1, "taps")):
            assert L.flo_batch_resample(b._h, rate, C.byref(h)) == ERR_ARG and not h.value
            assert word in L.flo_last_error(ctx._h).decode(), (rate, L.flo_last_error(ctx._h))
            with pytest.raises(flo_amd.FloError):
                b.resample(rate)
        assert L.flo_batch_resample(None, 48000, C.byref(h)) == ERR_ARG
        assert L.flo_batch_resample(b._h, 48000, None) == ERR_ARG
        out, n = C.c_void_p(), C.c_size_t()
        assert L.flo_resample(ctx._h, x.ctypes.data, x.size, 44100, 44101, 2, C.byref(out), C.byref(n)) == ERR_ARG and not out.value
        assert "L" in L.flo_last_error(ctx._h).decode()
        assert L.flo_resample(ctx._h, x.ctypes.data, x.size, 44100, 48000, 0, C.byref(out), C.byref(n)) == ERR_ARG and not out.value
        assert L.flo_resample(ctx._h, x.ctypes.data, x.size, 44100, 48000, 9, C.byref(out), C.byref(n)) == ERR_ARG and not out.value
        assert L.flo_resample(ctx._h, None, 0, 44100, 48000, 2, C.byref(out), C.byref(n)) == 0 and n.value == 0
        L.flo_free(out)
        # a batch of no clips
        assert L.flo_batch_resample(empty._h, 48000, C.byref(h)) == 0 and h.value
        L.flo_batch_destroy(h)
        r = empty.resample(22050)
        assert r.n_clips == 0
        r.close()
        assert ctx.resample(np.zeros(0, np.float32), 44100, 48000, 2).size == 0
    finally:
        b.close()
        empty.close()


def test_cli_resample_and_encode_rate(tmp_path, capsys):
    audio = open(os.path.join(EXAMPLES, "audio.wav"), "rb").read()
    samples, sr, ch = read_wav_bytes(audio)
    assert sr != 22050
    wav = tmp_path / "audio.wav"
    wav.write_bytes(audio)
    out = tmp_path / "out.wav"
    assert cli.main(["resample", str(wav), str(out), "--rate", "22050"]) == 0
    got, gsr, gch = read_wav_bytes(out.read_bytes())
    want = flo_amd.resample(samples, sr, 22050, ch)
    assert (gsr, gch) == (22050, ch) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got.size == flo_amd.resample_out_frames(sr, 22050, samples.size // ch) * ch
    for extra in ([], ["--lossy", "--quality", "high"]):
        flo = tmp_path / "out.flo"
        assert cli.main(["encode", str(wav), str(flo), "--rate", "22050"] + extra) == 0
        data = flo.read_bytes()
        info = cli.flo_info(data)
        assert info["sample_rate"] == 22050 and info["channels"] == ch and info["crc_valid"]
        pcm = flo_amd.decode(data)
        assert pcm.size >= want.size
        if not extra:   # lossless at 16 bits: the converted audio, quantised
            assert float(np.abs(pcm[:want.size] - want).max()) <= 1.0 / 32767 + 1e-6
        md = cli.get_metadata(data)
        assert md is not None and abs(md["length_ms"] - 1000.0 * (want.size // ch) / 22050) <= 1.0
    capsys.readouterr()
    assert cli.main(["resample", str(wav), str(out), "--rate", "44101" if math.gcd(sr, 44101) == 1 else "1"]) == 1
    assert "Error" in capsys.readouterr().err
