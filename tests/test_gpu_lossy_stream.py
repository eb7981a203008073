"""The lossy streaming encoder (flo_stream_create_lossy / flo_stream_encode_ready): frames as they complete, byte for byte
the offline file's (flo_encode_lossy), however the input is cut into pushes and however many streams share a device pass.
Needs an MI355X."""
import struct

import numpy as np
import pytest

import flo_amd
from gpu_util import ctx  # noqa: F401
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FLO_ERR_ARG, FLO_ERR_STATE = 1, 4
CONFIGS = [(44100, 2, 0.55), (48000, 1, 0.3), (22050, 6, 0.8), (8000, 2, 1.0), (96000, 2, 0.0)]


def _toc(f: bytes):
    """[(frame_index, byte_offset, frame_size, timestamp_ms)], DATA"""
    tsz, dsz = struct.unpack_from("<QQ", f, 38)
    n = struct.unpack_from("<I", f, 70)[0]
    toc = [struct.unpack_from("<IQII", f, 74 + 20 * i) for i in range(n)]
    return toc, f[70 + tsz:70 + tsz + dsz]


def _file_frames(f: bytes):
    toc, data = _toc(f)
    return [(i, ts, 1024, data[off:off + size]) for (i, off, size, ts) in toc]


def _frames(frames):
    return [(fr.index, fr.timestamp_ms, fr.samples, fr.data) for fr in frames]


def _signal(n_sf, ch, seed):
    return O.synth_clip(n_sf, ch, clip_id=seed).astype(np.float32).reshape(-1)


def _pieces(x, ch, how, rng):
    if how == "whole":
        return [x]
    if how == "sample":   # one sample-frame per push
        return [x[i:i + ch] for i in range(0, x.size, ch)]
    if how == "odd":
        cuts = list(range(0, x.size, 1531)) + [x.size]
        return [x[a:b] for a, b in zip(cuts[:-1], cuts[1:])] or [x]
    cuts = np.sort(rng.integers(0, x.size + 1, size=max(1, x.size // 3000)))
    cuts = [0] + list(cuts) + [x.size]
    return [x[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


@pytest.mark.parametrize("sr,ch,q", CONFIGS)
def test_finalize_equals_offline_file(ctx, sr, ch, q):
    rng = np.random.default_rng(sr + ch)
    lengths = [0, 1, 1023, 1024, 1025, 3 * sr + 777, 301 * 1024 + 5]
    for n_sf in lengths:
        x = _signal(n_sf, ch, n_sf + 7)
        if n_sf == 1025:
            x = np.concatenate([x, np.float32([0.25] * (ch - 1 if ch > 1 else 0))])   # a trailing partial sample-frame
        want = ctx.encode_lossy(x, sr, ch, q, b"meta!")
        for how in ["whole", "odd", "random"] + (["sample"] if n_sf <= 4096 else []):
            e = flo_amd.LossyStreamingEncoder(sr, ch, q, ctx=ctx)
            for p in _pieces(x, ch, how, rng):
                e.push_samples(p)
                assert e.pending_samples() < 1024
            got = e.finalize(b"meta!")
            e.close()
            assert got == want, (sr, ch, q, n_sf, how)


@pytest.mark.parametrize("sr,ch,q", CONFIGS[:3])
def test_frames_as_they_complete(ctx, sr, ch, q):
    n_sf = 5 * 1024 + 300
    x = _signal(n_sf, ch, 11)
    want = _file_frames(ctx.encode_lossy(x, sr, ch, q))
    e = flo_amd.LossyStreamingEncoder(sr, ch, q, ctx=ctx)
    got, pushed = [], 0
    for a in range(0, n_sf, 700):
        b = min(n_sf, a + 700)
        e.push_samples(x[a * ch:b * ch])
        pushed = b
        complete = pushed // 1024
        assert e.pending_frames() == complete - len(got)
        assert e.pending_samples() == pushed - complete * 1024
        while (fr := e.next_frame()) is not None:
            got.append(fr)
        assert len(got) == complete
    fr = e.flush()
    assert e.pending_frames() == len(want) - len(got) - 1
    got.append(fr)
    while (fr := e.next_frame()) is not None:
        got.append(fr)
    assert _frames(got) == want
    assert e.flush() is None


def test_chunking_does_not_matter(ctx):
    sr, ch, q = 48000, 2, 0.55
    n_sf = 400 * 1024 + 333
    x = _signal(n_sf, ch, 5)
    want = _file_frames(ctx.encode_lossy(x, sr, ch, q))
    for per in (1, 7, 130, None):
        e = flo_amd.LossyStreamingEncoder(sr, ch, q, ctx=ctx)
        step = n_sf if per is None else per * 1024
        for a in range(0, n_sf, step):
            e.push_samples(x[a * ch:min(n_sf, a + step) * ch])
        got = []
        while (fr := e.next_frame()) is not None:
            got.append(fr)
        fr = e.flush()
        while fr is not None:
            got.append(fr)
            fr = e.next_frame()
        assert _frames(got) == want, per


def test_encode_streams_many_mixed(ctx):
    rng = np.random.default_rng(3)
    cfgs = [(44100, 2, 0.55), (48000, 1, 0.3), (48000, 6, 0.8), (22050, 2, 0.0)]
    encs, twins, sigs, kinds = [], [], [], []
    for i in range(72):
        if i % 9 == 8:   # lossless streams
            sr, ch = (44100, 2) if i % 2 else (16000, 1)
            encs.append(flo_amd.StreamingEncoder(sr, ch, 16, ctx=ctx))
            twins.append(flo_amd.StreamingEncoder(sr, ch, 16, ctx=ctx))
            kinds.append(("ll", sr, ch, None))
        else:
            sr, ch, q = cfgs[i % len(cfgs)]
            encs.append(flo_amd.LossyStreamingEncoder(sr, ch, q, ctx=ctx))
            twins.append(None)
            kinds.append(("lossy", sr, ch, q))
        sigs.append([])
    for tick in range(3):
        for i, e in enumerate(encs):
            ch = kinds[i][2]
            r = rng.integers(0, 6)
            n_sf = [0, 100, 1023, 1024 * int(rng.integers(1, 4)), 3000 + int(rng.integers(0, 500)), 5000 * (tick + 1)][r]
            if i == 5 and tick == 1:
                n_sf = 2100 * 1024   # thousands of frames in one call
            x = _signal(n_sf, ch, 1000 * tick + i)
            sigs[i].append(x)
            e.append_samples(x)
            if twins[i] is not None:
                twins[i].push_samples(x)
        res = flo_amd.encode_streams(encs)
        assert not res.status.any(), res.errors
        for i, e in enumerate(encs):
            assert e.pending_samples() < (kinds[i][1] if kinds[i][0] == "ll" else 1024)
    for i, e in enumerate(encs):
        if kinds[i][0] == "ll":
            got, want = [], []
            while (fr := e.next_frame()) is not None:
                got.append(fr)
            while (fr := twins[i].next_frame()) is not None:
                want.append(fr)
            assert _frames(got) == _frames(want), i
            assert e.finalize() == twins[i].finalize()
        else:
            _, sr, ch, q = kinds[i]
            x = np.concatenate(sigs[i])
            assert e.finalize() == ctx.encode_lossy(x, sr, ch, q), i
        e.close()


def test_flush_then_push_and_partial_finalize(ctx):
    sr, ch, q = 44100, 2, 0.55
    x = _signal(10 * 1024 + 17, ch, 9)
    want = ctx.encode_lossy(x, sr, ch, q)
    toc, data = _toc(want)
    e = flo_amd.LossyStreamingEncoder(sr, ch, q, ctx=ctx)
    e.push_samples(x)
    pulled = [e.next_frame() for _ in range(4)]
    assert _frames(pulled) == _file_frames(want)[:4]
    f = e.finalize()
    rest = _toc(f)
    assert [t[0] for t in rest[0]] == [t[0] for t in toc[4:]]
    assert [t[3] for t in rest[0]] == [t[3] for t in toc[4:]]
    assert rest[1] == data[toc[4][1]:]
    with pytest.raises(flo_amd.FloError):
        e.push_samples(x[:10])
    with pytest.raises(flo_amd.FloError):
        e.append_samples(x[:10])
    e2 = flo_amd.LossyStreamingEncoder(sr, ch, q, ctx=ctx)
    e2.push_samples(x)
    e2.flush()
    rc = ctx._L.flo_stream_push(e2._h, x.ctypes.data, 2)
    assert rc == FLO_ERR_STATE
    e.close()
    e2.close()


def test_nonfinite_and_loud_input(ctx):
    sr, ch, q = 48000, 2, 0.55
    x = _signal(6 * 1024 + 100, ch, 4) * 1e6
    x[500] = np.nan
    x[3001] = np.inf
    x[7000] = -np.inf
    x[9000:9100] = 3e38
    want = ctx.encode_lossy(x, sr, ch, q)
    e = flo_amd.LossyStreamingEncoder(sr, ch, q, ctx=ctx)
    for a in range(0, x.size, 2049):
        e.push_samples(x[a:a + 2049])
    assert e.finalize() == want


def test_argument_errors(ctx):
    for bad in (0, 9):
        with pytest.raises(flo_amd.FloError):
            flo_amd.LossyStreamingEncoder(44100, bad, 0.5, ctx=ctx)
    e = flo_amd.LossyStreamingEncoder(44100, 2, flo_amd.QualityPreset.High, ctx=ctx)
    assert e.quality == flo_amd.QualityPreset.High.as_f32()
    other = flo_amd.Context(0)
    try:
        f = flo_amd.LossyStreamingEncoder(44100, 2, 0.5, ctx=other)
        x = _signal(3000, 2, 1)
        e.append_samples(x)
        f.append_samples(x)
        res = flo_amd.encode_streams([e, f], ctx=ctx)
        assert list(res.status) == [0, FLO_ERR_ARG] and res.errors[1]
        assert e.pending_frames() == 2 and f.pending_frames() == 0
        f.close()
    finally:
        other.close()
    e.close()
    with pytest.raises(flo_amd.FloError):
        flo_amd.encode_streams([e])
    with pytest.raises(flo_amd.FloError):
        e.push_samples(np.zeros(4, np.float32))


def test_scale_1024_streams_equal_batch(ctx):
    sr, ch, q = 48000, 2, 0.55
    n_sf = 2 * sr
    clips = [_signal(n_sf, ch, i) for i in range(1024)]
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [c.size for c in clips], sr, ch, q)
    try:
        for i, c in enumerate(clips):
            b.upload(i, c)
        b.encode(0)
        b.sync()
        want = [b.fetch(i) for i in range(len(clips))]
    finally:
        b.close()
    encs = [flo_amd.LossyStreamingEncoder(sr, ch, q, ctx=ctx) for _ in clips]
    tick = sr // 2
    for a in range(0, n_sf, tick):
        for e, c in zip(encs, clips):
            e.append_samples(c[a * ch:(a + tick) * ch])
        res = flo_amd.encode_streams(encs)
        assert not res.status.any()
    for i, e in enumerate(encs):
        assert e.finalize() == want[i], i
        e.close()
