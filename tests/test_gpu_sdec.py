"""The streaming decoder on the device (flo_sdec_*): next_frame and the batched decode_streams against flo_decode (bit for
bit) and against tests/sdec_model.py (bit for bit lossless, 2e-6 lossy: the oracle's FFT is not the device's), under
random feeds, interleaved calls and frame caps that cut the 16-frame runs at every place. Needs an MI355X."""
import glob
import os
import struct

import numpy as np
import pytest

import flo_amd
import flofile
from conftest import EXAMPLES
from gpu_util import ctx  # noqa: F401
from oracle import oracle as O
from sdec_model import READY, FINISHED, ModelError, StreamingDecoderModel

pytestmark = pytest.mark.gpu

LOSSY_TOL = 2e-6
FILES = sorted(glob.glob(os.path.join(EXAMPLES, "*.flo")))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _model_ready(m, cap):
    """what one decode_ready does to the model: (frames, status message or None)"""
    if m.state != READY:
        return [], None
    if m.current >= len(m.toc):
        m.state = FINISHED
        return [], None
    out = []
    while m.current < m._count_complete() and (cap == 0 or len(out) < cap):
        try:
            out.append(m.next_frame())
        except ModelError as e:
            return out, str(e)
    return out, None


def _same(got, want, lossy):
    assert got.size == want.size
    if lossy:
        assert float(np.abs(got - want).max(initial=0)) <= LOSSY_TOL
    else:
        assert np.array_equal(_bits(got), _bits(want))


def _drive(ctx, b, rng, caps=(0, 1, 15, 16, 17)):
    """feed `b` in random chunks; after each feed one of: next_frame, decode_streams with a cap, or nothing"""
    d, m = flo_amd.StreamingDecoder(ctx), StreamingDecoderModel()
    got_all = []
    at = 0
    while at < len(b) or d.state() == flo_amd.DecoderState.Ready:
        if at < len(b):
            step = int(rng.choice([1, 7, 70, 333, 4096, 60000, len(b)]))
            assert d.feed(b[at:at + step]) == m.feed(b[at:at + step])
            at += step
        op = int(rng.integers(0, 3)) if at < len(b) else 1 + int(rng.integers(0, 2))
        if op == 1:
            for _ in range(int(rng.integers(1, 4))):
                try:
                    want = m.next_frame()
                except ModelError:
                    with pytest.raises(flo_amd.FloError):
                        d.next_frame()
                    return d, m, got_all, True
                got = d.next_frame()
                assert (got is None) == (want is None)
                if got is not None:
                    _same(got, want, m.is_lossy)
                    got_all.append(got)
        elif op == 2:
            cap = int(rng.choice(caps))
            wants, err = _model_ready(m, cap)
            r = flo_amd.decode_streams([d], max_frames=cap)
            out = r.out.cpu().numpy()
            assert int(r.offsets[1]) == sum(w.size for w in wants)
            if wants:
                _same(out, np.concatenate(wants), m.is_lossy)
                got_all.append(out)
            assert (r.status[0] != 0) == (err is not None)
            if err is not None:
                return d, m, got_all, True
        assert int(d.state()) == m.state and d.current_frame_index() == m.current
        if at >= len(b) and d.state() != flo_amd.DecoderState.Ready:
            break
    return d, m, got_all, False


def _check_file(ctx, b, seed):
    rng = np.random.default_rng(seed)
    d, m, parts, failed = _drive(ctx, b, rng)
    assert not failed
    got = np.concatenate(parts) if parts else np.zeros(0, np.float32)
    full = ctx.decode(b)
    assert np.array_equal(_bits(got), _bits(full))
    assert d.state() == flo_amd.DecoderState.Finished


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_golden_files(ctx, path):
    b = open(path, "rb").read()
    for seed in range(3):
        _check_file(ctx, b, seed)


@pytest.mark.parametrize("q", [0.35, 0.55, 0.95])
@pytest.mark.parametrize("ch,sr", [(1, 44100), (2, 44100), (2, 96000)])
@pytest.mark.parametrize("frames", [1, 17, 33])
def test_lossy_synthetic(ctx, q, ch, sr, frames):
    n = frames * 1024 - 300 if frames > 1 else 500
    pcm = O.synth_clip(n, ch, clip_id=frames * 7 + ch)
    b = ctx.encode_lossy(pcm, sr, ch, q)
    _check_file(ctx, b, frames + ch)


@pytest.mark.parametrize("level", [0, 5, 9])
@pytest.mark.parametrize("ch", [1, 2])
def test_lossless_synthetic(ctx, level, ch):
    pcm = O.synth_clip(int(2.5 * 44100), ch, clip_id=level)
    b = ctx.encode_lossless(pcm, 44100, ch, 16, level)
    _check_file(ctx, b, level)


def _lossy_with_broken(ctx, where):
    """an encoder-made stereo file whose frame `where` does not deserialise (block size byte 7: deserialize_frame -> None)"""
    pcm = O.synth_clip(20 * 1024, 2, clip_id=3)
    b = bytearray(ctx.encode_lossy(pcm, 44100, 2, 0.55))
    toc_n = struct.unpack_from("<I", b, 70)[0]
    ds = 70 + struct.unpack_from("<Q", b, 38)[0]
    off = struct.unpack_from("<Q", b, 74 + 20 * where + 4)[0]
    assert b[ds + off] == 253 and toc_n == 21
    b[ds + off + 10] = 7
    return bytes(b)


@pytest.mark.parametrize("where", [0, 1, 7])
def test_undeserialisable_frame(ctx, where):
    b = _lossy_with_broken(ctx, where)
    for seed in range(3):
        rng = np.random.default_rng(seed)
        d, m, parts, failed = _drive(ctx, b, rng)
        assert not failed
        # the empty frame is consumed; the overlap goes on from the frame before it
        want = []
        m2 = StreamingDecoderModel()
        m2.feed(b)
        while True:
            x = m2.next_frame()
            if x is None:
                break
            want.append(x)
        assert len(want) == 21 and want[where].size == 0
        got = np.concatenate(parts)
        _same(got, np.concatenate(want), True)
    # decode_available skips the frame (flo_decode fails on the file)
    d = flo_amd.StreamingDecoder(ctx)
    d.feed(b)
    x = d.decode_available()
    _same(x, np.concatenate(want), True)
    assert d.state() == flo_amd.DecoderState.Finished
    with pytest.raises(flo_amd.FloError):
        ctx.decode(b)


def test_reset_reuse_and_decode_available(ctx):
    files = [open(p, "rb").read() for p in FILES[:4]]
    d = flo_amd.StreamingDecoder(ctx)
    for b in files + files[::-1]:
        d.reset()
        assert d.feed(b)
        k = min(2, d.available_frames() - 1)   # a partial drain: the decoder stays Ready
        first = [d.next_frame() for _ in range(k)]
        assert d.current_frame_index() == k and all(x is not None for x in first)
        rest = d.decode_available()   # the whole buffer from frame 0, whatever current_frame is
        assert np.array_equal(_bits(rest), _bits(ctx.decode(b)))
        assert d.state() == flo_amd.DecoderState.Finished
        assert d.next_frame() is None
    # an incomplete buffer: the reader's error, the state unchanged
    d.reset()
    d.feed(files[0][:len(files[0]) // 2])
    with pytest.raises(flo_amd.FloError):
        d.decode_available()
    assert d.state() == flo_amd.DecoderState.Ready


def test_many_streams_in_rounds(ctx):
    import torch
    rng = np.random.default_rng(11)
    ch, sr = 2, 44100
    srcs = []
    for k in range(6):
        pcm = O.synth_clip(int((1.5 + k) * sr), ch, clip_id=200 + k)
        srcs.append(ctx.encode_lossy(pcm, sr, ch, 0.3 + 0.1 * k))
        srcs.append(ctx.encode_lossless(pcm, sr, ch, 16, k))
    ok = {"coeffs": [1], "shift": 0, "k": 2, "residuals": b"\x55" * 40}
    bad = flofile.build_lossless(sr, ch, [(1, 64, 0, [ok, ok]), (1, 64, 0, [bytes([13]) + b"\0" * 8, ok])])
    n = 1100
    which = [int(rng.integers(0, len(srcs))) for _ in range(n)]
    which[5] = -1
    blobs = [bad if w < 0 else srcs[w] for w in which]
    decs = [flo_amd.StreamingDecoder(ctx) for _ in range(n)]
    models = [StreamingDecoderModel() for _ in range(n)]
    pos = [0] * n
    outs = [[] for _ in range(n)]
    s = torch.cuda.Stream()
    for rnd in range(8):
        for i in range(n):
            if i % 97 == 0 and rnd < 3:
                continue   # some stay WaitingForHeader for a while
            step = int(rng.integers(20000, 160000)) if rnd < 7 else 1 << 30
            chunk = blobs[i][pos[i]:pos[i] + step]
            pos[i] += len(chunk)
            assert decs[i].feed(chunk) == models[i].feed(chunk)
        with torch.cuda.stream(s):
            r = flo_amd.decode_streams(decs, max_frames=int(rng.choice([0, 3, 16])) if rnd < 7 else 0)
            host = r.out.cpu().numpy()
        for i in range(n):
            seg = host[int(r.offsets[i]):int(r.offsets[i + 1])]
            outs[i].append(seg)
            assert decs[i].current_frame_index() >= models[i].current
        # the model follows the decoder's own count of frames per call
        for i in range(n):
            want, err = [], None
            while models[i].current < decs[i].current_frame_index():
                x = models[i].next_frame()
                want.append(x)
            if r.status[i]:
                err = r.errors[i]
                with pytest.raises(ModelError, match=err):
                    models[i].next_frame()
                assert which[i] < 0 and err == "Invalid LPC order"
            elif models[i].state == READY and models[i].current >= len(models[i].toc) and decs[i].state() == flo_amd.DecoderState.Finished:
                models[i].next_frame()
            seg = outs[i][-1]
            _same(seg, np.concatenate(want) if want else np.zeros(0, np.float32), models[i].is_lossy)
            assert int(decs[i].state()) == models[i].state
    # one more call with nothing new: every drained stream moves to Finished, as a next_frame call returning None would
    r = flo_amd.decode_streams(decs)
    assert int(r.offsets[-1]) == 0
    for i in range(n):
        if which[i] >= 0:
            assert decs[i].state() == flo_amd.DecoderState.Finished
            assert np.array_equal(_bits(np.concatenate(outs[i])), _bits(ctx.decode(blobs[i])))
        else:
            assert int(r.status[i]) == 5 and decs[i].current_frame_index() == 1


def test_decode_streams_on_a_side_stream(ctx):
    import torch
    files = [open(p, "rb").read() for p in FILES if flo_amd.probe_container(open(p, "rb").read()).channels == 2
             and flo_amd.probe_container(open(p, "rb").read()).sample_rate == 44100]
    decs = []
    for b in files:
        d = flo_amd.StreamingDecoder(ctx)
        d.feed(b)
        decs.append(d)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        big = torch.full((1 << 24,), 7.0, device="cuda")   # queued work in front of the decode on the same stream
        r = flo_amd.decode_streams(decs)
        y = r.out * 1.0 + big[:1].sum() * 0
    s.synchronize()
    host = y.cpu().numpy()
    for i, b in enumerate(files):
        assert np.array_equal(_bits(host[int(r.offsets[i]):int(r.offsets[i + 1])]), _bits(ctx.decode(b)))


def test_reset_to_more_channels(ctx):
    """one decoder through lossy files of growing channel count (its device state must grow with them), decoded in
    calls of 20 frames - more than one run each - and with next_frame, against flo_decode"""
    files = []
    for k, ch in enumerate([1, 2, 1, 6, 2]):
        pcm = O.synth_clip(40 * 1024 + 77, ch, clip_id=300 + k)
        files.append(ctx.encode_lossy(pcm, 48000 if ch == 6 else 44100, ch, 0.55))
    d = flo_amd.StreamingDecoder(ctx)
    for k, b in enumerate(files):
        d.reset()
        d.feed(b)
        parts = []
        if k % 2:
            while True:
                x = d.next_frame()
                if x is None:
                    break
                parts.append(x)
        else:
            while d.state() == flo_amd.DecoderState.Ready:
                parts.append(flo_amd.decode_streams([d], max_frames=20).out.cpu().numpy())
        assert d.state() == flo_amd.DecoderState.Finished
        assert np.array_equal(_bits(np.concatenate(parts)), _bits(ctx.decode(b))), k


def test_runs_of_one_call_share_no_state(ctx):
    """streams whose every call carries several runs (43 - 60 blocks), many streams per launch, several calls: the first
    run of a call reads the overlap the previous call stored, never the one this call's last run stores"""
    import torch
    srcs = [ctx.encode_lossy(O.synth_clip(300 * 1024 + 13 * k, 2, clip_id=400 + k), 44100, 2, 0.35 + 0.2 * k) for k in range(3)]
    n = 600
    blobs = [srcs[i % 3] for i in range(n)]
    decs = [flo_amd.StreamingDecoder(ctx) for _ in range(n)]
    rng = np.random.default_rng(5)
    pos = [0] * n
    outs = [[] for _ in range(n)]
    while any(d.state() != flo_amd.DecoderState.Finished for d in decs):
        for i in range(n):
            step = int(rng.integers(43, 61)) * (len(blobs[i]) // 300)   # 43 - 60 frames' worth of bytes
            decs[i].feed(blobs[i][pos[i]:pos[i] + step])
            pos[i] += step
        r = flo_amd.decode_streams(decs)
        host = r.out.cpu().numpy()
        torch.cuda.synchronize()
        for i in range(n):
            outs[i].append(host[int(r.offsets[i]):int(r.offsets[i + 1])])
    want = [ctx.decode(b) for b in srcs]
    for i in range(n):
        assert np.array_equal(_bits(np.concatenate(outs[i])), _bits(want[i % 3])), i


def test_decode_streams_rejects_a_closed_decoder(ctx):
    d = flo_amd.StreamingDecoder(ctx)
    d.close()
    with pytest.raises(flo_amd.FloError):
        flo_amd.decode_streams([d])
