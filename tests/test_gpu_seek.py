"""Seeking on the device: decode_frame_at against flo_decode and the oracle, and the corpus window decode
(flo_corpus_decode_windows) against slices of flo_decode / flo_batch_decode, bit for bit. Needs an MI355X."""
import glob
import os
import struct

import numpy as np
import pytest

from conftest import EXAMPLES, example_bytes
from fixtures_util import LOSSLESS_EXAMPLES, LOSSY_EXAMPLES, dequantise
from gpu_util import ctx  # noqa: F401
from oracle import oracle as O

import flo_amd

pytestmark = pytest.mark.gpu

LOSSY_TOL = 2e-6
FILES = sorted(glob.glob(os.path.join(EXAMPLES, "*.flo")))


def _frames(b):
    """(type, samples, blob bytes of the first channel wrapper) of every frame the reader accepts"""
    toc_size, data_size = struct.unpack_from("<QQ", b, 38)
    n = struct.unpack_from("<I", b, 70)[0] if toc_size >= 4 else 0
    ds = 74 + 20 * n if toc_size >= 4 else 70
    out = []
    for e in flo_amd.get_toc(b):
        fs = ds + e.byte_offset
        if fs >= ds + data_size:
            break
        t, ns, _ = struct.unpack_from("<BIB", b, fs)
        cl = struct.unpack_from("<I", b, fs + 6)[0]
        out.append((t, ns, b[fs + 10: fs + 10 + cl]))
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_decode_frame_at_every_frame(ctx, path):
    b = open(path, "rb").read()
    info = flo_amd.probe_container(b)
    ch, sr = info.channels, info.sample_rate
    fr = _frames(b)
    full = ctx.decode(b)
    if not info.is_transform:
        ints = O.decode_lossless_i32(b)[0].reshape(-1)
        at = 0
        for i, (_, ns, _) in enumerate(fr):
            x = ctx.decode_frame_at(b, i)
            assert x.size == ns * ch
            assert np.array_equal(_bits(x), _bits(full[at * ch:(at + ns) * ch])), (path, i)
            want = ints[at * ch:(at + ns) * ch].astype(np.float32) * np.float32(1.0 / 32767.0)
            assert np.array_equal(_bits(x), _bits(want)), (path, i)
            at += ns
    else:
        ref = O.decode(b)[0].reshape(-1)
        band = O.psy_tables(sr)[1]
        for i in range(len(fr)):
            x = ctx.decode_frame_at(b, i)
            assert x.size == 1024 * ch
            if i >= 1:
                assert np.array_equal(_bits(x), _bits(full[(i - 1) * 1024 * ch:i * 1024 * ch])), (path, i)
                assert float(np.abs(x - ref[(i - 1) * 1024 * ch:i * 1024 * ch]).max()) <= LOSSY_TOL, (path, i)
            else:
                # frame 0: first half of its own inverse transform, nothing to overlap with (restated from the blob)
                blob = fr[0][2]
                nb = blob[1]
                words = np.frombuffer(blob, "<u2", count=25 * nb, offset=2).reshape(nb, 25)
                pos = 2 + 50 * nb
                want = np.zeros((1024, ch), np.float64)
                for c in range(nb):
                    ln = struct.unpack_from("<I", blob, pos)[0]
                    q = np.asarray(O.deserialize_sparse(blob[pos + 4:pos + 4 + ln]), np.float32)
                    pos += 4 + ln
                    spec = dequantise(q, words[c], band).astype(np.float32)
                    want[:, c] = np.asarray(O.mdct_inverse(spec))[:1024]
                assert float(np.abs(x.reshape(1024, ch) - want).max()) <= LOSSY_TOL, path
    with pytest.raises(flo_amd.FloError, match=f"Frame index {len(fr)} out of bounds \\(total frames: {len(fr)}\\)"):
        ctx.decode_frame_at(b, len(fr))


def _window_ref(dec, ch, s, L):
    want = np.zeros(L * ch, np.float32)
    seg = dec[s * ch:(s + L) * ch]
    want[:seg.size] = seg
    return want


def _check_corpus(ctx, files, windows_by_len, seed=0):
    import torch
    corpus = flo_amd.Corpus(files, ctx)
    decs = [ctx.decode(f) for f in files]
    ch = corpus.channels
    for i, d in enumerate(decs):
        assert d.size == int(corpus.lengths[i]) * ch
    for L, wins in windows_by_len.items():
        fi = np.array([w[0] for w in wins], np.uint32)
        st = np.array([w[1] for w in wins], np.uint64)
        got = corpus.decode_windows(fi, st, L).cpu().numpy()
        assert got.shape == (len(wins), L, ch)
        for k, (f, s) in enumerate(wins):
            assert np.array_equal(_bits(got[k].reshape(-1)), _bits(_window_ref(decs[f], ch, s, L))), (L, f, s)
    corpus.sync()
    corpus.close()


def _windows(rng, lengths, L, n_random=24):
    out = []
    for f, n in enumerate(lengths):
        n = int(n)
        starts = {0, max(n - 1, 0), max(n - 5, 0), n, n + 7, (n // 1024) * 1024, max((n // 1024) * 1024 - 1, 0),
                  44100 - 1, 44100, 44100 - L // 2 if L < 44100 else 0, 16 * 1024 - 3, 17 * 1024 + 5}
        starts |= set(int(x) for x in rng.integers(0, max(n, 1) + 100, n_random))
        out += [(f, s) for s in sorted(starts)]
    out += out[:5]   # duplicates
    return out


@pytest.mark.parametrize("ch,sr", [(1, 44100), (2, 44100), (6, 48000), (2, 96000)])
def test_corpus_windows_mixed(ctx, ch, sr):
    rng = np.random.default_rng(ch * 1000 + sr)
    files = []
    for k, secs in enumerate([2.3, 3.0, 0.4, 5.71]):
        n = int(secs * sr) + k * 37
        pcm = O.synth_clip(n, ch, clip_id=100 + k)
        files.append(ctx.encode_lossless(pcm, sr, ch, 16, 5))
        if ch <= 8:
            files.append(ctx.encode_lossy(pcm, sr, ch, 0.55 if k % 2 else 0.3))
    if ch == 2 and sr == 44100:   # reference-made files, with mid/side frames among them
        for name in LOSSLESS_EXAMPLES + [n for n, _, _ in LOSSY_EXAMPLES]:
            b = example_bytes(name + ".flo")
            i = flo_amd.probe_container(b)
            if i.channels == 2 and i.sample_rate == 44100:
                files.append(b)
    corpus = flo_amd.Corpus(files, ctx)
    lengths = corpus.lengths
    corpus.close()
    wins = {}
    for L in (1, 1024, sr, 9 * sr):
        wins[L] = _windows(rng, lengths, L)
    _check_corpus(ctx, files, wins)


def test_corpus_back_to_back_calls_and_stream_order(ctx):
    import torch
    sr, ch = 44100, 2
    files = []
    for k in range(4):
        pcm = O.synth_clip(int(3.5 * sr) + k * 101, ch, clip_id=7 + k)
        files.append(ctx.encode_lossless(pcm, sr, ch, 16, 5) if k % 2 else ctx.encode_lossy(pcm, sr, ch, 0.55))
    decs = [ctx.decode(f) for f in files]
    corpus = flo_amd.Corpus(files, ctx)
    rng = np.random.default_rng(5)
    L = 5000
    calls = []
    outs = []
    for i in range(64):
        n = int(rng.integers(1, 40))
        fi = rng.integers(0, len(files), n).astype(np.uint32)
        st = np.array([int(rng.integers(0, corpus.lengths[f] + 10)) for f in fi], np.uint64)
        calls.append((fi, st))
        outs.append(corpus.decode_windows(fi, st, L))
    corpus.sync()
    for (fi, st), o in zip(calls, outs):
        g = o.cpu().numpy()
        for k in range(len(fi)):
            assert np.array_equal(_bits(g[k].reshape(-1)), _bits(_window_ref(decs[fi[k]], ch, int(st[k]), L)))
    # ordering on the current stream with no explicit synchronisation: a torch op behind the decode sees its values
    fi = np.zeros(8, np.uint32)
    st = np.arange(8, dtype=np.uint64) * 1000
    out = torch.full((8, L, ch), 7.0, device="cuda")
    corpus.decode_windows(fi, st, L, out=out)
    s = (out * 2.0).sum().item()
    want = sum(float(_window_ref(decs[0], ch, int(x), L).astype(np.float64).sum()) for x in st) * 2.0
    assert abs(s - want) <= 1e-3 * max(1.0, abs(want))
    corpus.close()


def test_corpus_errors(ctx):
    a = ctx.encode_lossless(O.synth_clip(50000, 2, clip_id=1), 44100, 2, 16, 5)
    b = ctx.encode_lossless(O.synth_clip(50000, 2, clip_id=2), 48000, 2, 16, 5)
    c = ctx.encode_lossless(O.synth_clip(50000, 1, clip_id=3), 44100, 1, 16, 5)
    for pair in ((a, b), (a, c)):
        with pytest.raises(flo_amd.FloError):
            flo_amd.Corpus(list(pair), ctx)
    with pytest.raises(flo_amd.FloError, match="bad magic"):
        flo_amd.Corpus([a, b"XXXX" + a[4:]], ctx)
    # a damaged lossy blob: the block-size byte of frame 5 made nonzero
    lossy = bytearray(ctx.encode_lossy(O.synth_clip(10 * 44100, 2, clip_id=4), 44100, 2, 0.55))
    toc = flo_amd.get_toc(bytes(lossy))
    ds = 74 + 20 * len(toc)
    lossy[ds + toc[5].byte_offset + 10] = 3
    lossy = bytes(lossy)
    with pytest.raises(flo_amd.FloError) as e:
        ctx.decode(lossy)
    corpus = flo_amd.Corpus([a, lossy], ctx)
    corpus.decode_windows(np.array([1, 0], np.uint32), np.array([3 * 1024, 0], np.uint64), 44100)
    with pytest.raises(flo_amd.FloError) as e2:
        corpus.sync()
    assert str(e2.value) == str(e.value)
    corpus.sync()   # the error word was cleared
    corpus.close()


@pytest.mark.parametrize("mode", [flo_amd.MODE_LOSSY, flo_amd.MODE_LOSSLESS])
def test_corpus_full_size(ctx, mode):
    import torch
    sr, ch, n_files = 44100, 2, 64
    n = 180 * sr * ch
    bt = flo_amd.Batch(ctx, mode, [n] * n_files, sr, ch, 0.55 if mode == flo_amd.MODE_LOSSY else 5)
    bt.fill_synthetic(seed=11)
    bt.encode()
    bt.sync()
    files = [bt.fetch(i) for i in range(n_files)]
    total = n_files * (n + 2048 * ch)
    ref = torch.empty(total, dtype=torch.float32, device="cuda")
    offs = bt.decode_to(ref.data_ptr(), total)
    bt.close()
    corpus = flo_amd.Corpus(files, ctx)
    del files
    rng = np.random.default_rng(mode)
    fi = rng.integers(0, n_files, 1024).astype(np.uint32)
    st = np.array([int(rng.integers(0, corpus.lengths[f] - sr // 2)) for f in fi], np.uint64)
    got = corpus.decode_windows(fi, st, sr)
    lens = torch.tensor(corpus.lengths.astype(np.int64), device="cuda")
    base = torch.tensor(np.array(offs, np.int64), device="cuda")[torch.tensor(fi.astype(np.int64), device="cuda")]
    t = torch.tensor(st.astype(np.int64), device="cuda")[:, None] + torch.arange(sr, device="cuda")[None, :]
    valid = t < lens[torch.tensor(fi.astype(np.int64), device="cuda")][:, None]
    idx = (base[:, None, None] + t[:, :, None] * ch + torch.arange(ch, device="cuda")[None, None, :]).clamp(max=total - 1)
    want = torch.where(valid[:, :, None], ref[idx], torch.zeros((), device="cuda"))
    assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))
    corpus.close()
