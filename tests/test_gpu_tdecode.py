"""The transform decoder on the device (lossy_decode_kernel, all four instantiations) against the exact f64 reference of
the operation (tests/tdec_ref.py), in units of the oracle's own f32 error on the same file - not against the oracle at a
flat 2e-6.

Tight class (hand-made files over every rate's band edges, per-band scale words, zero words, wide words, frame counts
around the run lengths, frames with fewer channels than the header, sparse bytes around the kernel's thresholds; encoder-
made files at three qualities, rates and levels; the reference's example files): per file the device's worst
max|err| / block scale is at most 2 x the oracle's and its relative RMS error at most 1.5 x the oracle's, both measured
here from O.decode on the CPU. Blocks that are silent in the reference hold nothing but zeros. Then every other path -
corpus windows, decode_frame_at, the streaming decoder under three feeds, Batch.decode_to, the fused compare - equals
flo_decode bit for bit. Edge class (words 1 - 600 and 62000 - 65535): the oracle's pattern of NaN and inf, finite values
within the oracle-relative bound of the damage tests. All calls go through the C ABI. Needs an MI355X.

Measured (MI355X): oracle worst 2.0e-7 ... 5.0e-7 per file, RMS 0.9e-7 ... 1.6e-7; device worst 1.8e-7 ... 4.4e-7 (at most
1.48 x the oracle's on a file), RMS 0.9e-7 ... 1.4e-7 (at most 1.02 x). Before the kernel read all four window entries
of a row (it mirrored the first half of an asymmetric f32 table) words_1ch_11025_dense stood at 2.06 x, and before a run
looked for an absent channel's older overlap every absent_* file failed by the size of the signal."""
import numpy as np
import pytest

import fidelity_ref as M
import flofile
import signals
import tdec_ref as T
from gpu_util import ctx  # noqa: F401
from oracle import oracle as O

import flo_amd

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _frame_end(flo, k):
    """the byte behind frame k of the file"""
    f = flofile.parse(flo)
    return 70 + f.toc_size + f.toc[k][1] + f.toc[k][2]


def _stream(ctx, flo, cuts):
    """the file fed to one StreamingDecoder up to each byte position of `cuts` in turn, decode_streams after each feed"""
    d = flo_amd.StreamingDecoder(ctx)
    parts, at = [], 0
    for end in list(cuts) + [len(flo)]:
        if end <= at:
            continue
        d.feed(flo[at:end])
        at = end
        r = flo_amd.decode_streams([d])
        assert int(r.status[0]) == 0, r.errors
        parts.append(r.out.cpu().numpy()[int(r.offsets[0]):int(r.offsets[1])].copy())
    if d.state() == flo_amd.DecoderState.Ready:
        flo_amd.decode_streams([d])
    assert d.state() == flo_amd.DecoderState.Finished
    d.close()
    return np.concatenate(parts) if parts else np.zeros(0, np.float32)


def every_path(ctx, name, flo, want):
    """corpus windows, decode_frame_at and the streaming decoder give flo_decode's samples bit for bit"""
    f = flofile.parse(flo)
    ch, nf = f.channels, len(f.frames)
    corpus = flo_amd.Corpus([flo], ctx)
    n = int(corpus.lengths[0])
    assert n * ch == want.size
    whole = corpus.decode_windows(np.zeros(1, np.uint32), np.zeros(1, np.uint64), max(n, 1)).cpu().numpy().reshape(-1)
    assert np.array_equal(_bits(whole[:want.size]), _bits(want)), (name, "the window over the whole file")
    # windows that start and end inside a block, on both sides of the run boundaries (runs are 8 or 16 blocks)
    L = 2500
    starts = sorted({s for s in (0, 517, 7 * 1024 + 512, 8 * 1024 - 1500, 8 * 1024 - 5, 8 * 1024 + 300, 9 * 1024 + 1, 15 * 1024 + 900,
                                 16 * 1024 - 1500, 16 * 1024 + 7, 17 * 1024 - 3, 32 * 1024 - 700, max(n - 1300, 0)) if s < max(n, 1)})
    got = corpus.decode_windows(np.zeros(len(starts), np.uint32), np.array(starts, np.uint64), L).cpu().numpy()
    corpus.sync()
    corpus.close()
    for k, s in enumerate(starts):
        w = np.zeros(L * ch, np.float32)
        seg = want[s * ch:(s + L) * ch]
        w[:seg.size] = seg
        assert np.array_equal(_bits(got[k].reshape(-1)), _bits(w)), (name, "window at", s)
    for i in range(1, nf):
        x = ctx.decode_frame_at(flo, i)
        assert np.array_equal(_bits(x), _bits(want[(i - 1) * 1024 * ch:i * 1024 * ch])), (name, "decode_frame_at", i)
    assert ctx.decode_frame_at(flo, 0).size == 1024 * ch
    # the streaming decoder: the file whole; in pieces of 777 bytes, which cut frames in two; and cut behind frames 8 and 16
    # and in the middle of frame 17, so that a call ends on a run boundary and the next starts from the stored overlap
    feeds = {"whole": [], "777 bytes": list(range(777, len(flo), 777)),
             "run boundary": [_frame_end(flo, k) for k in (8, 16) if k < nf] + ([_frame_end(flo, 17) - 9] if nf > 17 else [])}
    for tag, cuts in feeds.items():
        assert np.array_equal(_bits(_stream(ctx, flo, cuts)), _bits(want)), (name, "streaming decoder fed", tag)


@pytest.fixture(scope="module")
def encoded(ctx):
    return dict(T.encoder_cases(ctx.encode_lossy))


@pytest.mark.parametrize("name", T.HAND_MADE)
def test_hand_made_files_against_the_f64_reference_on_every_path(ctx, name):
    flo = T.hand_made(name)
    got = ctx.decode(flo)
    T.assert_tight(name, flo, got)
    every_path(ctx, name, flo, got)


@pytest.mark.parametrize("name", T.encoder_names())
def test_encoder_made_files_against_the_f64_reference_on_every_path(ctx, encoded, name):
    flo = encoded[name]
    got = ctx.decode(flo)
    T.assert_tight(name, flo, got)
    every_path(ctx, name, flo, got)


@pytest.mark.parametrize("name,flo", T.edge_cases(), ids=[n for n, _ in T.edge_cases()])
def test_edge_words_follow_the_oracle(ctx, name, flo):
    want = O.decode(flo)[0]
    got = ctx.decode(flo)
    assert got.shape == want.shape
    with np.errstate(invalid="ignore", over="ignore"):
        assert np.array_equal(np.isnan(want), np.isnan(got)) and np.array_equal(np.isinf(want), np.isinf(got)), name
        fin = np.isfinite(want) & np.isfinite(got)
        if fin.any():
            assert np.array_equal(np.signbit(want[np.isinf(want)]), np.signbit(got[np.isinf(got)]))
            diff = np.abs(want[fin].astype(np.float64) - got[fin].astype(np.float64))
            peak = float(np.abs(want[fin]).max())
            ref, scale = T.decode(flo)
            dm, om = T.measure(got, ref, scale), T.measure(want, ref, scale)
            print(f"{name}: peak {peak:.3e}, device - oracle at most {float(diff.max()):.3e}; against f64: device worst {dm['worst']:.2e} "
                  f"rms {dm['rms']:.2e}, oracle worst {om['worst']:.2e} rms {om['rms']:.2e}; device subnormals "
                  f"{int(((got != 0) & (np.abs(got) < 1.1754944e-38)).sum())}, oracle subnormals {int(((want != 0) & (np.abs(want) < 1.1754944e-38)).sum())}")
            assert float(diff.max()) <= 2e-6 * max(1.0, peak), name


def test_files_of_different_formats_take_turns(ctx):
    """One launch holds one format (a Corpus and a decode_streams call refuse files that differ in rate or channel count),
    so each file's band map is chosen per call: calls that alternate between rates and channel counts, through one context
    and one streaming decoder, give what each file gives alone."""
    names = ["band_edges_8000", "band_edges_384000", "words_3ch_128000_dense", "band_edges_44100", "words_8ch_16000_sparse",
             "absent_6ch_0", "band_edges_11025", "words_1ch_11025_sparse"]
    files = [T.hand_made(n) for n in names]
    alone = [ctx.decode(f) for f in files]
    d = flo_amd.StreamingDecoder(ctx)
    for rnd in range(2):
        for n, f, a in zip(names, files, alone):
            assert np.array_equal(_bits(ctx.decode(f)), _bits(a)), n
            d.reset()
            d.feed(f)
            r = flo_amd.decode_streams([d])
            assert int(r.status[0]) == 0 and np.array_equal(_bits(r.out.cpu().numpy()), _bits(a)), n
            c = flo_amd.Corpus([f, f], ctx)
            w = c.decode_windows(np.array([1, 0], np.uint32), np.array([1024 + 7, 0], np.uint64), 3000).cpu().numpy()
            c.sync()
            c.close()
            ch = flofile.parse(f).channels
            assert np.array_equal(_bits(w[1].reshape(-1)), _bits(a[:3000 * ch])), n
            assert np.array_equal(_bits(w[0].reshape(-1)), _bits(a[(1024 + 7) * ch:(1024 + 7 + 3000) * ch])), n
    d.close()
    a, b = flo_amd.StreamingDecoder(ctx), flo_amd.StreamingDecoder(ctx)
    a.feed(files[0])
    b.feed(files[1])
    with pytest.raises(flo_amd.FloError, match="differ in sample rate"):
        flo_amd.decode_streams([a, b])
    a.close()
    b.close()
    with pytest.raises(flo_amd.FloError):
        flo_amd.Corpus([files[0], files[1]], ctx)


@pytest.mark.parametrize("ch,sr", [(1, 8000), (2, 48000), (3, 22050), (6, 96000), (8, 192000)])
def test_batch_decode_equals_the_files_decode_beyond_stereo(ctx, ch, sr):
    import torch
    lens = [5 * 1024 + 300, 17 * 1024 + 1, 700]
    clips = [signals.music_like(sr, n, ch, seed=ch * 10 + k).astype(np.float32).reshape(-1) for k, n in enumerate(lens)]
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [c.size for c in clips], sr, ch, 0.55)
    try:
        for i, c in enumerate(clips):
            b.upload(i, c)
        b.encode(0)
        b.sync()
        hops = [(n + 1024 + 1023) // 1024 for n in lens]
        total = sum((h - 1) * 1024 * ch for h in hops)
        out = torch.full((total + 8,), float("nan"), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        offs = b.decode_to(out.data_ptr(), total)
        host = out.cpu().numpy()
        assert np.isnan(host[total:]).all()
        for i, h in enumerate(hops):
            flo = b.fetch(i)
            want = ctx.decode(flo)
            assert want.size == (h - 1) * 1024 * ch
            assert np.array_equal(_bits(host[offs[i]:offs[i] + want.size]), _bits(want)), (ch, sr, i)
            T.assert_tight(f"batch_{ch}ch_{sr}_clip{i}", flo, want)
    finally:
        b.close()


@pytest.mark.parametrize("name", ["absent_2ch_0", "absent_6ch_0", "band_edges_8000"])
def test_fused_compare_sees_what_decode_returns(ctx, name):
    """flo_compare decodes in the kernel's fourth instantiation and never stores PCM: against the f64 reference rounded to
    f32 as the source, every block's error energy is the model's (tests/fidelity_ref.py) of (source, flo_decode's PCM),
    bit for bit - a few 1e-14 of the signal's energy, where one wrong sample would show"""
    flo = T.hand_made(name)
    ch = flofile.parse(flo).channels
    ref, _ = T.decode(flo)
    source = ref.astype(np.float32)
    rep = ctx.compare(source, flo, blocks=True)
    want, wb = M.fidelity(source, ctx.decode(flo), ch)
    M.assert_matches(rep, want, wb, tag=name)
    assert np.all(rep["snr_db"] > 120.0), rep["snr_db"]
