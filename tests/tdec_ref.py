"""The exact reference of the transform (lossy) decoder, in float64 NumPy, and the files every decode path is held to it on.

A plain restatement of decoder.rs:29-131 plus mdct.rs:231-290, 437-468 as oracle/lossy.c:652-749 cites them:

    sf[b]   = 2 ** ((word[b] - 32768) / 256) for word[b] > 0; a band whose word is 0 gives zero coefficients
    coef[k] = q[k] / sf[band[k]],  band[k] = freq_to_bark_band((k + 0.5) * sr / 2048)
    y[n]    = (2 / 1024) * w[n] * sum_k coef[k] * cos(pi / 1024 * (n + 0.5 + 512) * (k + 0.5)),  n < 2048
    block h of channel c = y_h[:1024] + overlap_c, then overlap_c = y_h[1024:]
    a channel the frame does not carry gives a zero block and leaves its overlap unchanged
    the first frame's block is dropped (lib.rs:338-341); the output is interleaved

w is the oracle's f32 Vorbis window promoted to float64 and band[] the oracle's table (both are data; test_tdec_ref_cpu.py
checks band[] against a restatement of its own): the arithmetic is what is being checked. The integers of a frame come from
O.deserialize_sparse, whose agreement with the device has tests of its own.

Errors are normalised per (block, channel) by the block's SCALE = max(max |y_h[:1024]|, max |previous overlap|), not by the
block's own peak: two large halves that cancel would otherwise make a tiny denominator. A block of scale 0 is exactly zero (of either sign: a
few of the oracle's own zeros in such a block are -0.0, what its FFT makes of a spectrum of +0.0 and -0.0)."""
import functools
import struct

import numpy as np

import flofile
from oracle import oracle as O

RATES = [8000, 11025, 16000, 22050, 44100, 48000, 96000, 128000, 176400, 192000, 384000]
BARK_EDGES = np.array([0, 100, 200, 300, 400, 510, 630, 770, 920, 1080, 1270, 1480, 1720, 2000, 2320, 2700, 3150, 3700, 4400, 5300,
                       6400, 7700, 9500, 12000, 15500, 20500], np.float32)


# ------------------------------------------------------------------------------------------------------- the reference
@functools.lru_cache(maxsize=1)
def _basis():
    """(2 / 1024) * w[n] * cos(pi / 1024 * (n + 0.5 + 512) * (k + 0.5)) as [2048][1024] float64. The angle is
    (2 n + 1025)(2 k + 1) * pi / 4096: the integer product is reduced mod 8192 (a whole turn) before it meets pi."""
    n = np.arange(2048, dtype=np.int64)[:, None]
    k = np.arange(1024, dtype=np.int64)[None, :]
    turn = ((2 * n + 1025) * (2 * k + 1)) % 8192
    w = O.window(2048).astype(np.float64)[:, None]
    return (2.0 / 1024.0) * w * np.cos(turn.astype(np.float64) * (np.pi / 4096.0))


def band_map(sr):
    """freq_to_bark_band of every bin with the f32 frequency arithmetic of oracle/lossy.c:713 (independent of O.psy_tables)"""
    freq = (np.arange(1024, dtype=np.float32) + np.float32(0.5)) * (np.float32(sr) / np.float32(2048.0))
    assert freq.dtype == np.float32
    return np.minimum(np.searchsorted(BARK_EDGES[1:], freq, side="right"), 24).astype(np.uint8)


def describe(flo):
    """a transform file -> (sample_rate, channels, frames); frames[f] = [(25 words, 1024 integers) per carried channel]"""
    f = flofile.parse(flo)
    assert f.is_lossy
    frames = []
    for fr in f.frames:
        assert fr.frame_type == 253
        blob = fr.channels[0].raw
        assert len(blob) >= 2 and blob[0] == 0
        nch = blob[1]
        assert nch <= f.channels
        words = np.frombuffer(blob, "<u2", count=25 * nch, offset=2).reshape(nch, 25)
        pos = 2 + 50 * nch
        chans = []
        for c in range(nch):
            ln = struct.unpack_from("<I", blob, pos)[0]
            assert pos + 4 + ln <= len(blob)
            chans.append((words[c], O.deserialize_sparse(blob[pos + 4:pos + 4 + ln])))
            pos += 4 + ln
        frames.append(chans)
    return f.sample_rate, f.channels, frames


def decode(desc):
    """desc = a file's bytes or (sample_rate, channels, frames) -> (pcm float64 interleaved [(F - 1) * 1024 * channels],
    scale float64 [F - 1][channels])"""
    sr, ch, frames = describe(desc) if isinstance(desc, (bytes, bytearray)) else desc
    band = O.psy_tables(sr)[1].astype(np.int64)
    nf = len(frames)
    carried = [(f, c) for f in range(nf) for c in range(len(frames[f]))]
    coef = np.zeros((len(carried), 1024), np.float64)
    for i, (f, c) in enumerate(carried):
        words, q = frames[f][c]
        w = np.asarray(words, np.float64)
        sf = np.where(w > 0, np.exp2((w - 32768.0) / 256.0), 1.0)
        coef[i] = np.where(w[band] > 0, np.asarray(q, np.float64) / sf[band], 0.0)
    y = coef @ _basis().T if carried else np.zeros((0, 2048))
    nb = max(nf - 1, 0)
    pcm = np.zeros((nb, 1024, ch), np.float64)
    scale = np.zeros((nb, ch), np.float64)
    overlap = np.zeros((ch, 1024), np.float64)
    where = {fc: i for i, fc in enumerate(carried)}
    for f in range(nf):
        for c in range(ch):
            i = where.get((f, c))
            if i is None:
                continue                        # a zero block; the overlap stays
            if f > 0:
                pcm[f - 1, :, c] = y[i, :1024] + overlap[c]
                scale[f - 1, c] = max(np.abs(y[i, :1024]).max(), np.abs(overlap[c]).max())
            overlap[c] = y[i, 1024:]
    return pcm.reshape(-1), scale


def measure(got, ref, scale):
    """got: decoded f32 interleaved; (ref, scale) = decode(...) -> dict(worst = max over (block, channel) of
    max|err| / scale, rms = relative RMS error, at = (block, channel, position) of the worst, zero_ok = every block of
    scale 0 holds nothing but zeros, finite)"""
    nb, ch = scale.shape
    got = np.asarray(got)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    g = got.astype(np.float64).reshape(nb, 1024, ch)
    r = ref.reshape(nb, 1024, ch)
    finite = bool(np.isfinite(g).all())
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(g - r)
        emax = err.max(axis=1) if nb else np.zeros((0, ch))
        live = scale > 0
        ratio = np.where(live, emax / np.where(live, scale, 1.0), 0.0)
        silent = (g == 0.0).all(axis=1) | live if nb else np.ones((0, ch), bool)
        zero_ok = bool(silent.all())
        zero_at = None if zero_ok else tuple(int(x) for x in np.argwhere(~silent)[0])
        if nb and np.isnan(ratio).any():
            b, c = (int(x) for x in np.argwhere(np.isnan(ratio))[0])
        elif nb:
            b, c = (int(x) for x in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
        else:
            b = c = 0
        worst = float(ratio[b, c]) if nb else 0.0
        pos = int(np.argmax(np.nan_to_num(err[b, :, c], nan=np.inf))) if nb else 0
        den = float((r ** 2).sum())
        rms = float(np.sqrt((err ** 2).sum() / den)) if den > 0 else float(np.sqrt((err ** 2).sum()))
    return dict(worst=worst, rms=rms, at=(b, c, pos), zero_ok=zero_ok, zero_at=zero_at, finite=finite, blocks=int(live.sum()),
                got=float(g[b, pos, c]) if nb else 0.0, want=float(r[b, pos, c]) if nb else 0.0, scale=float(scale[b, c]) if nb else 0.0)


# ------------------------------------------------------------------------------------------------------------ the cases
def sparse_blob(records):
    """[(zero_run, [values...]) ...] -> sparse bytes (encoder.rs:284-314 layout: varint zeros, count, i16 values)"""
    out = bytearray()
    for z, vals in records:
        out += flofile.encode_varint(z) + bytes([len(vals)]) + np.asarray(vals, dtype="<i2").tobytes()
    return bytes(out)


def _file(sr, ch, frames):
    """frames[f] = [(words, integers[1024]) per carried channel] -> the file (canonical sparse bytes)"""
    return flofile.build_transform(sr, ch, [[(w, O.serialize_sparse(q)) for w, q in chans] for chans in frames])


def _ints(rng, density, lim=32767, extremes=False):
    q = rng.integers(-lim, lim + 1, 1024)
    q[rng.random(1024) >= density] = 0
    if extremes:
        at = rng.choice(1024, 6, replace=False)
        q[at] = [32767, -32768, -32767, 32767, -32768, 1]
    return q.astype(np.int16)


def _words(rng, lo=28900, hi=45100):
    return rng.integers(lo, hi + 1, 25).astype(np.int64)


def band_edge_file(sr):
    """For every band the rate has: a frame with one integer at the band's first bin (channel 0) and one at its last bin
    (channel 1), then an all-zero frame. Adjacent bands' factors differ by 16 (256 * 4 in the word), the other way round in
    channel 1: a bin read with a neighbour's factor is wrong by 16 x. Bands the rate lacks carry words 0 and 65535."""
    band = O.psy_tables(sr)[1]
    present = sorted(set(int(b) for b in band))
    words = []
    for flip in (0, 1):
        w = np.array([32768 + 256 * (3 + 4 * ((b + flip) % 2)) for b in range(25)], np.int64)
        for b in range(25):
            if b not in present:
                w[b] = 65535 if (b + flip) % 2 else 0
        words.append(w)
    zero = np.zeros(1024, np.int16)
    frames = [[(words[0], zero), (words[1], zero)]]
    for i, b in enumerate(present):
        ks = np.flatnonzero(band == b)
        q0, q1 = zero.copy(), zero.copy()
        q0[ks[0]] = 1000 if i % 2 else -1000
        q1[ks[-1]] = -1000 if i % 2 else 1000
        frames += [[(words[0], q0), (words[1], q1)], [(words[0], zero), (words[1], zero)]]
    return _file(sr, 2, frames)


def _loud(f):
    """frames directly before and after a run boundary (runs are 8 or 16 blocks) and on one"""
    return f % 16 in (7, 9) or (f % 16 == 0 and f > 0)


def frame_count_file(n, seed):
    rng = np.random.default_rng(seed)
    frames = []
    for f in range(n):
        w = _words(rng, 33000, 36000) - (256 * 6 if _loud(f) else 0)
        frames.append([(w + 40 * c, _ints(rng, 0.1, 3000)) for c in range(2)])
    return _file(44100, 2, frames)


ABSENT = {   # header channels -> per-frame channel counts: drops and returns inside a run and across frames 7-10, 15-18
    2: [[2, 1, 2, 1, 2, 2, 2, 1, 1, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2],
        [2, 2, 2, 2, 2, 2, 2, 2, 1, 2, 2, 0, 2, 2, 2, 2, 1, 2, 1, 2],
        [1, 2, 1, 1, 0, 2, 2, 1, 2, 1, 2, 2, 2, 2, 2, 1, 2, 1, 2, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 2, 2]],
    3: [[3, 3, 0, 1, 3, 3, 2, 1, 1, 3, 2, 3, 3, 3, 3, 2, 1, 3, 3, 3],
        [0, 3, 2, 3, 1, 1, 1, 3, 2, 2, 3, 3, 3, 3, 3, 3, 0, 0, 3, 1, 3]],
    6: [[6, 5, 6, 3, 6, 6, 6, 2, 4, 6, 6, 6, 1, 6, 6, 5, 0, 4, 6, 6],
        [6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 3, 3, 6]],
}


def absent_file(ch, counts, seed):
    rng = np.random.default_rng(seed)
    frames = []
    for f, n in enumerate(counts):
        frames.append([(_words(rng, 33000, 35000), _ints(rng, 0.1, 3000)) for _ in range(n)])
    return _file(48000 if ch == 3 else 44100, ch, frames)


def blob_size_file(kind, seed):
    """sparse bytes around the kernel's thresholds, every band with a word of its own: "doubling" - 128 records and under
    1024 bytes; "records" - 129 records; "bytes" - 1100 - 2000 bytes; "in_place" - more than 2304 bytes (non-canonical:
    five-byte varints, empty records and bytes behind position 1023)"""
    rng = np.random.default_rng(seed)
    frames = []
    for f in range(4):
        chans = []
        for c in range(2):
            if kind in ("doubling", "records"):
                n_rec = 128 if kind == "doubling" else 129
                recs = [(int(rng.integers(1, 4)), [int(v) for v in rng.integers(-3000, 3000, int(rng.integers(1, 3)))]) for _ in range(n_rec)]
                blob = sparse_blob(recs)
                assert len(blob) <= 1024 and sum(z + len(v) for z, v in recs) <= 1024
            elif kind == "bytes":
                recs = [(int(rng.integers(0, 3)), [int(v) for v in rng.integers(-3000, 3000, 100 + 20 * c + f)]) for _ in range(6)]
                blob = sparse_blob(recs)
                assert 1024 < len(blob) <= 2304
            else:
                blob = b""
                for r in range(40):
                    blob += b"\x80\x80\x80\x80\x00" + bytes([0])                      # an empty record behind a five-byte zero
                    blob += sparse_blob([(int(rng.integers(0, 3)), [int(v) for v in rng.integers(-3000, 3000, 20)])])
                blob += sparse_blob([(1024, [7] * 200)]) + bytes(rng.integers(0, 256, 500, dtype=np.uint8))   # never reached
                assert len(blob) > 2304
            chans.append((_words(rng, 33000, 36000), blob))
        frames.append(chans)
    return flofile.build_transform(44100, 2, frames)


def words_file(ch, sr, density):
    """every band of every channel of every frame with a word of its own, drawn across what the encoder can emit
    (floor(256 log2(30000 / band_max)) + 32768 for band maxima of 1e-10 ... 1e9), integers up to the i16 extremes"""
    rng = np.random.default_rng(1000 + 10 * ch + int(density * 10))
    return _file(sr, ch, [[(_words(rng), _ints(rng, density, extremes=True)) for _ in range(ch)] for _ in range(5)])


def level_file(centre):
    rng = np.random.default_rng(centre)
    return _file(22050, 2, [[(_words(rng, centre - 300, centre + 300), _ints(rng, 0.5)) for _ in range(2)] for _ in range(5)])


def zero_words_file():
    rng = np.random.default_rng(77)
    frames = []
    for f in range(5):
        chans = []
        for c in range(2):
            w = _words(rng, 33000, 36000)
            w[rng.random(25) < 0.4] = 0                       # a silenced band under non-zero integers
            if f == 3 and c == 1:
                w[:] = 0
            chans.append((w, _ints(rng, 1.0, 3000)))
        frames.append(chans)
    return _file(16000, 2, frames)


def wide_words_file(sr):
    """words 20000 ... 60000 (factors 2^-50 ... 2^106) under integers of at most 3: finite in the oracle"""
    rng = np.random.default_rng(sr)
    return _file(sr, 2, [[(_words(rng, 20000, 60000), _ints(rng, 0.5, 3)) for _ in range(2)] for _ in range(5)])


def _hand_made_makers():
    P = functools.partial
    out = [(f"band_edges_{sr}", P(band_edge_file, sr)) for sr in RATES]
    for i, ch in enumerate([1, 2, 3, 6, 8]):
        sr = RATES[(3 * i + 1) % len(RATES)]
        out += [(f"words_{ch}ch_{sr}_{'dense' if d == 1.0 else 'sparse'}", P(words_file, ch, sr, d)) for d in (1.0, 0.1)]
    out += [("whole_file_quiet", P(level_file, 32768 + 35 * 256)), ("whole_file_loud", P(level_file, 32768 - 14 * 256)),
            ("zero_words", zero_words_file), ("wide_words_8000", P(wide_words_file, 8000)), ("wide_words_96000", P(wide_words_file, 96000))]
    out += [(f"frames_{n}", P(frame_count_file, n, 300 + n)) for n in (2, 3, 8, 9, 10, 16, 17, 18, 33, 40)]
    for ch, pats in ABSENT.items():
        out += [(f"absent_{ch}ch_{i}", P(absent_file, ch, p, 500 + 10 * ch + i)) for i, p in enumerate(pats)]
    out += [(f"blob_{kind}", P(blob_size_file, kind, 700 + i)) for i, kind in enumerate(("doubling", "records", "bytes", "in_place"))]
    return out


HAND_MADE = [n for n, _ in _hand_made_makers()]     # the tight class's hand-made files: finite in the oracle and in float64


@functools.lru_cache(maxsize=None)
def hand_made(name):
    return dict(_hand_made_makers())[name]()


ENCODER_GRID = [(q, sr, amp) for q in (0.0, 0.55, 1.0) for sr in (8000, 44100, 192000) for amp in (1.0, 1e-5, 3000.0)]


def encoder_names():
    from fixtures_util import LOSSY_EXAMPLES
    return [f"encoded_q{q}_{sr}_x{amp:g}" for q, sr, amp in ENCODER_GRID] + [f"example_{name}" for name, _, _ in LOSSY_EXAMPLES]


def encoder_cases(encode_lossy):
    """[(name, file bytes)]: encode_lossy(pcm, sr, channels, quality) of signals.music_like at every quality, rate and level
    of ENCODER_GRID (twelve frames of stereo), and the reference-made example files"""
    import signals
    from conftest import example_bytes
    from fixtures_util import LOSSY_EXAMPLES
    out = []
    for q, sr, amp in ENCODER_GRID:
        pcm = (signals.music_like(sr, 11 * 1024 + 300, 2, seed=int(sr + 100 * q)) * np.float32(amp)).astype(np.float32)
        out.append((f"encoded_q{q}_{sr}_x{amp:g}", encode_lossy(pcm, sr, 2, q)))
    out += [(f"example_{name}", example_bytes(name + ".flo")) for name, _, _ in LOSSY_EXAMPLES]
    return out


def edge_cases():
    """[(name, file bytes)] of the edge class: words 1 - 600 (the oracle's own FFT overflows) and 62000 - 65535 (subnormal
    factors): no f64 bound, the oracle is the authority"""
    out = []
    for name, lo, hi in (("tiny_words", 1, 600), ("huge_words", 62000, 65535)):
        rng = np.random.default_rng(lo)
        frames = [[(_words(rng, lo, hi), _ints(rng, 0.5, 3)) for _ in range(2)] for _ in range(5)]
        out.append((name, _file(44100, 2, frames)))
    rng = np.random.default_rng(9)
    frames = [[(_words(rng, 60000, 65535), _ints(rng, 1.0, extremes=True)) for _ in range(2)] for _ in range(5)]
    out.append(("huge_words_large_integers", _file(48000, 2, frames)))
    return out


_YARD = {}


def yardstick(name, flo):
    """(ref, scale, oracle's measure) of a file, computed once per process: the f64 decode and what O.decode's f32 decode
    is off by - the unit the device's error is counted in"""
    key = (name, len(flo), hash(flo))
    if key not in _YARD:
        ref, scale = decode(flo)
        _YARD[key] = (ref, scale, measure(O.decode(flo)[0], ref, scale))
    return _YARD[key]


WORST_MARGIN, RMS_MARGIN = 2.0, 1.5     # what the device's forward transform is given against f64, too


def assert_tight(name, flo, got):
    """`got`, a device decode of `flo`, against the f64 reference: finite, silent where the reference is, and per case no
    further from it than WORST_MARGIN x the oracle's own worst max|err| / scale and RMS_MARGIN x its relative RMS error
    (both measured here from O.decode, never from the device). Prints both sides' figures; -> (device, oracle) measures."""
    ref, scale, om = yardstick(name, flo)
    assert np.asarray(got).shape == ref.shape, (name, np.asarray(got).shape, ref.shape)
    dm = measure(got, ref, scale)
    b, c, p = dm["at"]
    print(f"{name:34s} worst max|err|/scale: device {dm['worst']:.2e} oracle {om['worst']:.2e}; relative RMS: device {dm['rms']:.2e} "
          f"oracle {om['rms']:.2e}; {dm['blocks']} blocks")
    where = (f"{name}: block {b} channel {c} position {p}: device {dm['got']!r}, f64 {dm['want']!r}, block scale {dm['scale']:.6e}; "
             f"device worst {dm['worst']:.3e} rms {dm['rms']:.3e}, oracle worst {om['worst']:.3e} rms {om['rms']:.3e}")
    assert dm["finite"], where
    assert dm["zero_ok"], f"{name}: block {dm['zero_at']} (block, channel) is silent in the reference and not on the device"
    assert dm["worst"] <= WORST_MARGIN * om["worst"], where
    assert dm["rms"] <= RMS_MARGIN * om["rms"], where
    return dm, om
