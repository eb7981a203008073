"""A model of loudness normalisation and true-peak limiting as the device does it (flo_amd/csrc/normalize_plan.cpp,
normalize_kernels.hip), restated in numpy, and the case table of tests/test_gpu_normalize.py.

* the measure: h = the 1 -> 4 interpolator (resample_model.plan(1, 4), the table flo_resample_filter returns), the envelope
  through resample_model.chain, the exact FMA chain: envelope(), peaks(), true_peak().
* the plan: lookahead(), ceiling(), gain_plan() (f64, expression for expression), skip_bound(), the tile geometry.
* the limiter: r_of(), sliding_min(), sliding_sum(), limit(): integers behind the envelope.
* normalize(): one clip from its measured loudness and sample peak to the output and the report.
* cases(): the batches of the GPU tests, each clip a few tiles at the most, built once.
"""
import math

import numpy as np

import resample_model as RM

UNITY = 1 << 24
MAX_LOOKAHEAD = 1024          # kNormMaxLookahead
MIN_TILE = 2048               # kNormMinTile
THREADS = 512                 # kNormThreads
LDS_BYTES = 100 * 1024        # kNormLdsBytes
MAX_SCALED_PEAK = 2.0 ** 100  # kNormMaxScaledPeak
GAIN_MARGIN = 1.0 - 2.0 ** -15  # kNormGainMargin
GAIN, LIMIT = 0, 1
SILENT, NONFINITE = 1, 2
P14 = RM.plan(1, 4)

_table = None


def table():
    """h[4][64] f32"""
    global _table
    if _table is None:
        import flo_amd
        info, t = flo_amd.resample_filter(1, 4)
        assert (info["L"], info["M"], info["taps"]) == (4, 1, 64)
        _table = t
    return _table


# ---- the plan --------------------------------------------------------------------------------------------------------------
def lookahead(rate, asked=0):
    """frames, or None where the library refuses"""
    if asked > MAX_LOOKAHEAD:
        return None
    if asked:
        return asked
    a = (3 * rate + 1000) // 2000
    return None if a > MAX_LOOKAHEAD else max(a, 1)


def tile_frames(A):
    return max(8 * A, MIN_TILE)


def r_len(A):
    return tile_frames(A) + 4 * A


def m_len(A):
    return tile_frames(A) + 2 * A


def span(A):
    return r_len(A) + 63


def lds_bytes(A):
    return 2 * 4 * span(A)


def ceiling(ceiling_dbtp):
    return np.float32(math.pow(10.0, ceiling_dbtp / 20.0))


def skip_bound(h=None):
    """B: the largest row l1 norm times 1 + 2^-16, rounded up to f32"""
    h = table() if h is None else h
    b = float(np.abs(h.astype(np.float64)).sum(axis=1).max()) * (1.0 + 2.0 ** -16)
    f = np.float32(b)
    return f if float(f) >= b else np.nextafter(f, np.float32(np.inf))


def to_db(v):
    return 20.0 * math.log10(v) if v > 1e-9 else -150.0


def gain_plan(lufs, sample_peak_dbfs, tp, target=-14.0, ceiling_dbtp=-1.0, mode=GAIN, max_gain_db=30.0):
    """normalize_gain(): the report's fields but the two the kernel counts"""
    tp = np.float32(tp)
    rep = dict(input_lufs=float(lufs), input_true_peak=tp, input_true_peak_dbtp=to_db(float(tp)) if np.isfinite(tp) else float(tp),
               gain=np.float32(1.0), gain_db=0.0, ceiling_reduction_db=0.0, status=0)
    if not (math.isfinite(lufs) and math.isfinite(sample_peak_dbfs) and np.isfinite(tp)):
        rep["status"] = NONFINITE
        return rep
    if sample_peak_dbfs == -150.0:
        rep["status"] = SILENT
        return rep
    db = min(max(target - lufs, -max_gain_db), max_gain_db)
    g = np.float32(math.pow(10.0, db / 20.0))
    cap = float(ceiling(ceiling_dbtp)) * GAIN_MARGIN if mode == GAIN else MAX_SCALED_PEAK
    lowered = False
    if float(tp) * float(g) > cap:
        g = np.float32(cap / float(tp))
        while float(tp) * float(g) > cap:
            g = np.nextafter(g, np.float32(0.0))
        lowered = True
    rep["gain"] = g
    rep["gain_db"] = 20.0 * math.log10(float(g))
    rep["ceiling_reduction_db"] = db - rep["gain_db"] if lowered else 0.0
    return rep


# ---- the measure -----------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def envelope(y, ch):
    """(e[n, q, c] f32, subnormal): the four chains of every frame and channel of an interleaved f32 clip"""
    n = y.size // ch
    if not n:
        return np.zeros((0, 4, ch), np.float32), False
    e, sub = RM.chain(P14, table(), np.ascontiguousarray(y[:n * ch], np.float32), ch)
    return e.reshape(n, 4, ch), sub


def peaks(y, ch):
    """(p[n] as bit patterns (the magnitudes order like unsigned integers, any NaN above every number), subnormal)"""
    n = y.size // ch
    e, sub = envelope(y, ch)
    pb = np.maximum(_bits(y[:n * ch]).reshape(n, ch).max(axis=1, initial=0), _bits(e).reshape(n, 4 * ch).max(axis=1, initial=0))
    return pb.astype(np.uint32), sub


def true_peak(x, ch):
    """flo_batch_true_peak of one clip: f32; 0 without frames, the one quiet NaN where anything is NaN"""
    pb, _ = peaks(x, ch)
    v = np.uint32(pb.max(initial=0))
    if v > np.uint32(0x7F800000):
        v = np.uint32(0x7FC00000)
    return np.array([v], np.uint32).view(np.float32)[0]


# ---- the limiter -----------------------------------------------------------------------------------------------------------
def r_of(pb, C):
    """r[n] from p's bit patterns (finite): 2^24 where p <= C, else trunc((C / p) * 2^24) with the division in f32"""
    p = pb.view(np.float32)
    with np.errstate(all="ignore"):
        q = (np.float32(C) / np.where(p > C, p, np.float32(1.0))).astype(np.float32) * np.float32(16777216.0)
    return np.where(p <= C, np.uint32(UNITY), q.astype(np.uint32)).astype(np.uint32)


def sliding_min(r, A):
    """m[k] = min r[k - A .. k + A] for -A <= k < N + A, r outside the clip 2^24: N + 2A values, m[0] is k = -A"""
    pad = np.full(r.size + 4 * A, UNITY, np.uint32)
    pad[2 * A:2 * A + r.size] = r
    return np.lib.stride_tricks.sliding_window_view(pad, 2 * A + 1).min(axis=1)


def sliding_sum(m, A):
    """S[n] = sum m[n - A .. n + A] for 0 <= n < N (m as sliding_min returns it), int64"""
    c = np.concatenate([[0], np.cumsum(m.astype(np.int64))])
    return c[2 * A + 1:] - c[:-(2 * A + 1)]


def limit(y, ch, A, C):
    """(z, s, r, m, subnormal) of one interleaved f32 clip y (already at its gain)"""
    n = y.size // ch
    pb, sub = peaks(y, ch)
    r = r_of(pb, C)
    m = sliding_min(r, A)
    s = (sliding_sum(m, A) // (2 * A + 1)).astype(np.uint32)
    scale = s.astype(np.float32) * np.float32(2.0 ** -24)
    z = (y[:n * ch].reshape(n, ch) * scale[:, None]).astype(np.float32).reshape(-1)
    return z, s, r, m, sub


def normalize(x, ch, rate, lufs, sample_peak_dbfs, target=-14.0, ceiling_dbtp=-1.0, mode=GAIN, lookahead_frames=0, max_gain_db=30.0):
    """(out f32 [whole frames * ch], report, subnormal) of one clip from the loudness and the sample peak measured of it"""
    n = x.size // ch
    x = np.ascontiguousarray(x[:n * ch], np.float32)
    tp = true_peak(x, ch)
    rep = gain_plan(lufs, sample_peak_dbfs, tp, target, ceiling_dbtp, mode, max_gain_db)
    rep.update(limited_frames=0, min_gain_q24=UNITY)
    if rep["status"]:
        return x.copy(), rep, False
    y = (x * rep["gain"]).astype(np.float32)
    if mode == GAIN:
        return y, rep, False
    A = lookahead(rate, lookahead_frames)
    z, s, _, _, sub = limit(y, ch, A, ceiling(ceiling_dbtp))
    rep["limited_frames"] = int((s < UNITY).sum())
    rep["min_gain_q24"] = int(s.min(initial=UNITY))
    return z, rep, sub


def tile_skips(y, ch, A, C, tile):
    """whether tile `tile` of the clip y takes the short path: max |y| over its staged span times B at most C"""
    n = y.size // ch
    y0 = tile * tile_frames(A) - 2 * A - 31
    lo, hi = max(y0, 0), min(y0 + span(A), n)
    peak = _bits(y[lo * ch:hi * ch]).max(initial=0)
    v = np.array([peak], np.uint32).view(np.float32)[0]
    return bool(np.float32(v * skip_bound()) <= np.float32(C))


# ---- cases -----------------------------------------------------------------------------------------------------------------
GAIN_X2 = 20.0 * math.log10(2.0)


def _quiet(rng, n, ch, amp=0.05):
    """noise no sample of which is small enough for a product with a tap to be subnormal"""
    x = rng.uniform(-amp, amp, n * ch)
    x = np.where(np.abs(x) < 1e-6, 1e-6, x)
    return x.astype(np.float32)


def _spiky(rng, n, ch, amp=0.5, every=400):
    """noise with full-scale spikes every few hundred frames (at least one; every=None: none), each in a channel of its own"""
    x = _quiet(rng, n, ch, amp)
    if n and every:
        k = max(1, n // every)
        at = rng.integers(0, n, k)
        x.reshape(n, ch)[at, rng.integers(0, ch, k)] = rng.choice(np.array([-1.0, 1.0, 0.97], np.float32), k)
    return x


def _with_peaks(rng, n, ch, frames, c=None, v=1.0):
    x = _quiet(rng, n, ch)
    for f in frames:
        x.reshape(n, ch)[f, ch - 1 if c is None else c] = v
    return x


def lengths(A):
    t = tile_frames(A)
    return sorted({0, 1, 2, 30, 31, 32, 63, 64, A, 2 * A, 2 * A + 1, 4 * A + 62, 4 * A + 63, 4 * A + 64, t - 1, t, t + 1, 2 * t + 1, 3 * t + 5})


def _case(name, rate, ch, clips, mode=LIMIT, gain_db=0.0, ceiling_dbtp=-1.0, A=0, why=""):
    """every clip of a case gets the same gain, whatever its loudness: the target is out of reach (+30 LUFS) and max_gain_db
    is the gain wanted; 0 dB is a gain of exactly 1"""
    return dict(name=name, rate=rate, ch=ch, clips=clips, mode=mode, target=30.0, max_gain_db=gain_db, ceiling=ceiling_dbtp, lookahead_frames=A,
                A=lookahead(rate, A), why=why)


RESAMPLER_SHAPES = [(48000, 2), (44100, 1), (96000, 3), (8000, 6)]


def resampler_clips(rate, ch):
    """full-scale noise of a few lengths around the peak kernel's tile, for the comparison of Batch.true_peaks with
    Batch.resample at four times the rate (no sample small enough for a subnormal product: test_normalize_model_cpu.py)"""
    rng = np.random.default_rng(rate + ch)
    return [_quiet(rng, n, ch, amp=1.0) for n in (0, 1, 31, 64, 2047, 2048, 2049, 5000)]


_cases = None


def cases():
    """the batches: dicts with name, rate, ch, mode, target, max_gain_db, ceiling, lookahead_frames (as asked), A (in force),
    clips [(name, f32 interleaved)]"""
    global _cases
    if _cases is not None:
        return _cases
    out = []
    rng = np.random.default_rng(20240)
    A, t = 72, tile_frames(72)
    out.append(_case("lengths_limit", 48000, 2, [("n%d" % n, _spiky(rng, n, 2)) for n in lengths(A)], why="every length of the list, spikes all over"))
    out.append(_case("lengths_gain", 48000, 2, [("n%d" % n, _spiky(rng, n, 2, amp=0.2, every=None) if n % 2 else _spiky(rng, n, 2)) for n in lengths(A)],
                     mode=GAIN, gain_db=9.0, why="GAIN mode: quiet clips take the whole 9 dB, spiky ones are held by the ceiling"))
    n = t + 300
    where = [("first", [0]), ("last", [n - 1]), ("before_tile", [t - 1]), ("at_tile", [t]), ("apart_2A", [500, 500 + 2 * A]),
             ("apart_2A_1", [500, 500 + 2 * A + 1]), ("apart_4A", [500, 500 + 4 * A]), ("apart_4A_2", [500, 500 + 4 * A + 2]),
             ("across_tile_2A", [t - A, t + A]), ("across_tile_4A_2", [t - 2 * A - 1, t + 2 * A + 1])]
    out.append(_case("peak_places", 48000, 1, [(k, _with_peaks(rng, n, 1, f)) for k, f in where], why="where the peak sits, how far two lie apart"))
    for ch in (1, 2, 3, 6):
        out.append(_case("last_channel_x%d" % ch, 48000, ch, [("one", _with_peaks(rng, t + 100, ch, [t - 40, 900])), ("short", _with_peaks(rng, 50, ch, [7]))],
                         why="the peak in the last channel only"))
    # the skip bound at gain 1: the largest sample just meets it, or misses it by one ulp; the rest far below
    B, C = skip_bound(), ceiling(-1.0)
    hit = np.float32(float(C) / float(B))
    while np.float32(hit * B) > C:
        hit = np.nextafter(hit, np.float32(0.0))
    while np.float32(np.nextafter(hit, np.float32(1.0)) * B) <= C:
        hit = np.nextafter(hit, np.float32(1.0))
    miss = np.nextafter(hit, np.float32(1.0))
    out.append(_case("skip_bound", 48000, 2, [("meets", _with_peaks(rng, t + 50, 2, [100, t + 10], v=hit)), ("misses", _with_peaks(rng, t + 50, 2, [100, t + 10], v=miss)),
                                            ("misses_in_halo", _with_peaks(rng, 2 * t, 2, [t + 2 * A + 31], v=miss)),
                                            ("meets_beyond_halo", _with_peaks(rng, 2 * t, 2, [t + 2 * A + 33], v=1.0))],
                     why="tiles that just take, or just miss, the short path"))
    dc = np.full((t + 17) * 2, 0.95, np.float32)
    k = np.arange(t + 17)
    sine = np.repeat(np.sin(np.pi / 2 * k + np.pi / 4).astype(np.float32), 2)
    out.append(_case("dc_and_sine", 48000, 2, [("dc_0.95", dc), ("fs4_sine_45deg", sine)], why="a DC clip above the ceiling; samples at 0.707 under a true peak of 1"))
    bad_nan = _spiky(rng, 700, 2)
    bad_nan[333] = np.nan
    bad_inf = _spiky(rng, 700, 2)
    bad_inf[1] = -np.inf
    out.append(_case("copied", 48000, 2, [("zeros", np.zeros(900 * 2, np.float32)), ("below_1e-6", _quiet(rng, 900, 2, amp=5e-7) * np.float32(0.5)),
                                        ("nan", bad_nan), ("inf", bad_inf), ("loud", _spiky(rng, 700, 2)), ("negative_zero", np.full(64, -0.0, np.float32))],
                     why="silent and non-finite clips are copied, with their status"))
    out.append(_case("copied_gain", 48000, 2, [("zeros", np.zeros(900 * 2, np.float32)), ("nan", bad_nan), ("loud", _spiky(rng, 700, 2))], mode=GAIN, gain_db=9.0,
                     why="the same in GAIN mode"))
    for db, name in ((GAIN_X2, "x2"), (2 * GAIN_X2, "x4")):
        out.append(_case("gain_" + name, 48000, 2, [("spiky", _spiky(rng, t + 700, 2, amp=0.3)), ("quiet", _quiet(rng, 3000, 2, amp=0.1))], gain_db=db,
                         why="the limiter behind a gain of " + name))
    for rate in (8000, 48000, 384000):
        for a in (1, 12, 72, 576, 1024):
            ta = tile_frames(a)
            out.append(_case("A%d_at_%d" % (a, rate), rate, 2, [("2_tiles_1", _spiky(rng, 2 * ta + 1, 2, every=max(400, 3 * a))), ("4A_63", _spiky(rng, 4 * a + 63, 2, every=100))], A=a,
                             why="every look-ahead at every rate"))
    out.append(_case("default_lookahead_8000", 8000, 1, [("one", _spiky(rng, 2500, 1))], why="A = 12 by default"))
    ragged = [("c%02d" % i, _spiky(rng, 0 if i % 9 == 4 else int(rng.integers(1, 5000)), 1, amp=float(rng.choice([0.05, 0.5])))) for i in range(64)]
    out.append(_case("ragged_64", 48000, 1, ragged, why="64 clips of every length, empty ones among them"))
    _cases = out
    return out
