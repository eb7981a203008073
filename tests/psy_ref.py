"""High-precision model of the lossy stage behind the transform: a vectorised numpy f64 restatement of the oracle's
psy_masking_threshold, psy_calculate_smr and keep test (oracle/lossy.c), coefficients in.

What is f64 here is every sum, logarithm, maximum and subtraction the reference rounds to f32. What is NOT changed is
the reference's semantics: its f32 tables (O.psy_tables: ATH, band of a bin, spreading matrix), the f32 constants
1e-10f and 0.7f, the f32 quality threshold, the `> 1e-10` branches of band energy / band maximum / signal level (all
three compare exact f32 inputs, or - the band energy's - land on the -100 dB floor from either side, so no branch can
fall differently in f32 and f64 for finite input), and the maxima that skip NaN (fmaxf). An f32 sum of squares that
overflows is +inf in the reference; the model reproduces that from the f64 sum. Where non-finite input leaves the
margin NaN the caller falls back on O.lossy_quantize, the authority for such input.

The scale factor and the kept integer are exact IEEE f32 operations in the reference (one division, one product, one
rounding): the model computes them in f32, bit for bit."""
import numpy as np

from oracle import oracle as O

F32_TINY = np.float32(1e-10)
DECAY = np.float64(np.float32(0.7))
F32_MAX = np.float64(np.finfo(np.float32).max)


def band_slices(band):
    """[(lo, hi)] per band: the bins of a band are contiguous and ascending (hi == lo for an empty band)."""
    band = np.asarray(band).astype(np.int64)
    assert (np.diff(band) >= 0).all()
    return [(int(np.searchsorted(band, b, "left")), int(np.searchsorted(band, b, "right"))) for b in range(25)]


def round_half_away_i16(x):
    """f32::round then `as i16` (saturating, NaN -> 0) of an f32 array, exactly."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.trunc(x)
        d = (x - t).astype(np.float32)                      # exact
        r = np.where(np.isfinite(x), t + np.trunc(d + d), x)
        r = np.where(np.isnan(r), 0.0, np.clip(r, -32768.0, 32767.0))
    return r.astype(np.int64)


def model(coeffs, sample_rate, quality):
    """coeffs [hops][ch][1024] f32 -> dict of
    per coefficient: margin (f64, smr - smr_threshold; keep iff > 0), smr (f64), expect_q (the integer a kept
                     coefficient must become), band [1024];
    per band:        sf (exact f32 scale factor), word_v (f64 256 log2(sf) + 32768, clamped like the reference; NaN for
                     sf <= 1e-10 whose word is 0), band_db, level (masking level s after temporal masking),
                     set_by (distance i - j of the band j whose spread term alone sets band i's level in this frame,
                     -1 where the -100 dB floor, the temporal term or several terms together do)."""
    c32 = np.ascontiguousarray(coeffs, np.float32)
    assert c32.ndim == 3 and c32.shape[2] == 1024
    hops, nch, _ = c32.shape
    ath32, band, spreading32 = O.psy_tables(sample_rate)
    band = band.astype(np.int64)
    sl = band_slices(band)
    count = np.array([hi - lo for lo, hi in sl], np.float64)
    c = c32.astype(np.float64)
    a = np.abs(c)
    with np.errstate(all="ignore"):
        c2 = c * c
        energy = np.stack([c2[..., lo:hi].sum(-1) if hi > lo else np.zeros(c2.shape[:2]) for lo, hi in sl], -1)
        energy = np.where(energy > F32_MAX, np.inf, energy)             # the f32 accumulator overflows
        bmax32 = np.stack([np.fmax.reduce(np.abs(c32[..., lo:hi]), axis=-1, initial=np.float32(0.0)) if hi > lo
                           else np.zeros(c2.shape[:2], np.float32) for lo, hi in sl], -1).astype(np.float32)
        live = (count > 0) & (energy > np.float64(F32_TINY))            # NaN compares false
        band_db = np.where(live, 10.0 * np.log10(np.where(live, energy, 1.0) / np.where(count > 0, count, 1.0)), -100.0)
        L = 10.0 * np.log10(spreading32.astype(np.float64))             # [j][i]; -inf where the f32 power underflowed
        terms = band_db[..., :, None] + L                               # [hops][ch][j][i]; inf - inf = NaN is skipped
        spread = np.fmax(np.fmax.reduce(terms, axis=-2), -100.0)
        # which single band sets the level: strictly above every other term and the floor
        order = np.sort(np.where(np.isnan(terms), -np.inf, terms), axis=-2)
        top_j = np.argmax(np.where(np.isnan(terms), -np.inf, terms), axis=-2)
        alone = (order[..., -1, :] > order[..., -2, :]) & (order[..., -1, :] > -100.0)
        dist = np.arange(25)[None, None, :] - top_j
        spread = spread - 6.0
        level = np.empty_like(spread)
        prev = np.zeros((nch, 25))
        from_spread = np.zeros(spread.shape, bool)
        for h in range(hops):
            t = prev * DECAY
            level[h] = np.fmax(spread[h], t)
            from_spread[h] = spread[h] > t
            prev = level[h]
        set_by = np.where(alone & from_spread, dist, -1)
        thr = np.fmax(level[..., band], ath32.astype(np.float64)) - 10.0
        big = c32_gt(a, F32_TINY)
        signal_db = np.where(big, 20.0 * np.log10(np.where(big, a, 1.0)), -100.0)
        smr = signal_db - thr
        margin = smr - np.float64(np.float32(O.lib().flo_o_smr_threshold(float(quality))))
        sf = np.where(bmax32 > F32_TINY, np.float32(30000.0) / np.where(bmax32 > F32_TINY, bmax32, np.float32(1.0)),
                      np.float32(1.0)).astype(np.float32)
        expect_q = round_half_away_i16(c32 * sf[..., band])
        sfd = sf.astype(np.float64)
        word_v = np.where(sf > F32_TINY, np.clip(256.0 * np.log2(np.where(sf > F32_TINY, sfd, 1.0)) + 32768.0, 0.0, 65535.0), np.nan)
    return dict(margin=margin, smr=smr, expect_q=expect_q, band=band, sf=sf, word_v=word_v, band_db=band_db, level=level,
                set_by=set_by, band_max=bmax32)


def c32_gt(a64, tiny32):
    """|c| > 1e-10f as the reference compares it: both sides are exact f32 values (NaN false)."""
    with np.errstate(invalid="ignore"):
        return a64 > np.float64(tiny32)


def word_bounds(sf, word_v):
    """Scale words the model admits, per band (lo, hi inclusive). v = 256 log2(sf) + 32768 in f64; a word may leave
    floor(v) only by one and only where v lies within 2^-8 + 256 ulp_f32(log2 sf) of the integer boundary (one f32 ulp of
    the final sum in [2^15, 2^16), the logarithm at 1 ulp). sf = 1 and exact powers of two admit the exact word only;
    sf <= 1e-10 (a band maximum of +inf gives 30000 / inf = 0) has word 0."""
    sf = np.asarray(sf, np.float32)
    with np.errstate(all="ignore"):
        lg = np.abs(np.log2(np.where(sf > F32_TINY, sf, np.float32(1.0)).astype(np.float64)))
        tol = 2.0 ** -8 + 256.0 * np.spacing(np.maximum(lg, np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
        mant, _ = np.frexp(sf)
        tol = np.where(mant == 0.5, 0.0, tol)                           # powers of two, sf = 1 among them
        v = np.where(np.isnan(word_v), 0.0, word_v)
        lo = np.clip(np.floor(v - tol), 0, 65535)
        hi = np.clip(np.floor(v + tol), 0, 65535)
    dead = ~(sf > F32_TINY)
    return np.where(dead, 0, lo).astype(np.int64), np.where(dead, 0, hi).astype(np.int64)


def oracle_deviation(m, o):
    """Worst |smr_f32 - smr_f64| of the oracle result o against the model m over the coefficients where both are finite."""
    with np.errstate(invalid="ignore"):
        d = np.abs(o["smr"].astype(np.float64) - m["smr"])
    ok = np.isfinite(d)
    return float(d[ok].max()) if ok.any() else 0.0
