import numpy as np
import pytest

import flofile
import psy_ref
from fixtures_util import dequantise
from oracle import oracle as O


@pytest.fixture(scope="session")
def ctx():
    import flo_amd
    c = flo_amd.Context(0)
    yield c
    c.close()


def compare_lossy_stage(g, o, sr, tag=""):
    """SURVEY §8c tolerances (i)-(iv) for device-vs-oracle on identical input. g/o: dicts with coeffs,q,sf_words."""
    co, cg = o["coeffs"].astype(np.float64), g["coeffs"].astype(np.float64)
    rel = np.sqrt(((cg - co) ** 2).sum() / max((co ** 2).sum(), 1e-30))
    assert rel <= 1e-5, (tag, "coefficient relative RMS", rel)
    qo, qg = o["q"].astype(np.int32), g["q"].astype(np.int32)
    flips = int(((qo != 0) != (qg != 0)).sum())
    assert flips <= 5e-4 * qo.size, (tag, "keep/drop flips", flips, qo.size)
    # integers kept by both: an f32 FFT carries ABSOLUTE rounding noise of ~1e-7 x the frame's largest coefficient
    # (the oracle's FFT does too); in quantised units that noise is multiplied by the band's gain 30000/band_max.
    # So |dq| <= 1 + noise*gain everywhere, and where noise*gain is small (strong bands) mismatches stay under 1 %.
    both = (qo != 0) & (qg != 0)
    if both.any():
        band_g = O.psy_tables(sr)[1]
        gain = np.where(o["sf"] > 0, o["sf"], 0.0)[..., band_g] if "sf" in o else None
        d = np.abs(qo - qg)
        if gain is not None:
            fmax = np.abs(co).max(axis=2, keepdims=True)
            noise_q = 2e-6 * fmax * gain
            assert (d[both] <= 1 + noise_q[both]).all(), (tag, "kept mismatches beyond FFT noise", d[both].max())
            strong = both & (noise_q < 0.05)
            if strong.any():
                assert (d[strong] != 0).mean() <= 0.01, (tag, "mismatch rate in strong bands", (d[strong] != 0).mean())
        else:
            assert d[both].max() <= 1
    # scale words (256 steps per octave of 30000 / band_max): identical or +-1, except where the band's largest
    # coefficient is itself at the FFT's noise floor (a band of one or two bins far below the frame's peak, as the
    # lowest bands are at 128 kHz and up): the same absolute noise of ~1e-7 x frame maximum then moves the word by
    # 256 log2(1 + noise / band_max)
    sw = np.abs(o["sf_words"].astype(np.int32) - g["sf_words"].astype(np.int32))
    if "sf" in o:
        fmax = np.abs(co).max(axis=2, keepdims=True)                      # [hops][ch][1]
        bmax = np.where(o["sf"] > 0, 30000.0 / np.maximum(o["sf"], 1e-30), np.inf)   # [hops][ch][25]
        allow = 1 + 256 * np.log2(1 + 2e-6 * fmax / bmax)
        assert (sw <= allow + 1e-9).all(), (tag, "scale words", sw.max(), float((sw - allow).max()))
        assert (sw > 1).mean() <= 0.01, (tag, "scale words off by more than one", float((sw > 1).mean()))
    else:
        assert sw.max() <= 1, (tag, "scale words", sw.max())
    band = O.psy_tables(sr)[1]
    do, dg = dequantise(qo, o["sf_words"], band), dequantise(qg, g["sf_words"], band)
    den = np.sqrt((do ** 2).mean())
    if den > 0:
        db = 20 * np.log10(max(np.sqrt(((do - dg) ** 2).mean()), 1e-30) / den)
        assert db <= -80.0, (tag, "spectral RMS dB", db)
    return dict(rel=rel, flips=flips)


WINDOW_CAP = 1e-3      # largest share of a case's coefficients that may lie inside the undecided window


def explain_lossy_stage(g, coeffs, sr, quality, tag="", oracle=None):
    """Account for every coefficient and scale word of a device result against the f64 model of the stage (psy_ref).
    g: dict with the device's q [hops][ch][1024] and sf_words [hops][ch][25]; coeffs: the f32 coefficients they were
    computed from (the oracle's, hand-made ones, or the device's own transform). Where compare_lossy_stage bounds the
    RATE of disagreements, this asserts four rules coefficient by coefficient:

    keep/drop   Where |margin_f64| > eps the device's decision is the sign of the margin (margin = smr - smr_threshold).
                eps is measured per case, on the CPU, from the reference and never from the device: 4 x the oracle's own
                worst |smr_f32 - smr_f64| over this case's coefficients (O.lossy_quantize against psy_ref.model). The 4
                covers the device's second, independent set of roundings of about the same size - another summation
                order over up to ~900 bins, hardware log2 / exp2 at 1 ulp, the move from dB to amplitudes - plus headroom.
                Measured (tests/test_psy_ref_cpu.py prints them): the oracle's deviation is 1.0e-5 ... 1.5e-5 dB on
                music_like at every rate, channel count and quality, 1.1e-5 ... 2.8e-5 dB on the burst, silent-channel, DC,
                tone, impulse, square and fade classes, 2.0e-5 dB at x1e6, 2.8e-5 ... 3.2e-5 dB at x1e-5 ... x1e-10, and
                7.6e-6 ... 4.6e-5 dB on the hand-made and non-finite spectra (the ulp of dB values of 300 and more); eps is
                four times that: 3e-5 ... 1.8e-4 dB. The coefficients inside the window are left undecided; their share is
                asserted to stay within WINDOW_CAP = 1e-3 of the case (measured: at most 1.4e-4; music_like: 7e-5 even for a
                window of 1e-3 dB).
                A decision can only be observed through a non-zero integer: a coefficient the model keeps whose integer
                rounds to zero is satisfied by either decision.
    integers    Wherever the device keeps a coefficient - inside the window too - q = round_half_away(fl(c * sf)),
                sf = fl(30000 / band_max) (1 for band_max <= 1e-10). Tolerance zero: both sides are exact IEEE operations.
    scale words A word differs from floor(v), v = 256 log2(sf) + 32768 in f64, by at most one, and only where v lies within
                2^-8 + 256 ulp_f32(log2 sf) of that integer boundary (one f32 ulp of the final sum, the logarithm at
                1 ulp; the oracle's own f32 words disagree with f64 only within 2.1e-3 of a boundary). sf = 1 and powers of
                two give the exact word.
    non-finite  Where the margin is NaN (inf - inf) the decision must be O.lossy_quantize's, the authority there.

    On failure the worst offenders are listed with band, bin, hop, channel, margin and both decisions, and a per-band count.
    Returns dict(eps, window_share, worst_disagreement = largest |margin| at which device and model disagreed)."""
    from oracle import oracle as O
    coeffs = np.ascontiguousarray(coeffs, np.float32)
    m = psy_ref.model(coeffs, sr, quality)
    o = oracle if oracle is not None else O.lossy_quantize(coeffs, sr, quality)
    eps = 4.0 * psy_ref.oracle_deviation(m, o)
    margin, want_q, band = m["margin"], m["expect_q"], m["band"]
    qg = np.asarray(g["q"]).astype(np.int64)
    assert qg.shape == margin.shape, (tag, qg.shape, margin.shape)
    kept = qg != 0
    undefined = np.isnan(margin)
    with np.errstate(invalid="ignore"):
        inside = (np.abs(margin) <= eps) & ~undefined
        must_keep = (margin > eps) & (want_q != 0)
        must_drop = margin < -eps
    share = float(inside.mean())
    bad_keep = must_keep & ~kept
    bad_drop = must_drop & kept
    bad_int = kept & (qg != want_q)
    bad_nan = undefined & (kept != (o["q"] != 0))
    bad = bad_keep | bad_drop | bad_int | bad_nan
    with np.errstate(invalid="ignore"):
        model_keep = margin > 0
        dis = ~undefined & (kept != model_keep) & ~(model_keep & (want_q == 0))
    worst_dis = float(np.abs(margin[dis]).max()) if dis.any() else 0.0
    if bad.any():
        idx = np.argwhere(bad)
        order = np.argsort(-np.nan_to_num(np.abs(margin[bad]), nan=np.inf))[:12]
        lines = []
        for h, c, k in idx[order]:
            why = "dropped" if bad_keep[h, c, k] else "kept" if bad_drop[h, c, k] else "integer" if bad_int[h, c, k] else "non-finite"
            lines.append(f"  {why}: band {band[k]} bin {k} hop {h} ch {c} c={coeffs[h, c, k]!r} margin {margin[h, c, k]:+.3e} dB "
                         f"model {'keep' if margin[h, c, k] > 0 else 'drop'} q={want_q[h, c, k]} oracle q={int(o['q'][h, c, k])} "
                         f"device q={qg[h, c, k]}")
        per_band = np.bincount(band[idx[:, 2]], minlength=25)
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.size} coefficients unexplained (eps {eps:.2e} dB): "
                             f"{int(bad_keep.sum())} dropped, {int(bad_drop.sum())} kept, {int(bad_int.sum())} wrong integers, "
                             f"{int(bad_nan.sum())} non-finite\n" + "\n".join(lines) +
                             "\n  per band: " + ", ".join(f"{b}:{n}" for b, n in enumerate(per_band) if n))
    assert share <= WINDOW_CAP, (tag, "share of coefficients inside the undecided window", share, eps)
    lo, hi = psy_ref.word_bounds(m["sf"], m["word_v"])
    wg = np.asarray(g["sf_words"]).astype(np.int64)
    bad_w = (wg < lo) | (wg > hi)
    if bad_w.any():
        idx = np.argwhere(bad_w)[:12]
        lines = [f"  band {b} hop {h} ch {c}: sf={m['sf'][h, c, b]!r} v={m['word_v'][h, c, b]:.6f} admits {lo[h, c, b]}..{hi[h, c, b]} "
                 f"device {wg[h, c, b]}" for h, c, b in idx]
        raise AssertionError(f"{tag}: {int(bad_w.sum())} scale words unexplained\n" + "\n".join(lines) + "\n  per band: " +
                             ", ".join(f"{b}:{n}" for b, n in enumerate(np.bincount(np.argwhere(bad_w)[:, 2], minlength=25)) if n))
    return dict(eps=eps, window_share=share, worst_disagreement=worst_dis, model=m, oracle=o)


def same_structure(a: bytes, b: bytes):
    fa, fb = flofile.parse(a), flofile.parse(b)
    assert fa.crc_valid and fb.crc_valid
    for k in ("version", "flags", "sample_rate", "channels", "bit_depth", "total_samples", "level", "toc_size", "meta"):
        assert getattr(fa, k) == getattr(fb, k), k
    assert len(fa.frames) == len(fb.frames)
    assert [(f.frame_type, f.frame_samples, f.flags) for f in fa.frames] == [(f.frame_type, f.frame_samples, f.flags) for f in fb.frames]
    assert [t[3] for t in fa.toc] == [t[3] for t in fb.toc]
    return fa, fb


def snr_db(ref, x):
    ref, x = ref.astype(np.float64), x.astype(np.float64)
    n = min(ref.size, x.size)
    noise = ((ref[:n] - x[:n]) ** 2).sum()
    return 10 * np.log10(max((ref[:n] ** 2).sum(), 1e-30) / max(noise, 1e-30))
