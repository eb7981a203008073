"""The f64 model of the lossy stage (psy_ref) against the oracle, on the CPU: before explain_lossy_stage judges a device
result, the model and the oracle's new coefficient entry have to agree with the reference restatement itself, on every
input class the device tests use. Each test prints, per class, the oracle's worst |smr_f32 - smr_f64| (a quarter of the
window explain_lossy_stage then uses) and the share of coefficients inside that window."""
import numpy as np
import pytest

import lossy_cases
import psy_ref
import signals
from gpu_util import WINDOW_CAP, compare_lossy_stage, explain_lossy_stage
from oracle import oracle as O


def _report(name, r, o):
    print(f"{name:34s} oracle |smr_f32 - smr_f64| <= {r['eps'] / 4:.2e} dB, window {r['eps']:.2e} dB holds "
          f"{r['window_share']:.1e} of {o['q'].size} coefficients, {int((o['q'] != 0).sum())} kept")


def test_oracle_coefficient_entry_reproduces_the_clip_driver():
    # O.lossy_quantize over the driver's own coefficients is the driver, bit for bit (temporal state per channel included)
    for name, pcm, sr, ch, q in lossy_cases.pcm_cases():
        o = O.lossy_analyze(pcm, sr, ch, q)
        o2 = O.lossy_quantize(o["coeffs"], sr, q)
        for key in ("smr", "q", "sf", "sf_words"):
            assert np.array_equal(o[key].view(np.uint8), o2[key].view(np.uint8)), (name, key)
    o = O.lossy_quantize(np.zeros((0, 2, 1024), np.float32), 44100, 0.55)
    assert o["q"].shape == (0, 2, 1024)


def test_oracle_decisions_are_the_sign_of_the_f64_margin_on_pcm_classes():
    # the oracle's own f32 result must pass explain_lossy_stage: every decision outside the window is the sign of the
    # f64 margin, every kept integer and scale word is the model's, and the window holds at most 1e-3 of the case
    for name, pcm, sr, ch, q in lossy_cases.pcm_cases():
        o = O.lossy_analyze(pcm, sr, ch, q)
        r = explain_lossy_stage(o, o["coeffs"], sr, q, name, oracle=o)
        _report(name, r, o)
        assert r["window_share"] <= WINDOW_CAP


def test_oracle_decisions_are_the_sign_of_the_f64_margin_on_hand_made_spectra():
    far_cases = 0
    for name, c, sr, q, needs_far in lossy_cases.spectra_cases():
        o = O.lossy_quantize(c, sr, q)
        r = explain_lossy_stage(o, c, sr, q, name, oracle=o)
        _report(name, r, o)
        assert r["window_share"] <= WINDOW_CAP
        if needs_far:
            # a spread term of distance >= 9 alone sets some band's level here (the far branch of the device's
            # spread_threshold is then observable), and probes on both sides of that level exist
            far = r["model"]["set_by"] >= 9
            assert far.any(), name
            probes = (c != 0)[..., :]
            band = r["model"]["band"]
            hit = [(h, ch_, b) for h, ch_, b in np.argwhere(far)]
            seen = [(o["q"][h, ch_][band == b] != 0).any() and ((probes[h, ch_] & (o["q"][h, ch_] == 0))[band == b]).any() for h, ch_, b in hit]
            assert any(seen), (name, "no far-set band has both a kept and a dropped probe")
            far_cases += 1
    assert far_cases >= 10


def test_transformed_pcm_never_lets_a_far_term_decide():
    # what the PCM route cannot reach: however loud, no band's level is set by a term of distance >= 9 (an f32 transform
    # leaves a floor ~140 dB below the frame maximum in every band, and 25 dB per band falls below it after five bands)
    for amp in (1.0, 3000.0, 1e6, 1e12):
        pcm = signals.music_like(44100, 30000, 2, seed=3) * np.float32(amp)
        o = O.lossy_analyze(pcm, 44100, 2, 0.55)
        assert psy_ref.model(o["coeffs"], 44100, 0.55)["set_by"].max() < 9, amp


def test_reference_keeps_tiny_coefficients_at_transparent_quality():
    # |c| <= 1e-10 has signal_db = -100, and at quality >= 0.99 (smr_threshold = -100) it is kept wherever its threshold
    # is below 0 dB; with a band maximum just above 1e-10 it becomes a non-zero integer. Model and oracle agree on it.
    pcm = signals.music_like(44100, 10000, 2, seed=11) * np.float32(1e-8)
    o = O.lossy_analyze(pcm, 44100, 2, 1.0)
    kept = o["q"] != 0
    assert kept.sum() > 500 and (np.abs(o["coeffs"][kept]) <= np.float32(1e-10)).all()
    m = psy_ref.model(o["coeffs"], 44100, 1.0)
    assert (m["margin"][kept] > 0).all() and np.array_equal(m["expect_q"][kept], o["q"][kept])
    assert not (O.lossy_analyze(pcm, 44100, 2, 0.55)["q"] != 0).any()


def test_non_finite_spectra_follow_the_oracle():
    for name, c, sr, q in lossy_cases.nonfinite_cases():
        o = O.lossy_quantize(c, sr, q)
        r = explain_lossy_stage(o, c, sr, q, name, oracle=o)
        _report(name, r, o)
        # the model is defined (and right) everywhere but at inf - inf
        undefined = np.isnan(r["model"]["margin"])
        assert undefined.sum() <= 4 and (~np.isfinite(c[undefined])).all(), name


def test_scale_word_bounds_on_exact_factors():
    sf = np.array([1.0, 2.0, 0.5, 2.0 ** 20, 2.0 ** -20, 30000.0, 3e14, 1.0000001], np.float32)
    v = 256.0 * np.log2(sf.astype(np.float64)) + 32768.0
    lo, hi = psy_ref.word_bounds(sf, v)
    for i in range(5):
        assert lo[i] == hi[i] == int(v[i])                 # sf = 1 and powers of two: the exact word only
    assert (hi - lo <= 1).all() and lo[7] == 32767 and hi[7] == 32768      # next to a boundary: either side
    words = np.array([O.lib().flo_o_scale_factor_word(float(s)) for s in sf])
    assert ((words >= lo) & (words <= hi)).all()
    lo0, hi0 = psy_ref.word_bounds(np.array([0.0, 1e-11], np.float32), np.array([np.nan, np.nan]))
    assert not lo0.any() and not hi0.any()


def _decisions_with_level(m, o, sr, q, level):
    """the integers a quantiser would give that used `level` [hops][ch][25] as the bands' masking levels"""
    thr = np.maximum(level[..., m["band"]], O.psy_tables(sr)[0].astype(np.float64)) - 10.0
    a = np.abs(o["coeffs"].astype(np.float64))
    with np.errstate(divide="ignore"):
        smr = np.where(a > 1e-10, 20 * np.log10(np.where(a > 1e-10, a, 1.0)), -100.0) - thr
    keep = smr > np.float64(np.float32(O.lib().flo_o_smr_threshold(q)))
    return np.where(keep, m["expect_q"], 0).astype(np.int16)


@pytest.mark.parametrize("fault", ["band_edge_bin", "one_bin_band", "other_channel", "integer", "scale_word"])
def test_explanation_names_a_planted_fault_the_rate_bounds_let_through(fault):
    """The point of the per-coefficient account: systematic errors of a handful of coefficients, planted in a copy of the
    oracle's own result. explain_lossy_stage fails on every one and names the band. compare_lossy_stage's flip and mismatch
    RATES admit all of them; its -80 dB spectral bound notices a wrongly decided coefficient only where that coefficient
    is large against the whole clip (the one-bin-band and other-channel faults here), never the band-edge, integer and
    scale-word ones."""
    sr, q = (384000, 0.55) if fault == "one_bin_band" else (44100, 0.55)
    pcm = signals.music_like(sr, 40000, 2, seed=5)
    o = O.lossy_analyze(pcm, sr, 2, q)
    m = psy_ref.model(o["coeffs"], sr, q)
    band = m["band"]
    g = {k: v.copy() for k, v in o.items()}
    if fault == "band_edge_bin":
        # the first bin of band 20 takes band 19's level
        k = int(np.searchsorted(band, 20))
        level = m["level"].copy()
        level[..., 20] = level[..., 19]
        g["q"][..., k] = _decisions_with_level(m, o, sr, q, level)[..., k]
        want = f"band 20 bin {k} "
    elif fault == "one_bin_band":
        # a band of one bin decided against a level 3 dB too high in every third frame
        b = 8
        assert (band == b).sum() == 1
        level = m["level"].copy()
        level[::3, :, b] += 3.0
        g["q"] = _decisions_with_level(m, o, sr, q, level)
        want = f"band {b} "
    elif fault == "other_channel":
        # channel 1 reads channel 0's level of band 9 in every fifth frame
        level = m["level"].copy()
        level[::5, 1, 9] = level[::5, 0, 9]
        g["q"] = _decisions_with_level(m, o, sr, q, level)
        want = "band 9 "
    elif fault == "integer":
        h, c, k = np.argwhere((o["q"] > 1) & (band == 6)[None, None, :])[0]
        g["q"][h, c, k] += 1
        want = "band 6 "
    else:
        frac = m["word_v"] - np.floor(m["word_v"])
        h, c, b = np.argwhere((frac > 0.3) & (frac < 0.7) & (np.arange(25) == 14))[0]
        g["sf_words"][h, c, b] += 1
        want = "band 14 "
    assert not (np.array_equal(g["q"], o["q"]) and np.array_equal(g["sf_words"], o["sf_words"]))
    changed = int((g["q"] != o["q"]).sum() + (g["sf_words"] != o["sf_words"]).sum())
    assert 1 <= changed <= 10
    try:
        compare_lossy_stage(g, o, sr, tag=fault)
        noticed = None
    except AssertionError as e:
        noticed = e.args[0][1]
    print(f"{fault}: {changed} values changed; compare_lossy_stage {'passes' if noticed is None else 'fails on ' + noticed}")
    if fault in ("band_edge_bin", "integer", "scale_word"):
        assert noticed is None
    else:
        assert noticed in (None, "spectral RMS dB")        # never the rates
    with pytest.raises(AssertionError) as e:
        explain_lossy_stage(g, o["coeffs"], sr, q, fault, oracle=o)
    print(str(e.value)[:800])
    assert want in str(e.value) and "per band" in str(e.value), str(e.value)[:2000]
