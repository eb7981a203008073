"""The bands' hearing floors (StatMasks::band_ath_floor in flo_amd/csrc/pack_rows.h, built by tables.cpp), which the
lock-step stereo chain kernel's band-alive ballot compares a band's maximum against, on the host (read through
tests/ath_floor_tables.py, a small program compiled against tables.cpp):

    table       band_ath_floor[b] is the minimum of ath_lin over exactly the bins whose band is b, +inf for a band without
                bins at the sample rate and for entries 25..31
    superset    on the oracle's analysis of two of the benchmark's synthetic clips: every band that holds a non-zero integer
                has a maximum above its floor (the refined ballot never kills a band that keeps something), and in every
                frame at least one band is above its masking amplitude (tests/psy_ref.py) and not above its floor (the
                refinement has something to rule out: the first property does not hold vacuously)
"""
import numpy as np
import pytest

import ath_floor_tables
import psy_ref
from oracle import oracle as O

RATES = [44100, 48000, 96000, 8000]
QUALITIES = [0.0, 0.55, 0.8, 0.99]


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("rate", RATES)
def test_floor_is_the_minimum_over_the_bands_bins(rate, quality):
    t = ath_floor_tables.load(rate, quality)
    assert np.isfinite(t["ath_lin"]).all() and (t["ath_lin"] >= 0).all()
    assert t["band"].max() < 25
    for b in range(32):
        bins = np.flatnonzero(t["band"] == b)
        if bins.size:
            want = t["ath_lin"][bins].min()
            assert t["floor"][b].view(np.uint32) == want.view(np.uint32), (rate, quality, b, float(t["floor"][b]), float(want))
        else:
            assert t["floor"][b] == np.inf, (rate, quality, b, float(t["floor"][b]))
    assert (t["floor"][25:] == np.inf).all()
    if rate == 8000:      # the case is what it is here for: at this rate some of the 25 bands have no bins
        assert any((t["band"] == b).sum() == 0 for b in range(25))


@pytest.mark.parametrize("clip_id", [0, 1])
def test_floor_kills_no_band_that_keeps_something_and_kills_some(clip_id):
    sr, q, frames = 44100, 0.55, 40
    t = ath_floor_tables.load(sr, q)
    pcm = O.synth_clip(frames * 1024, 2, clip_id=clip_id)
    o = O.lossy_analyze(pcm, sr, 2, q)
    assert o["q"].shape[0] >= frames
    coeffs, ints = o["coeffs"][:frames], o["q"][:frames]
    m = psy_ref.model(coeffs, sr, q)
    assert np.array_equal(m["band"], t["band"])          # the reference's band map is the table builder's
    floor = t["floor"][:25].astype(np.float64)
    bmax = m["band_max"].astype(np.float64)                 # [frames][ch][25]
    # the band's masking amplitude: |c| is kept against the masking level alone iff 20 log10 |c| - (level - 10) > smr_thr
    smr_thr = np.float64(np.float32(O.lib().flo_o_smr_threshold(float(q))))
    tl1 = 10.0 ** ((smr_thr + m["level"] - 10.0) / 20.0)
    holds = np.stack([(ints[..., t["band"] == b] != 0).any(-1) for b in range(25)], -1)
    above_floor = bmax > floor
    bad = np.argwhere(holds & ~above_floor)
    assert bad.size == 0, (clip_id, "a band (frame, channel, band) keeps an integer under its floor", bad[0].tolist())
    ruled_out = (bmax > tl1) & ~above_floor
    per_frame = ruled_out.any(axis=(1, 2))
    assert per_frame.all(), (clip_id, "frames in which the floor rules nothing out", np.flatnonzero(~per_frame).tolist())
