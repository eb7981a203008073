"""Input classes of the explained lossy-stage tests (test_psy_ref_cpu.py on the CPU, test_gpu_lossy_explained.py on
the device): PCM clips for the whole pipeline and hand-made spectra for the isolated quantiser. Everything is
deterministic and built from numpy alone."""
import numpy as np

import psy_ref
import signals
from oracle import oracle as O

RATES = [8000, 22050, 48000, 96000, 128000, 176400, 192000, 384000]      # test_other_sample_rates
QUALITIES = [0.0, 0.35, 0.55, 0.75, 1.0]
BARK_EDGES = [100, 200, 300, 400, 510, 630, 770, 920, 1080, 1270, 1480, 1720, 2000, 2320, 2700, 3150, 3700, 4400, 5300,
              6400, 7700, 9500, 12000, 15500, 20500]


def _f32(x):
    return np.ascontiguousarray(x, np.float32).reshape(-1)


def _bark_edge_tones(sr, ch):
    """one tone per Bark edge below the Nyquist frequency, 4096 sample-frames each, back to back"""
    segs = [signals.sine(float(f), sr, 4096, 0.4, ch) for f in BARK_EDGES if f < 0.49 * sr]
    return np.concatenate(segs)


def pcm_cases():
    """-> list of (name, pcm interleaved f32, sample_rate, channels, quality)"""
    out = []
    for sr in RATES:
        out.append((f"rate{sr}", signals.music_like(sr, 20000, 2, seed=sr), sr, 2, 0.55))
    for ch in (1, 2, 3, 6, 8):
        out.append((f"ch{ch}", signals.music_like(44100, 12000, ch, seed=70 + ch), 44100, ch, 0.55))
    for q in QUALITIES:
        out.append((f"quality{q}", signals.music_like(44100, 20000, 2, seed=3), 44100, 2, q))
    sr = 44100
    # a loud burst, seconds at 1e-4, a burst: 0.7 x the previous level decides for many frames
    n = 3 * sr
    x = signals.fast_noise(n * 2, 4, 1e-4)
    x[: sr // 2] += signals.music_like(sr, sr // 4, 2, seed=2) * 2.0
    x[5 * sr: 5 * sr + sr // 2] += signals.music_like(sr, sr // 4, 2, seed=5)
    out.append(("burst_quiet_burst", np.clip(x, -1, 1), sr, 2, 0.55))
    m = signals.music_like(sr, 16000, 2, seed=11)
    a = m.copy(); a[1::2] = 0.0
    out.append(("right_silent", a, sr, 2, 0.55))
    a = m.copy(); a[0::2] = 0.0
    out.append(("left_silent", a, sr, 2, 0.55))
    a = m.copy(); a[1::2] *= np.float32(1e-3)
    out.append(("right_60dB_down", a, sr, 2, 0.55))
    out.append(("dc", np.full(12000 * 2, 0.5, np.float32), sr, 2, 0.55))
    out.append(("bark_edge_tones_44100", _bark_edge_tones(44100, 1), 44100, 1, 0.55))
    out.append(("bark_edge_tones_8000_stereo", _bark_edge_tones(8000, 2), 8000, 2, 0.75))
    a = np.zeros(9000 * 2, np.float32); a[2 * 3000] = 1.0; a[2 * 5000 + 1] = -1.0
    out.append(("impulse", a, sr, 2, 0.55))
    sq = np.where((np.arange(16000) // 50) % 2 == 0, 1.0, -1.0).astype(np.float32)
    out.append(("square_full_scale", np.repeat(sq, 2), sr, 2, 0.55))
    out.append(("level_x3000", m * np.float32(3000.0), sr, 2, 0.55))
    out.append(("level_x1e6", m * np.float32(1e6), sr, 2, 0.55))
    for e in range(5, 11):
        for q in (1.0, 0.55):
            out.append((f"level_x1e-{e}_q{q}", m[:2 * 10000] * np.float32(10.0 ** -e), sr, 2, q))
    ramp = np.linspace(1.0, 0.0, 16000).astype(np.float32)
    ramp[-2000:] = 0.0                                   # ... to exact zero
    fade = (signals.music_like(sr, 16000, 2, seed=12).reshape(-1, 2) * 4.0).clip(-1, 1) * ramp[:, None]
    out.append(("fade_to_zero_q1.0", fade, sr, 2, 1.0))
    out.append(("fade_to_zero_q0.55", fade, sr, 2, 0.55))
    return [(name, _f32(p), sr_, ch, q) for name, p, sr_, ch, q in out]


# ------------------------------------------------------------------------------------------------ hand-made spectra
def _amp(db):
    return np.float32(10.0 ** (db / 20.0))


def _with_probes(base, sr, q, offsets_db=(-3.0, -0.3, 0.3, 3.0)):
    """Bins of the bands that `base` leaves exactly zero, set next to the keep threshold the model gives them: the probes sit
    ~30 dB (quality 0.55) below their band's masking level, so they do not move any level, and whether they are kept says
    which level their band was given. base: [hops][ch][1024]."""
    m = psy_ref.model(base, sr, q)
    thr_keep = np.float64(np.float32(O.lib().flo_o_smr_threshold(float(q))))
    ath, band, _ = O.psy_tables(sr)
    out = base.copy()
    sl = psy_ref.band_slices(band)
    for h in range(base.shape[0]):
        for c in range(base.shape[1]):
            for b, (lo, hi) in enumerate(sl):
                if hi - lo < 2 or np.any(base[h, c, lo:hi] != 0):
                    continue
                ks = np.linspace(lo, hi - 1, min(len(offsets_db), hi - lo)).astype(int)
                for k, off in zip(ks, offsets_db):
                    if ath[k] >= m["level"][h, c, b]:      # the ATH decides here, a constant: a probe of that size would
                        continue                           # itself mask every band below it at full strength
                    t = m["level"][h, c, b] - 10.0 + thr_keep                         # dB a coefficient must exceed
                    if np.isfinite(t) and t + off < 370.0:
                        out[h, c, k] = _amp(t + off) * (1 if (k + h) % 2 else -1)
    return out


def _one_band(sr, j, level_db, nch=1, loud_ch=0, hops=2):
    """band j at a mean level of level_db (alternating signs), everything else exactly zero; hop 1 repeats hop 0 at half
    the amplitude (0.7 x the previous level then competes with the spread terms)"""
    _, band, _ = O.psy_tables(sr)
    lo, hi = psy_ref.band_slices(band)[j]
    c = np.zeros((hops, nch, 1024), np.float32)
    sign = np.where(np.arange(hi - lo) % 2 == 0, 1.0, -1.0).astype(np.float32)
    for h in range(hops):
        c[h, loud_ch, lo:hi] = _amp(level_db) * sign * np.float32(0.5 ** h)
    return c


def spectra_cases():
    """-> list of (name, coeffs [hops][ch][1024] f32, sample_rate, quality, needs_far): needs_far = the case must have a
    band whose level is set by a spread term of distance >= 9 (asserted from the model where the case is used)."""
    out = []
    sr = 44100
    # one loud band; L on both sides of 25 d - 100 (where the term passes the -100 dB floor) and of 25 d + 6 (where it
    # passes the level 0 dB every clip starts from, so that it is the term that sets band j + d's level)
    for d in range(1, 20):
        for side in (-0.5, 0.5):
            L = 25.0 * d - 100.0 + side
            out.append((f"floor_d{d}_{side:+}", _with_probes(_one_band(sr, 0, L), sr, 0.55), sr, 0.55, False))
    for d in range(1, 15):      # 25 d + 14 dB <= 364 dB: the f32 energy of band 0 (four or five bins) stays finite
        for side in (-0.5, 8.0):    # (+8 dB: the level the term sets then also clears the hearing threshold of band d's bins)
            L = 25.0 * d + 6.0 + side
            out.append((f"sets_d{d}_{side:+}", _with_probes(_one_band(sr, 0, L), sr, 0.55), sr, 0.55, d >= 9 and side > 0))
            out.append((f"sets_bare_d{d}_{side:+}", _one_band(sr, 0, L), sr, 0.55, False))
    # two bins in band 0 at 96 kHz: the largest level an f32 band energy holds (~382 dB), distances up to 15
    out.append(("sets_d15_96k", _with_probes(_one_band(96000, 0, 381.8), 96000, 0.55), 96000, 0.55, True))
    out.append(("loud_mid_band", _with_probes(_one_band(sr, 6, 300.0), sr, 0.55), sr, 0.55, True))
    for L in (98.5, 99.5, 105.9, 106.1):
        out.append((f"gmax_{L}", _with_probes(_one_band(sr, 3, L), sr, 0.55), sr, 0.55, False))
        out.append((f"gmax_{L}_q1", _with_probes(_one_band(sr, 3, L), sr, 1.0), sr, 1.0, False))
    # stereo, a loud band in one channel only: the other channel's probes sit at the thresholds of a silent channel
    for loud_ch in (0, 1):
        for L in (120.0, 260.0, 356.5):
            for j in (0, 2):
                out.append((f"stereo_loud{loud_ch}_band{j}_{L}", _with_probes(_one_band(sr, j, L, 2, loud_ch), sr, 0.55), sr, 0.55,
                            L >= 260.0))
    out.append(("stereo_loud_96k", _with_probes(_one_band(96000, 0, 381.8, 2, 1), 96000, 0.55), 96000, 0.55, True))
    # bands with a single non-zero bin, every band, both channels at different bins
    for sr_ in (44100, 384000):
        _, band, _ = O.psy_tables(sr_)
        c = np.zeros((3, 2, 1024), np.float32)
        for b, (lo, hi) in enumerate(psy_ref.band_slices(band)):
            if hi > lo:
                for h in range(3):
                    c[h, 0, lo + (h * 7) % (hi - lo)] = np.float32(0.01 * (b + 1) * (-1) ** b * 3.0 ** h)
                    c[h, 1, hi - 1 - (h * 5) % (hi - lo)] = np.float32(20.0 / (b + 1) * 0.3 ** h)
        for q in (0.55, 1.0):
            out.append((f"single_bin_bands_{sr_}_q{q}", c, sr_, q, False))
    # band maxima just above and just below 1e-10 (the scale factor's branch), quality 1.0 keeps such coefficients
    rng = np.random.default_rng(17)
    _, band, _ = O.psy_tables(sr)
    tiny = np.float32(1e-10)
    c = np.zeros((3, 2, 1024), np.float32)
    for b, (lo, hi) in enumerate(psy_ref.band_slices(band)):
        top = [np.nextafter(tiny, np.float32(1)), tiny, np.nextafter(tiny, np.float32(0)), np.float32(3e-10), np.float32(5e-9)][b % 5]
        for h in range(3):
            for ch in range(2):
                v = (rng.uniform(0.0, 1.0, hi - lo) * top).astype(np.float32) * rng.choice([-1, 1], hi - lo).astype(np.float32)
                v[rng.integers(0, hi - lo)] = top if ch == 0 else -top
                c[h, ch, lo:hi] = v
    for q in (1.0, 0.55):
        out.append((f"band_max_at_1e-10_q{q}", c, sr, q, False))
    return out


def nonfinite_cases():
    """-> list of (name, coeffs, sample_rate, quality): +-inf, NaN, 3e38, 1e19 and 2e19 (the square, or the sum of a few
    squares, overflows f32) in one band of ordinary spectra. O.lossy_quantize decides these."""
    sr = 44100
    base = O.lossy_analyze(signals.music_like(sr, 6000, 2, seed=23), sr, 2, 0.55)["coeffs"]
    _, band, _ = O.psy_tables(sr)
    sl = psy_ref.band_slices(band)
    out = []
    for name, vals in (("inf", [np.inf, -np.inf]), ("nan", [np.nan]), ("3e38", [3e38, -3e38]), ("1e19", [1e19] * 4),
                       ("2e19", [2e19, -2e19]), ("mixed", [np.nan, np.inf, 3e38, -1e19])):
        for b in (0, 7, 24):
            c = base.copy()
            lo, hi = sl[b]
            for i, v in enumerate(vals):
                c[2, i % 2, lo + i % (hi - lo)] = np.float32(v)        # hop 2: the frames behind it inherit the level
            for q in (0.55, 1.0):
                out.append((f"{name}_band{b}_q{q}", c, sr, q))
    return out
