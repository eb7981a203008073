"""The model of loudness normalisation (tests/normalize_model.py) against brute-force restatements of its sliding stages and of
the kernel's own decomposition, and the properties of the limiter and of the gain on the model's output. The GPU tests
(tests/test_gpu_normalize.py) hold the device to the model bit for bit, so what holds here holds there. No GPU needed."""
import math

import numpy as np
import pytest

import normalize_model as M
from oracle import oracle as O

C1 = M.ceiling(-1.0)
# |z| = fl(|y| s 2^-24) with s 2^-24 <= fl(C / p) <= (C / p) (1 + 2^-24) and |y| <= p: at most C (1 + 2^-24)^2
ROUNDING = 1.0 + 2.0 ** -22

# What the model measured on the signals below (A = 72, C = -1 dBTP; gains of 1, 2 and 4; printed by the tests), in dB of the
# output's oversampled peak over the ceiling: white noise 0.02318 / 0.02318 / 0.02318, fs/4 sine at 45 degrees 0.00837 /
# 0.02088 / 0.02088, burst 0.01780 / 0.01780 / 0.01780, single click 0 / 0 / 0, square wave 0.00010 / 0.00010 / 0.00010.
# The bound is twice the worst of them.
OVERSHOOT_WORST_DB = 0.02318
OVERSHOOT_BOUND_DB = 2 * OVERSHOOT_WORST_DB
# |L(fl32(x g)) - (L(x) + 20 log10 g)| in LU over the clips below: the worst the model measured is 1.80e-9; four times that
LOUDNESS_WORST_LU = 1.80e-9
LOUDNESS_BOUND_LU = 4 * LOUDNESS_WORST_LU


# ---- the sliding stages ----------------------------------------------------------------------------------------------------
def _brute(r, A):
    n = r.size
    at = lambda j: int(r[j]) if 0 <= j < n else M.UNITY
    m = {k: min(at(j) for j in range(k - A, k + A + 1)) for k in range(-A, n + A)}
    s = [sum(m[k] for k in range(i - A, i + A + 1)) // (2 * A + 1) for i in range(n)]
    return np.array([m[k] for k in range(-A, n + A)], np.uint32), np.array(s, np.uint32)


@pytest.mark.parametrize("A", [1, 2, 5, 12])
def test_sliding_stages_match_brute_force(A):
    rng = np.random.default_rng(A)
    for n in (1, 2, A, 2 * A, 2 * A + 1, 4 * A + 3, 97):
        for dense in (0.05, 0.5, 1.0):
            r = np.where(rng.uniform(size=n) < dense, rng.integers(0, M.UNITY, n), M.UNITY).astype(np.uint32)
            m = M.sliding_min(r, A)
            s = (M.sliding_sum(m, A) // (2 * A + 1)).astype(np.uint32)
            bm, bs = _brute(r, A)
            assert np.array_equal(m, bm) and np.array_equal(s, bs), (A, n, dense)
            assert (s <= r).all()


def _kernel_tile(r_clip, A, tile):
    """s of one tile the way norm_limit_kernel makes it: r over F + 4A frames, the minimum by doubling, the inclusive prefix
    sums of m's 12-bit halves, S from two differences"""
    F, lr, lm, w = M.tile_frames(A), M.r_len(A), M.m_len(A), 2 * A + 1
    n, r0 = r_clip.size, tile * F - 2 * A
    idx = np.arange(r0, r0 + lr)
    a = np.where((idx >= 0) & (idx < n), r_clip[np.clip(idx, 0, max(n - 1, 0))], M.UNITY).astype(np.uint32)
    pw = 1
    while 2 * pw <= w:
        pw *= 2
    j = 1
    while j < pw:
        a = np.minimum(a, np.concatenate([a[j:], np.full(j, M.UNITY, np.uint32)]))
        j *= 2
    m = np.minimum(a[:lm], a[w - pw:w - pw + lm])
    hi, lo = np.cumsum(m >> 12, dtype=np.uint32), np.cumsum(m & 4095, dtype=np.uint32)
    nf = min(F, n - tile * F)
    jj = np.arange(nf)
    before = lambda p: np.where(jj > 0, p[np.maximum(jj - 1, 0)], 0).astype(np.uint32)
    S = (hi[jj + 2 * A] - before(hi)).astype(np.uint64) * np.uint64(4096) + (lo[jj + 2 * A] - before(lo)).astype(np.uint64)
    return (S // np.uint64(w)).astype(np.uint32)


@pytest.mark.parametrize("A", [1, 12, 72, 576, 1024])
def test_the_kernels_decomposition_is_the_definition(A):
    rng = np.random.default_rng(100 + A)
    F = M.tile_frames(A)
    for n in (1, 4 * A + 63, F - 1, F + 1, 2 * F + 5):
        r = np.where(rng.uniform(size=n) < 0.02, rng.integers(0, M.UNITY, n), M.UNITY).astype(np.uint32)
        r[[0, n - 1, min(n - 1, F - 1), min(n - 1, F)]] = [5, 7, 11, 13][:4]
        want = (M.sliding_sum(M.sliding_min(r, A), A) // (2 * A + 1)).astype(np.uint32)
        got = np.concatenate([_kernel_tile(r, A, t) for t in range(-(-n // F))])
        assert np.array_equal(got, want), (A, n)


# ---- the cases of the GPU tests --------------------------------------------------------------------------------------------
def _measured(x, ch, rate):
    m = O.loudness_metrics(x[:x.size // ch * ch], ch, rate) if x.size >= ch else dict(integrated_lufs=-23.0, sample_peak_dbfs=-150.0)
    return m["integrated_lufs"], m["sample_peak_dbfs"]


def _subnormal(a):
    b = np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return bool(((b - np.uint32(1)) < np.uint32(0x007FFFFF)).any())


@pytest.mark.parametrize("case", M.cases(), ids=lambda c: c["name"])
def test_cases_have_no_subnormal_and_s_stays_below_r(case):
    """the bits must not depend on whether the device flushes subnormals: no partial sum of an envelope (of x for the true
    peak, of y for the limiter), no y and no output is a non-zero subnormal; and s[n] <= r[n] on every frame"""
    ch, A, C = case["ch"], case["A"], M.ceiling(case["ceiling"])
    for name, x in case["clips"]:
        lufs, peak = _measured(x, ch, case["rate"])
        if np.isfinite(x).all():
            assert not M.peaks(x, ch)[1], (name, "true peak")
        out, rep, sub = M.normalize(x, ch, case["rate"], lufs, peak, case["target"], case["ceiling"], case["mode"], case["lookahead_frames"],
                                    case["max_gain_db"])
        assert not sub, (name, "limiter")
        if rep["status"]:
            assert np.array_equal(out.view(np.uint32), x[:out.size].view(np.uint32))
            continue
        y = (x[:out.size] * rep["gain"]).astype(np.float32)
        assert not _subnormal(y) and not _subnormal(out), name
        if case["mode"] == M.LIMIT:
            _, s, r, _, _ = M.limit(y, ch, A, C)
            assert (s <= r).all() and int((s < M.UNITY).sum()) == rep["limited_frames"]
            assert (np.abs(out) <= float(C) * ROUNDING).all(), name


@pytest.mark.parametrize("rate,ch", M.RESAMPLER_SHAPES)
def test_resampler_clips_have_no_subnormal(rate, ch):
    """the clips of test_true_peaks_are_the_resampler_at_four_times_the_rate: no partial sum of their envelope is a non-zero
    subnormal either (the envelope IS the conversion to four times the rate, so this covers both sides of that test)"""
    for x in M.resampler_clips(rate, ch):
        assert not M.peaks(x, ch)[1] and not _subnormal(x)


def test_the_cases_reach_what_they_are_there_for():
    by = {c["name"]: c for c in M.cases()}
    sk = by["skip_bound"]
    A, C = sk["A"], M.ceiling(sk["ceiling"])
    clips = dict(sk["clips"])
    assert M.tile_skips(clips["meets"], 2, A, C, 0) and M.tile_skips(clips["meets"], 2, A, C, 1)
    assert not M.tile_skips(clips["misses"], 2, A, C, 0) and not M.tile_skips(clips["misses"], 2, A, C, 1)
    assert not M.tile_skips(clips["misses_in_halo"], 2, A, C, 0) and not M.tile_skips(clips["misses_in_halo"], 2, A, C, 1)
    assert M.tile_skips(clips["meets_beyond_halo"], 2, A, C, 0) and not M.tile_skips(clips["meets_beyond_halo"], 2, A, C, 1)
    # a clip that misses the bound by an ulp is still not limited: the bound is not tight
    for name in ("misses", "misses_in_halo"):
        assert M.normalize(clips[name], 2, 48000, -23.0, -1.0, -23.0, -1.0, M.LIMIT)[1]["limited_frames"] == 0
    assert M.normalize(clips["meets_beyond_halo"], 2, 48000, -23.0, -1.0, -23.0, -1.0, M.LIMIT)[1]["limited_frames"] == 4 * A + 1
    sine = dict(by["dc_and_sine"]["clips"])["fs4_sine_45deg"]
    inner = M.peaks(sine, 2)[0].view(np.float32)[100:-100]   # (the clip's cut ends ring higher)
    assert abs(float(np.abs(sine).max()) - math.sqrt(0.5)) < 1e-6 and abs(float(inner.max()) - 1.0) < 2e-3
    assert {c["A"] for c in M.cases()} >= {1, 12, 72, 576, 1024} and {c["rate"] for c in M.cases()} >= {8000, 48000, 384000}
    assert {c["ch"] for c in M.cases()} >= {1, 2, 3, 6} and max(len(c["clips"]) for c in M.cases()) >= 64
    got = {x.size // c["ch"] for c in M.cases() if c["name"].startswith("lengths") for _, x in c["clips"]}
    assert got == set(M.lengths(72))
    for c in M.cases():
        for _, x in c["clips"]:
            assert x.size // c["ch"] <= 3 * M.tile_frames(c["A"]) + 5


# ---- the skip bound --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", range(4))
def test_skip_bound_holds_on_the_adversarial_clips(q):
    """y[k] = a sign(h[q][k - n + 31]) drives |e_q[n]| to a times the row's l1 norm: still at most fl32(a B), so a tile that
    passes the test fl32(max |y| * B) <= C has no p above C; at the clip's edges too, where the window is cut"""
    h, B = M.table(), M.skip_bound()
    n_frames = 200
    worst = 0.0
    for a in (np.float32(float(C1) / float(B)), np.float32(1.0), np.float32(0.3), np.float32(1e-3), np.float32(3.7)):
        for n in (0, 1, 30, 31, 32, 33, 100, n_frames - 34, n_frames - 33, n_frames - 32, n_frames - 1):
            y = np.full(n_frames, a, np.float32)
            k = np.arange(64) + n - 31
            ok = (k >= 0) & (k < n_frames)
            y[k[ok]] = np.where(h[q][ok] < 0, -a, a)
            pb, sub = M.peaks(y, 1)
            assert not sub
            p = float(pb.view(np.float32).max())
            assert p <= float(np.float32(a * B)), (q, float(a), n, p)
            worst = max(worst, p / (float(a) * float(B)))
    print("row %d: the largest p over a B is %.7f" % (q, worst))
    assert worst <= 1.0 and (q != 2 or worst > 0.9999)   # row 2 has the largest norm: the bound is nearly met there


# ---- properties ------------------------------------------------------------------------------------------------------------
A48 = 72
N_PROP = 3 * 2048 + 77


def _signals():
    rng = np.random.default_rng(7)
    k = np.arange(N_PROP)
    burst = np.zeros(N_PROP, np.float32)
    burst[2000:2600] = rng.uniform(-1.0, 1.0, 600).astype(np.float32)
    click = np.zeros(N_PROP, np.float32)
    click[3000] = 1.0
    return [("white noise", rng.uniform(-1.0, 1.0, N_PROP).astype(np.float32)),
            ("fs/4 sine at 45 degrees", np.sin(np.pi / 2 * k + np.pi / 4).astype(np.float32)),
            ("burst", burst), ("single click", click),
            ("square wave", np.where((k // 24) % 2 == 0, 0.9, -0.9).astype(np.float32))]


@pytest.mark.parametrize("gain", [1.0, 2.0, 4.0])
def test_limit_mode_overshoot(gain):
    """the oversampled peak of z passes C only through the modulation of the gain (every sample of z is at or below C but for two roundings,
    and so is every envelope value of y * s[n] taken with the s of its own frame)"""
    for name, x in _signals():
        y = (x * np.float32(gain)).astype(np.float32)
        z, s, r, _, sub = M.limit(y, 1, A48, C1)
        assert not sub and (s <= r).all() and (np.abs(z) <= float(C1) * ROUNDING).all()
        tp = float(M.true_peak(z, 1))
        over = 20.0 * math.log10(tp / float(C1)) if tp > float(C1) else 0.0
        print("%s at a gain of %g: true peak of the output %.6f, %.5f dB over the ceiling, %d frames limited" % (name, gain, tp, over, int((s < M.UNITY).sum())))
        assert over <= OVERSHOOT_BOUND_DB, (name, gain, over)
        if name == "single click":
            # one frame above the ceiling is limited over 4A + 1 frames; at the higher gains the sub-sample positions a quarter
            # of a frame in front of the click pass the ceiling too, and they belong to the frame before it
            lim = np.flatnonzero(s < M.UNITY)
            first = 3000 - 2 * A48 - (gain > 1.0)
            assert lim.size == 3000 + 2 * A48 - first + 1 and lim[0] == first and lim[-1] == 3000 + 2 * A48


def test_gain_mode_loudness():
    """GAIN mode is linear but for one rounding per sample: the integrated loudness of the output against that of the exact
    product, L(x) + 20 log10 g. K-weighting and the relative gate scale with the signal; the absolute gate at -70 LUFS does
    not, so the clips keep every 400 ms block further than |gain| + 1 LU from it."""
    sr, ch = 48000, 2
    rng = np.random.default_rng(11)
    n = sr * 2
    t = np.arange(n) / sr
    clips = [("noise at 0.1", rng.uniform(-0.1, 0.1, n * ch).astype(np.float32)),
             ("tone and noise", (np.repeat(0.3 * np.sin(2 * np.pi * 997.0 * t), ch) + rng.uniform(-0.01, 0.01, n * ch)).astype(np.float32)),
             ("loud noise", rng.uniform(-0.9, 0.9, n * ch).astype(np.float32))]
    worst = 0.0
    for name, x in clips:
        m = O.loudness_metrics(x, ch, sr)
        for target in (-14.0, -23.0, -30.0):
            out, rep, _ = M.normalize(x, ch, sr, m["integrated_lufs"], m["sample_peak_dbfs"], target, -1.0, M.GAIN)
            blocks = -0.691 + 10.0 * np.log10(O.block_energies(x, ch, sr))
            assert (np.abs(blocks + 70.0) > abs(rep["gain_db"]) + 1.0).all(), name
            got = O.integrated_lufs(out, ch, sr)
            d = abs(got - (m["integrated_lufs"] + rep["gain_db"]))
            print("%s to %g LUFS: gain %+.3f dB, output at %.6f LUFS, off the exact product by %.2e LU" % (name, target, rep["gain_db"], got, d))
            worst = max(worst, d)
            assert d <= LOUDNESS_BOUND_LU, (name, target, d)
    print("worst %.2e LU" % worst)


def test_gain_mode_peak():
    """the ceiling in GAIN mode: the true peak of the output is at most C (1 + 2^-22). The plan keeps tp g at or below
    C (1 - 2^-15): y is within 2^-24 relative of x g and each of the two chains within 2^-18 of sum |h x|, which is at most
    2.2525 tp, so the output's own peak is at most tp g (1 + 2.2525 (2^-17 + 2^-23)) < C"""
    worst = 0.0
    n_capped = 0
    for c in M.cases():
        if c["mode"] != M.GAIN:
            continue
        C = M.ceiling(c["ceiling"])
        for name, x in c["clips"]:
            lufs, peak = _measured(x, c["ch"], c["rate"])
            out, rep, _ = M.normalize(x, c["ch"], c["rate"], lufs, peak, c["target"], c["ceiling"], M.GAIN, 0, c["max_gain_db"])
            if rep["status"]:
                continue
            n_capped += rep["ceiling_reduction_db"] > 0
            tp = float(M.true_peak(out, c["ch"]))
            worst = max(worst, tp / float(C))
            assert tp <= float(C) * (1.0 + 2.0 ** -22), (name, tp)
    print("the largest true peak of a GAIN-mode output over C: %.9f; %d clips held by the ceiling" % (worst, n_capped))
    assert n_capped >= 5
