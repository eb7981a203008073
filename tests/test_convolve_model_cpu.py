"""tests/convolve_model.py held to three independent references on CPU: a scalar restatement of the definition in rational
arithmetic, rounded once per FMA; np.convolve in f64 within the bound resample_model.dot_reference derives; and
tests/mix_model.py, whose K-part mix of one clip at gains h[k] and offsets at = k is the same chain of FMAs. Then the table of
named paths: every name is reached by the cases the device tests run (tests/test_gpu_convolve.py asserts the same of each of
its batches)."""
from fractions import Fraction

import numpy as np
import pytest

import convolve_model as M
import mix_model

F32 = np.float32


def _round_f32(q):
    """the f32 nearest to the rational q, ties to even; +0.0 for 0 (the sum of +0.0 and a zero product of either sign)"""
    if q == 0:
        return F32(0.0)
    sign, a = (-1 if q < 0 else 1), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    e = max(e, -126)                    # subnormals share the exponent of the smallest normal
    scaled = a / Fraction(2) ** (e - 23)
    n = scaled.numerator // scaled.denominator
    rest = scaled - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n & 1):
        n += 1
    with np.errstate(over="ignore"):
        return F32(sign * float(Fraction(n) * Fraction(2) ** (e - 23)))   # exact in f64; beyond FLT_MAX it rounds to infinity


def _scalar(x, ch, h, ir_ch, g):
    """the definition, sample by sample, every FMA exact and rounded once (finite values only)"""
    N, P = x.size // ch, h.size // ir_ch
    K = M.taps_of(g["taps"], P, g["ir_start"])
    out = np.zeros((g["frames"], ch), F32)
    for t in range(g["frames"]):
        for c in range(ch):
            a = F32(0.0)
            for k in range(K):
                m = t + g["skip"] - k
                xv = x[m * ch + c] if 0 <= m < N else F32(0.0)
                hv = h[(g["ir_start"] + k) * ir_ch + (0 if ir_ch == 1 else c)]
                a = _round_f32(Fraction(float(hv)) * Fraction(float(xv)) + Fraction(float(a)))
            out[t, c] = a
    return out.reshape(-1)


def _random_case(rng):
    ch = int(rng.integers(1, 4))
    ir_ch = ch if rng.integers(2) else 1
    N, P = int(rng.integers(0, 9)), int(rng.integers(0, 7))
    scale = F32(10.0) ** rng.integers(-3, 4)
    x = (rng.standard_normal(N * ch) * scale).astype(F32)
    h = rng.standard_normal(P * ir_ch).astype(F32)
    if N and rng.integers(3) == 0:
        x[rng.integers(x.size)] = F32(rng.choice([0.0, -0.0, 2.0 ** -140, -2.0 ** -127, 3e38]))
    if P and rng.integers(3) == 0:
        h[rng.integers(h.size)] = F32(rng.choice([0.0, -0.0, 2.0 ** -20, 1.0, -1.0]))
    g = M.job(0, 0, int(rng.integers(0, 12)), skip=int(rng.integers(0, 12)), ir_start=int(rng.integers(0, 8)),
              taps=int(rng.choice([0, 1, 2, 5, M.ALL])))
    return x, ch, h, ir_ch, g


def test_the_model_equals_the_rational_restatement():
    rng = np.random.default_rng(2024)
    seen_sub = 0
    for i in range(400):
        x, ch, h, ir_ch, g = _random_case(rng)
        got, sub = M.convolve_clip(x, ch, h, ir_ch, g)
        want = _scalar(x, ch, h, ir_ch, g)
        assert M.same(got, want) is None, (i, g, x, h, M.same(got, want))
        seen_sub += sub
    assert seen_sub > 0   # the planted denormals were reported


def test_the_model_reports_subnormals():
    x = np.array([1.0, 2.0 ** -100], F32)
    assert M.convolve_clip(x, 1, np.array([1.0], F32), 1, M.job(0, 0, 2))[1] is False
    assert M.convolve_clip(x, 1, np.array([2.0 ** -40], F32), 1, M.job(0, 0, 2))[1] is True            # a product
    assert M.convolve_clip(np.array([1.0, -1.0], F32), 1, np.array([2.0 ** -126, 2.0 ** -127 + 2.0 ** -126], F32), 1, M.job(0, 0, 2))[1] is True
    with pytest.raises(AssertionError):
        M.convolve([x], 1, [np.array([2.0 ** -40], F32)], 1, [M.job(0, 0, 2)], strict=True)


@pytest.mark.parametrize("ch,ir_ch", [(1, 1), (2, 1), (2, 2), (3, 3)])
def test_the_model_lies_within_the_bound_of_the_f64_convolution(ch, ir_ch):
    """|y - np.convolve| <= (K + 1) 2^-24 sum |h x| + K 2^-126: resample_model.dot_reference's bound for K products and
    K - 1 additions in f32 in any order"""
    rng = np.random.default_rng(7 + ch)
    N, P = 700, 130
    x, h = rng.standard_normal(N * ch).astype(F32), (rng.standard_normal(P * ir_ch) * 0.3).astype(F32)
    for g in (M.mode_job("full", N, P), M.mode_job("centered", N, P), M.job(0, 0, 300, skip=40, ir_start=5, taps=77)):
        K = M.taps_of(g["taps"], P, g["ir_start"])
        got, _ = M.convolve_clip(x, ch, h, ir_ch, g)
        got = got.reshape(-1, ch).astype(np.float64)
        X, H = x.reshape(N, ch).astype(np.float64), h.reshape(P, ir_ch).astype(np.float64)[g["ir_start"]:g["ir_start"] + K]
        for c in range(ch):
            hc = H[:, 0 if ir_ch == 1 else c]
            full, mag = np.convolve(X[:, c], hc), np.convolve(np.abs(X[:, c]), np.abs(hc))
            pad = np.zeros(g["skip"] + g["frames"])
            ref, bound = pad.copy(), pad.copy()
            ref[:full.size], bound[:full.size] = full[:pad.size], mag[:pad.size]
            ref, bound = ref[g["skip"]:], (K + 1) * 2.0 ** -24 * bound[g["skip"]:] + K * 2.0 ** -126
            assert (np.abs(got[:, c] - ref) <= bound).all(), (g, c)


def test_an_fir_is_a_mix_of_shifted_copies():
    """for finite taps an FIR of K taps equals, bit for bit, the mix of K parts of the same clip at gains h[k] and offsets
    at = k in list order: each live part adds fma(h[k], x[t - k], a), and a part that is not live on a frame is a tap
    against +0.0, which leaves a finite sum unchanged (fma(h, +0, a) = a for a != 0, and +0 for a = +0, since a chain that
    starts at +0.0 never reaches -0.0). It holds at both ends of the clip, with `skip` as the mix's start offset"""
    rng = np.random.default_rng(11)
    for ch, N, K, skip, T in ((1, 50, 7, 0, 56), (2, 40, 9, 0, 40), (2, 40, 9, 4, 40), (3, 10, 25, 12, 30), (2, 300, 64, 31, 300), (1, 5, 3, 9, 4)):
        x = rng.standard_normal(N * ch).astype(F32)
        h = (rng.standard_normal(K) * 0.5).astype(F32)
        h[rng.integers(K)] = F32(-0.0)
        got, _ = M.convolve_clip(x, ch, h, 1, M.job(0, 0, T, skip=skip))
        # output t = sum_k h[k] x[t + skip - k]: part k lays source frames from max(skip - k, 0) on at max(k - skip, 0)
        parts = [mix_model.part(0, 0, 0, max(skip - k, 0), N, max(k - skip, 0), float(h[k])) for k in range(K)]
        want = mix_model.mix_clip([[x]], ch, parts, T)
        assert M.same(got, want) is None, (ch, N, K, skip, T, M.same(got, want))


def test_non_finite_taps_and_the_identity():
    x = np.array([1.0, -0.0, -2.0, np.inf, 0.5, 3.0], F32)
    one, _ = M.convolve_clip(x, 2, np.array([1.0], F32), 1, M.job(0, 0, 3))
    assert M.same(one, np.array([1.0, 0.0, -2.0, np.inf, 0.5, 3.0], F32)) is None          # -0.0 becomes +0.0
    y, _ = M.convolve_clip(x, 2, np.array([0.5, np.nan, 0.25, 2.0], F32), 2, M.job(0, 0, 5))
    assert np.isnan(y.reshape(5, 2)[:, 1]).all() and np.isfinite(y.reshape(5, 2)[[0, 2, 3, 4], 0]).all()   # a NaN tap: its whole channel
    y, _ = M.convolve_clip(x, 2, np.array([0.5, np.inf, 0.25, 2.0], F32), 2, M.job(0, 0, 5))
    # an infinite tap: NaN where it meets a zero (the -0.0 of frame 0, every frame outside the clip), an infinity elsewhere
    assert np.isnan(y.reshape(5, 2)[[0, 3, 4], 1]).all() and np.isposinf(y.reshape(5, 2)[[1, 2], 1]).all()
    z, _ = M.convolve_clip(x, 2, np.array([0.5], F32), 1, M.job(0, 0, 4, ir_start=1))
    assert z.size == 8 and not z.view(np.uint32).any()                                      # K == 0: +0.0 everywhere


def test_every_named_path_is_reached_by_the_device_cases():
    assert len(set(M.PATHS)) == len(M.PATHS)
    reached = set()
    for ch, ir_ch in ((1, 1), (2, 1), (2, 2), (3, 1), (3, 3), (8, 1), (8, 8)):
        src, irs, jobs = M.device_case(ch, ir_ch)
        got = M.case_paths(src, irs, jobs, ch, ir_ch)
        assert got >= M.expected_paths(ch, ir_ch), (ch, ir_ch, sorted(M.expected_paths(ch, ir_ch) - got))
        assert max(x.size // ch for x in src) <= 3 * M.TILE + 5 and M.work(src, irs, jobs, ch, ir_ch) < 2e8
        assert M.refusal([x.size // ch for x in src], ch, [h.size // ir_ch for h in irs], ir_ch, jobs) is None
        reached |= got
    g = M.job(0, 0, 5)
    assert "irs is src" not in reached and M.paths(g, 9, 9, 2, 2) <= set(M.PATHS)   # (tests/test_gpu_convolve.py::test_a_batch_as_its_own_response)
    assert reached | {"irs is src"} == set(M.PATHS)
