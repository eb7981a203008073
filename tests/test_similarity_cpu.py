"""spectral_similarity (core/analysis.rs:395-437) and extract_dominant_frequencies (analysis.rs:367-387) on the host: a
NumPy restatement of the reference's score with explicit f32 steps, checked against the reference's own cases, against
flo_amd.spectral_similarity bit for bit, and against the error bound the device filter relies on
(flo_amd/csrc/similarity_kernels.hpp); fingerprints read back from files' META. No GPU needed."""
import os

import numpy as np
import pytest

import flo_amd
import signals
from conftest import EXAMPLES
from oracle import oracle as O

F32 = np.float32
U = 2.0 ** -24
# the reference's term 1.0 - |a - b| / 255.0 for every byte distance: correctly rounded division, then the subtraction
TERM = (F32(1.0) - np.arange(256, dtype=np.float32) / F32(255.0)).astype(np.float32)


def rand_fps(rng, n, formats=((44100, 2),), hash_pool=None):
    """n random fingerprints (FINGERPRINT_DTYPE), distinct hashes unless drawn from hash_pool"""
    f = np.zeros(n, flo_amd.FINGERPRINT_DTYPE)
    if hash_pool is None:
        f["hash"] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        f["hash"][:, :4] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)   # distinct
    else:
        f["hash"] = hash_pool[rng.integers(0, len(hash_pool), n)]
    fm = np.array(formats)[rng.integers(0, len(formats), n)]
    f["sample_rate"], f["channels"] = fm[:, 0], fm[:, 1]
    f["avg_loudness"] = rng.integers(0, 256, n)
    f["frequency_peaks"] = rng.integers(0, 256, (n, 8))
    f["energy_profile"] = rng.integers(0, 256, (n, 16))
    return f


def np_scores(a, b):
    """the reference's f32 score of the pairs (a[p], b[p]) (arrays of equal length), step by step in its order"""
    ea, eb = a["energy_profile"].astype(np.int32), b["energy_profile"].astype(np.int32)
    pa, pb = a["frequency_peaks"].astype(np.int32), b["frequency_peaks"].astype(np.int32)
    e = np.zeros(len(a), np.float32)
    for k in range(16):   # Iterator::sum: a left fold in index order
        e = (e + TERM[np.abs(ea[:, k] - eb[:, k])]).astype(np.float32)
    p = np.zeros(len(a), np.float32)
    for k in range(8):
        p = (p + TERM[np.abs(pa[:, k] - pb[:, k])]).astype(np.float32)
    lo = TERM[np.abs(a["avg_loudness"].astype(np.int32) - b["avg_loudness"].astype(np.int32))]
    e = (e / F32(16.0)).astype(np.float32)
    p = (p / F32(8.0)).astype(np.float32)
    x = (e * F32(0.5)).astype(np.float32)
    y = (p * F32(0.3)).astype(np.float32)
    z = (lo * F32(0.2)).astype(np.float32)
    s = ((x + y).astype(np.float32) + z).astype(np.float32)
    same_fmt = (a["sample_rate"] == b["sample_rate"]) & (a["channels"] == b["channels"])
    s = np.where(same_fmt, s, F32(0.0)).astype(np.float32)
    same_hash = np.all(a["hash"] == b["hash"], axis=1)
    return np.where(same_hash, F32(1.0), s).astype(np.float32)


def np_score_matrix(q, r, rows_per_block=64):
    """scores [len(q), len(r)]"""
    out = np.empty((len(q), len(r)), np.float32)
    for s in range(0, len(q), rows_per_block):
        qq = q[s:s + rows_per_block]
        out[s:s + len(qq)] = np_scores(np.repeat(qq, len(r)), np.tile(r, len(qq))).reshape(len(qq), len(r))
    return out


def bound_key(a, b):
    """K = 5 SAD_e + 6 SAD_p + 32 D_l of the device filter"""
    se = np.abs(a["energy_profile"].astype(np.int64) - b["energy_profile"]).sum(1)
    sp = np.abs(a["frequency_peaks"].astype(np.int64) - b["frequency_peaks"]).sum(1)
    dl = np.abs(a["avg_loudness"].astype(np.int64) - b["avg_loudness"])
    return 5 * se + 6 * sp + 32 * dl


def device_bound(key):
    """fp_bound of similarity_kernels.hpp in f32"""
    c = F32(1.0) / F32(40800.0)
    r = (F32(1.0) - (key.astype(np.float32) * c).astype(np.float32)).astype(np.float32)
    return (r + F32(2.0 ** -17)).astype(np.float32)


def _fp(d):
    return flo_amd.fingerprint_array(d)[0]


# ---- the reference's own cases (spectral_analysis_tests.rs:80-130, 160-190) -------------------------------------------
def test_reference_similarity_cases():
    s = np.array([0.5, -0.3, 0.8, -0.2, 0.1, -0.9], np.float32)
    f1, f2 = O.spectral_fingerprint(s, 1, 44100), O.spectral_fingerprint(s, 1, 44100)
    assert flo_amd.spectral_similarity(f1, f2) == F32(1.0)                       # identical: the hash matches
    c = np.full(100, 0.5, np.float32)
    m1, m2 = O.spectral_fingerprint(c, 1, 44100), O.spectral_fingerprint(c, 2, 44100)
    assert flo_amd.spectral_similarity(m1, m2) == F32(0.0)                       # channel mismatch
    i = np.arange(1000, dtype=np.float32)
    d1 = O.spectral_fingerprint(np.sin(i * F32(0.01)).astype(np.float32), 1, 44100)
    d2 = O.spectral_fingerprint(np.sin(i * F32(0.05)).astype(np.float32), 1, 44100)
    assert d1["hash"] != d2["hash"]
    v = flo_amd.spectral_similarity(d1, d2)
    assert 0.0 <= v <= 1.0
    a, b = flo_amd.fingerprint_array([d1]), flo_amd.fingerprint_array([d2])
    assert v.view(np.uint32) == np_scores(a, b)[0].view(np.uint32)
    for x, y in ((f1, f2), (m1, m2)):
        assert np_scores(flo_amd.fingerprint_array([x]), flo_amd.fingerprint_array([y]))[0] == flo_amd.spectral_similarity(x, y)


def test_reference_dominant_frequency_cases():
    s = np.array([0.5, -0.3, 0.8, -0.2, 0.1, -0.9], np.float32)
    fp = O.spectral_fingerprint(s, 1, 44100)
    for n in range(1, 9):
        d = flo_amd.extract_dominant_frequencies(fp, n)
        assert len(d) == 1 and len(d[0]) == n
        assert all(0.0 <= f <= 22050.0 for f in d[0])
    assert len(flo_amd.extract_dominant_frequencies(fp, 16)[0]) == 8               # capped at 8 bands
    fp2 = O.spectral_fingerprint(np.full(2000, 0.5, np.float32), 1, 44100)
    assert all(0.0 <= f <= 22050.0 for f in flo_amd.extract_dominant_frequencies(fp2, 3)[0])
    # the mapping itself, in f64 as the reference writes it
    f = dict(fp, frequency_peaks=[0, 1, 17, 128, 200, 254, 255, 3], sample_rate=48000)
    assert flo_amd.extract_dominant_frequencies(f, 8)[0] == [p / 255.0 * (48000 / 2.0) for p in f["frequency_peaks"]]
    assert flo_amd.extract_dominant_frequencies(f, 0) == [[]]


# ---- the restatement against the library, bit for bit -----------------------------------------------------------------
def test_host_score_bit_exact_on_random_pairs():
    rng = np.random.default_rng(7)
    n = 100_000
    pool = rng.integers(0, 256, (50, 32), dtype=np.uint8)
    a = rand_fps(rng, n, formats=((44100, 2), (44100, 1), (48000, 2)), hash_pool=pool)
    b = rand_fps(rng, n, formats=((44100, 2), (44100, 1), (48000, 2)), hash_pool=pool)
    # a third of the pairs close to each other (small byte distances), where the f32 rounding matters most
    close = rng.random(n) < 0.33
    for f in ("energy_profile", "frequency_peaks"):
        near = np.clip(a[f].astype(np.int32) + rng.integers(-3, 4, a[f].shape), 0, 255).astype(np.uint8)
        b[f][close] = near[close]
    want = np_scores(a, b)
    lib = flo_amd._native.lib()
    fpp = flo_amd._native.C.POINTER(flo_amd._native.Fingerprint)
    pa, pb = a.ctypes.data, b.ctypes.data
    sz = a.dtype.itemsize
    got = np.array([lib.flo_spectral_similarity(flo_amd._native.C.cast(pa + i * sz, fpp),
                                                flo_amd._native.C.cast(pb + i * sz, fpp)) for i in range(n)], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (want == 1.0).sum() > 100 and (want == 0.0).sum() > 1000                 # both early returns exercised
    # symmetric bit for bit
    assert np.array_equal(np_scores(b, a).view(np.uint32), want.view(np.uint32))


def test_term_table_needs_the_correctly_rounded_division():
    d = np.arange(256, dtype=np.float32)
    recip = (F32(1.0) - d * (F32(1.0) / F32(255.0))).astype(np.float32)
    assert (recip.view(np.uint32) != TERM.view(np.uint32)).sum() > 0
    exact = np.array([np.float32(1.0 - float(np.float32(k / 255.0))) for k in range(256)], np.float32)
    assert np.array_equal(exact.view(np.uint32), TERM.view(np.uint32))


def test_sum_order_matters():
    """a reordered sum is not the score: permuted distance vectors give different f32 results"""
    rng = np.random.default_rng(3)
    n = 20000
    d = rng.integers(0, 256, (n, 16))
    dp = np.take_along_axis(d, rng.permuted(np.tile(np.arange(16), (n, 1)), axis=1), 1)
    s1, s2 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for k in range(16):
        s1 = (s1 + TERM[d[:, k]]).astype(np.float32)
        s2 = (s2 + TERM[dp[:, k]]).astype(np.float32)
    assert (s1 != s2).sum() > 1000


# ---- the device filter's bound (similarity_kernels.hpp) ---------------------------------------------------------------
def test_filter_bound_holds():
    rng = np.random.default_rng(11)
    n = 400_000
    a = rand_fps(rng, n)
    b = rand_fps(rng, n)
    close = rng.random(n) < 0.5
    for f in ("energy_profile", "frequency_peaks", "avg_loudness"):
        near = np.clip(a[f].astype(np.int32) + rng.integers(-2, 3, a[f].shape), 0, 255).astype(np.uint8)
        b[f][close] = near[close]
    # permutations of one distance vector: same K, different f32 sums
    m = 20000
    base = rng.integers(0, 256, 16)
    perm = rng.permuted(np.tile(base, (m, 1)), axis=1)
    a2, b2 = rand_fps(rng, m), rand_fps(rng, m)
    a2["energy_profile"] = 0
    b2["energy_profile"] = perm
    b2["frequency_peaks"], b2["avg_loudness"] = a2["frequency_peaks"], a2["avg_loudness"]
    a, b = np.concatenate([a, a2]), np.concatenate([b, b2])
    s = np_scores(a, b).astype(np.float64)
    key = bound_key(a, b)
    r = 1.0 - key / 40800.0
    assert np.abs(s - r).max() <= 11 * U                                           # the claim of the proof
    ub = device_bound(key)
    assert np.all(s <= ub.astype(np.float64))                                      # never filters out a candidate
    assert np.all(ub.astype(np.float64) - r <= 132 * U)                            # ...and rejects every larger K
    assert len(np.unique(s[-m:])) > 1 and len(np.unique(key[-m:])) == 1


# ---- fingerprints from files ---------------------------------------------------------------------------------------------
def test_fingerprints_from_files(tmp_path):
    clips = [(signals.music_like(44100, 30000, 2, seed=s), 44100, 2) for s in (1, 2)]
    clips.append((signals.music_like(22050, 20000, 1, seed=3), 22050, 1))
    paths, blobs = [], []
    for n, (pcm, sr, ch) in enumerate(clips):
        flo = O.encode_lossless(pcm, sr, ch, meta=O.analysis_metadata(pcm, sr, ch))
        p = tmp_path / f"c{n}.flo"
        p.write_bytes(flo)
        paths.append(str(p))
        blobs.append(flo)
    got = flo_amd.fingerprints_from_files(paths)
    assert got.dtype == flo_amd.FINGERPRINT_DTYPE and got.size == 3
    for g, (pcm, sr, ch) in zip(got, clips):
        want = O.spectral_fingerprint(pcm, ch, sr)
        assert bytes(g["hash"]) == want["hash"] and int(g["duration_ms"]) == want["duration_ms"]
        assert int(g["sample_rate"]) == sr and int(g["channels"]) == ch and int(g["avg_loudness"]) == want["avg_loudness"]
        assert list(g["frequency_peaks"]) == want["frequency_peaks"] and list(g["energy_profile"]) == want["energy_profile"]
    assert np.array_equal(flo_amd.fingerprints_from_files(blobs), got)              # bytes work as well as paths
    assert flo_amd.spectral_similarity(got[0], got[0]) == 1.0
    assert flo_amd.spectral_similarity(got[0], got[2]) == 0.0                       # other format


def test_file_without_fingerprint_names_the_file(tmp_path):
    ex = os.path.join(EXAMPLES, "sine_440hz_mono.flo")   # written by the reference CLI: no analysis fields in its META
    with pytest.raises(flo_amd.FloError, match="sine_440hz_mono.flo"):
        flo_amd.fingerprints_from_files([ex])
    bad = tmp_path / "garbage.flo"
    bad.write_bytes(b"not a flo file at all")
    with pytest.raises(flo_amd.FloError, match="garbage.flo"):
        flo_amd.fingerprints_from_files([str(bad)])


def test_fingerprint_inputs():
    fp = O.spectral_fingerprint(signals.music_like(44100, 5000, 2, seed=9), 2, 44100)
    a = flo_amd.fingerprint_array(fp)
    assert a.size == 1 and bytes(a[0]["hash"]) == fp["hash"]
    assert np.array_equal(flo_amd.fingerprint_array(a), a)
    assert np.array_equal(flo_amd.fingerprint_array([fp, fp]), np.concatenate([a, a]))
    with pytest.raises(flo_amd.FloError):
        flo_amd.fingerprint_array(dict(fp, energy_profile=[0] * 15))
    with pytest.raises(flo_amd.FloError):
        flo_amd.fingerprint_array(np.zeros(3, [("x", "u1")]))
