"""Spectral similarity over fingerprint sets on the device (flo_fpindex_*, FingerprintIndex): every score bit for bit the
reference's (core/analysis.rs:395-437, restated in test_similarity_cpu.py), every ranking equal to a stable argsort of the
NumPy score matrix (score descending, index ascending), independent of the chunking; threshold pairs in (i, j) order."""
import ctypes as C

import numpy as np
import pytest

import flo_amd
import signals
from gpu_util import ctx  # noqa: F401
from test_similarity_cpu import np_score_matrix, rand_fps

pytestmark = pytest.mark.gpu

PAD = np.uint32(0xFFFFFFFF)


def expected_topk(S, k, self_join):
    """the ranking rule applied to a score matrix: stable argsort of -score, the diagonal left out of a self-join"""
    n_q, n_r = S.shape
    S = S.astype(np.float64)
    if self_join:
        S[np.arange(n_q), np.arange(n_q)] = -np.inf
    order = np.argsort(-S, axis=1, kind="stable")
    avail = n_r - 1 if self_join else n_r
    idx = np.full((n_q, k), PAD, np.uint32)
    sc = np.full((n_q, k), np.float32(-1.0), np.float32)
    m = min(k, avail)
    idx[:, :m] = order[:, :m]
    sc[:, :m] = np.take_along_axis(S, order[:, :m], 1).astype(np.float32)
    return idx, sc


def check(got, want):
    assert got[0].shape == want[0].shape
    bad = np.argwhere((got[0] != want[0]) | (got[1].view(np.uint32) != want[1].view(np.uint32)))
    assert bad.size == 0, (bad[:5], got[0][tuple(bad[0])], want[0][tuple(bad[0])])


def clustered(rng, n, centres=20, formats=((44100, 2),)):
    """fingerprints around a few centres (small byte distances: many near-ties), plus planted duplicates"""
    f = rand_fps(rng, n, formats=formats)
    c = rand_fps(rng, centres)
    pick = rng.integers(0, centres, n)
    for fld in ("energy_profile", "frequency_peaks", "avg_loudness"):
        f[fld] = np.clip(c[fld][pick].astype(np.int32) + rng.integers(-4, 5, f[fld].shape), 0, 255).astype(np.uint8)
    return f


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4097])
def test_topk_self_sizes(ctx, n):
    rng = np.random.default_rng(n)
    f = clustered(rng, n, formats=((44100, 2), (48000, 2)))
    if n > 8:
        f["hash"][n // 2] = f["hash"][1]                    # equal hashes, different bytes: 1.0
        f["energy_profile"][n // 3] = f["energy_profile"][2]  # equal bytes, different hashes
    S = np_score_matrix(f, f)
    ix = flo_amd.FingerprintIndex(f, ctx)
    for k in sorted({1, 10, 64, min(n + 2, 64)}):
        check(ix.topk_self(k), expected_topk(S, k, True))
    ix.close()


def test_results_do_not_depend_on_the_chunking(ctx, monkeypatch):
    rng = np.random.default_rng(5)
    f = clustered(rng, 3000)
    q = clustered(rng, 300)
    S, Q = np_score_matrix(f, f), np_score_matrix(q, f)
    ix = flo_amd.FingerprintIndex(f, ctx)
    for chunk in ("256", "768", "2048", ""):
        monkeypatch.setenv("FLO_FPINDEX_CHUNK_REFS", chunk)
        for k in (3, 16, 40):
            check(ix.topk_self(k), expected_topk(S, k, True))
            check(ix.topk(q, k), expected_topk(Q, k, False))
        i, j, s = ix.pairs(0.97)
        ii, jj = np.nonzero(np.triu(S >= np.float32(0.97), 1))
        assert np.array_equal(i, ii) and np.array_equal(j, jj) and np.array_equal(s.view(np.uint32), S[ii, jj].view(np.uint32))
    ix.close()


def test_few_queries_against_many_references(ctx):
    rng = np.random.default_rng(50)
    f = clustered(rng, 50_000, centres=50, formats=((44100, 2), (44100, 1)))
    q = f[[7, 123, 49_999]].copy()
    q["hash"][0] = rng.integers(0, 256, 32)                # a hash no member has
    q["hash"][2] = rng.integers(0, 256, 32)
    q["sample_rate"][2] = 8000                             # a format no member has: every member at 0.0
    Q = np_score_matrix(q, f)
    ix = flo_amd.FingerprintIndex(f, ctx)
    for k in (1, 10, 64):
        got = ix.topk(q, k)
        check(got, expected_topk(Q, k, False))
    assert got[0][1, 0] == 123 and got[1][1, 0] == 1.0        # the member itself
    assert np.all(got[1][2] == 0.0) and np.array_equal(got[0][2], np.arange(64))
    ix.close()


def test_adversarial_order_cases(ctx):
    """references whose energy distances to the query are permutations of each other: one SAD, different f32 sums"""
    rng = np.random.default_rng(9)
    m = 4000
    q = rand_fps(rng, 1)
    q["energy_profile"] = 100
    d = rng.integers(0, 120, 16)
    f = rand_fps(rng, m)
    f["energy_profile"] = 100 + rng.permuted(np.tile(d, (m, 1)), axis=1)
    f["frequency_peaks"], f["avg_loudness"] = q["frequency_peaks"], q["avg_loudness"]
    Q = np_score_matrix(q, f)
    assert len(np.unique(Q)) > 1                           # the sums do differ
    ix = flo_amd.FingerprintIndex(f, ctx)
    for k in (1, 10, 64):
        check(ix.topk(q, k), expected_topk(Q, k, False))
    S = np_score_matrix(f[:600], f[:600])
    ix2 = flo_amd.FingerprintIndex(f[:600], ctx)
    check(ix2.topk_self(20), expected_topk(S, 20, True))
    thr = np.float32(np.median(Q[0, :500]))
    ix3 = flo_amd.FingerprintIndex(np.concatenate([q, f[:500]]), ctx)
    i, j, s = ix3.pairs(float(thr))
    row = j[i == 0] - 1
    assert np.array_equal(row, np.nonzero(Q[0, :500] >= thr)[0])  # a bound too tight would drop some of them
    ix3.close()
    ix.close()
    ix2.close()


def test_exact_ties_in_index_order(ctx):
    rng = np.random.default_rng(2)
    n = 700
    f = rand_fps(rng, n)
    f["energy_profile"] = f["energy_profile"][0].copy()
    f["frequency_peaks"] = f["frequency_peaks"][0].copy()
    f["avg_loudness"] = 17
    f["energy_profile"][::3] = 3                           # two classes of identical profiles
    S = np_score_matrix(f, f)
    ix = flo_amd.FingerprintIndex(f, ctx)
    for k in (5, 33, 64):
        got = ix.topk_self(k)
        check(got, expected_topk(S, k, True))
    assert np.all(np.diff(got[0][5].astype(np.int64)) > 0)  # equal scores: ascending indices
    ix.close()


def test_pairs(ctx):
    rng = np.random.default_rng(300)
    f = clustered(rng, 300, centres=6, formats=((44100, 2), (22050, 1)))
    f["hash"][200] = f["hash"][10]
    f["hash"][250] = f["hash"][10]
    S = np_score_matrix(f, f)
    ix = flo_amd.FingerprintIndex(f, ctx)
    for thr in (1.0, 0.99, 0.95, 0.0):
        i, j, s = ix.pairs(thr)
        ii, jj = np.nonzero(np.triu(S >= np.float32(thr), 1))
        assert np.array_equal(i, ii) and np.array_equal(j, jj)
        assert np.array_equal(s.view(np.uint32), S[ii, jj].view(np.uint32))
    assert len(i) == 300 * 299 // 2                        # threshold 0: every pair, other formats at 0.0 included
    i1, j1, _ = ix.pairs(1.0)
    assert {(10, 200), (10, 250), (200, 250)} <= set(zip(i1.tolist(), j1.tolist()))
    # FLO_ERR_NOMEM with the exact count, nothing written; then the Python side's retry
    L = flo_amd._native.lib()
    n = C.c_uint64()
    small = np.zeros(10, np.uint32)
    rc = L.flo_fpindex_pairs(ix._h, 0.0, 10, small.ctypes.data, small.ctypes.data, small.ctypes.data, C.byref(n))
    assert rc == 3 and n.value == 44850 and not small.any()
    assert "44850" in L.flo_last_error(ctx._h).decode()
    ix._pair_cap = 7
    assert len(ix.pairs(0.0)[0]) == 44850 and ix._pair_cap == 44850
    with pytest.raises(flo_amd.FloError):
        ix.pairs(float("nan"))
    ix.close()


def test_arguments_and_empty_cases(ctx):
    rng = np.random.default_rng(1)
    f = rand_fps(rng, 10)
    ix = flo_amd.FingerprintIndex(f, ctx)
    with pytest.raises(flo_amd.FloError, match="64"):
        ix.topk_self(65)
    with pytest.raises(flo_amd.FloError):
        ix.topk(f[:2], 65)
    assert ix.topk_self(0)[0].shape == (10, 0) and ix.topk(f[:0], 5)[0].shape == (0, 5)
    empty = flo_amd.FingerprintIndex(f[:0], ctx)
    idx, sc = empty.topk(f[:3], 4)
    assert np.all(idx == PAD) and np.all(sc == -1.0)
    assert empty.topk_self(4)[0].shape == (0, 4) and len(empty.pairs(0.0)[0]) == 0
    one = flo_amd.FingerprintIndex(f[:1], ctx)
    idx, sc = one.topk_self(3)
    assert np.all(idx == PAD) and np.all(sc == -1.0) and len(one.pairs(0.0)[0]) == 0
    for x in (ix, empty, one):
        x.close()


def test_fingerprints_of_a_real_batch_find_each_other(ctx):
    sr, ch, n = 44100, 2, 3 * 44100
    clips = [signals.music_like(sr, n, ch, seed=s) for s in range(6)]
    clips.append(clips[2].copy())                          # one clip twice
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSLESS, [c.size for c in clips], sr, ch, 5)
    for i, c in enumerate(clips):
        b.upload(i, c)
    b.sync()
    an = b.analyze_all()
    b.close()
    ix = flo_amd.FingerprintIndex(an, ctx)
    idx, sc = ix.topk_self(3)
    assert idx[2, 0] == 6 and idx[6, 0] == 2 and sc[2, 0] == 1.0 and sc[6, 0] == 1.0
    fa = flo_amd.fingerprint_array(an)
    check((idx, sc), expected_topk(np_score_matrix(fa, fa), 3, True))
    i, j, s = ix.pairs(1.0)
    assert list(zip(i.tolist(), j.tolist())) == [(2, 6)]
    ix.close()


def test_cli_similar(ctx, tmp_path, capsys):
    from flo_amd import cli
    sr, ch = 44100, 2
    a, b = signals.music_like(sr, 2 * sr, ch, seed=1), signals.music_like(sr, 2 * sr, ch, seed=2)
    paths = []
    for name, pcm in (("a.flo", a), ("b.flo", b), ("a2.flo", a)):
        p = tmp_path / name
        p.write_bytes(flo_amd.encode(pcm, sr, ch, 16))
        paths.append(str(p))
    assert cli.main(["similar", *paths, "-k", "1"]) == 0
    out = capsys.readouterr().out.splitlines()
    assert out[0] == paths[0] and out[1] == f"  1.000000  {paths[2]}"
    assert out[4] == paths[2] and out[5] == f"  1.000000  {paths[0]}"
    assert cli.main(["similar", *paths, "--threshold", "1.0"]) == 0
    out = capsys.readouterr().out.splitlines()
    assert out == ["Pairs with similarity >= 1.0: 1", f"  1.000000  {paths[0]}  {paths[2]}"]


def test_large_index_sampled_rows(ctx):
    rng = np.random.default_rng(60_000)
    n = 60_000
    f = clustered(rng, n, centres=400, formats=((44100, 2), (48000, 2)))
    f["hash"][rng.integers(0, n, 50)] = f["hash"][rng.integers(0, n, 50)]
    ix = flo_amd.FingerprintIndex(f, ctx)
    idx, sc = ix.topk_self(10)
    rows = np.sort(rng.choice(n, 200, replace=False))
    S = np_score_matrix(f[rows], f)
    S[np.arange(200), rows] = -np.inf
    want = expected_topk(S, 10, False)
    check((idx[rows], sc[rows]), want)
    i, j, s = ix.pairs(0.99)
    for r_, row in zip(rows[:50], S[:50]):
        jj = np.nonzero(row >= np.float32(0.99))[0]
        jj = jj[jj > r_]
        sel = i == r_
        assert np.array_equal(j[sel], jj) and np.array_equal(s[sel].view(np.uint32), row[jj].astype(np.float32).view(np.uint32))
    assert np.all(np.diff(i.astype(np.int64)) >= 0)
    ix.close()
