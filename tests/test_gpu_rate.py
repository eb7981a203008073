"""Size curves and the rate-targeted lossy encode on the device (flo_batch_size_curve, flo_batch_set_quality,
flo_encode_batch_to_size and their Python / CLI faces). The yardstick of the curve is exact: the length of the file the
device's own encode produces at that quality. Against the oracle the project's bound for device-against-oracle DATA sizes
holds (0.5 % + 8 bytes, test_gpu_lossy.py), and the selection is tested at budgets that lie outside that tolerance."""
import ctypes as C
import json
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import flo_amd
import flofile
import lossy_cases
import signals
from conftest import ROOT, example_bytes
from flo_amd import cli
from gpu_util import ctx  # noqa: F401
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GRID = list(flo_amd.DEFAULT_RATE_GRID)
GRID_X = GRID + [0.99, 0.9899]          # both sides of the exact-threshold switch at quality 0.99
GRID16 = [i / 16 for i in range(16)]


def _batch(ctx, clips, sr, ch, q=0.5):
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [c.size for c in clips], sr, ch, q)
    for i, c in enumerate(clips):
        b.upload(i, c)
    return b


def _curve(ctx, clips, sr, ch, grid, q=0.5):
    b = _batch(ctx, clips, sr, ch, q)
    try:
        return b.size_curve(grid)
    finally:
        b.close()


def _own_sizes(ctx, clips, sr, ch, grid):
    return np.array([[len(ctx.encode_lossy(c, sr, ch, q)) for q in grid] for c in clips], np.uint64)


def _same(curve, own, tag):
    bad = np.argwhere(curve != own)
    assert bad.size == 0, (tag, [(int(i), int(j), int(curve[i, j]), int(own[i, j])) for i, j in bad[:8]])


# ---------------------------------------------------------------------------------------------- 1. the encoder's own size
def _ragged_stereo():
    lens = [0, 1, 1023, 1024, 5000, 44100, 70001, 3 * 1024]
    return [signals.music_like(44100, n, 2, seed=40 + i) for i, n in enumerate(lens)], 44100, 2


def _mono_edges():
    return [signals.music_like(44100, n, 1, seed=60 + i) for i, n in enumerate([0, 1, 1025, 4097])], 44100, 1


def _many_short():
    # 70 clips of one to three frames: more clips than kFewClips
    return [signals.music_like(44100, 1 + (37 * i) % 2000, 2, seed=200 + i) for i in range(70)], 44100, 2


EXACT_CASES = {
    "ragged_stereo": _ragged_stereo,
    "mono_edges": _mono_edges,
    "ch3": lambda: ([signals.music_like(44100, 12000, 3, seed=73)], 44100, 3),
    "ch8": lambda: ([signals.music_like(44100, 12000, 8, seed=78)], 44100, 8),
    "rate8000": lambda: ([signals.music_like(8000, 20000, 2, seed=8000)], 8000, 2),
    "rate96000": lambda: ([signals.music_like(96000, 20000, 2, seed=96000)], 96000, 2),
    "rate384000": lambda: ([signals.music_like(384000, 20000, 2, seed=384000)], 384000, 2),
    "many_short": _many_short,
}


@pytest.mark.parametrize("case", list(EXACT_CASES))
def test_curve_is_the_encoders_own_size(ctx, case):
    clips, sr, ch = EXACT_CASES[case]()
    curve = _curve(ctx, clips, sr, ch, GRID_X)
    assert curve.shape == (len(clips), len(GRID_X)) and curve.dtype == np.uint64
    _same(curve, _own_sizes(ctx, clips, sr, ch, GRID_X), case)


# ---------------------------------------------------------------------------------------------- 2. sparse-size branches
def _vectors(ctx, pcm, sr, ch, q):
    """the device's own integers, one row of 1024 per (frame, channel)"""
    return ctx.lossy_analyze(pcm, sr, ch, q)["q"].reshape(-1, 1024)


def _longest_run(rows, of_nonzero):
    best = 0
    for r in rows:
        m = (r != 0) if of_nonzero else (r == 0)
        edges = np.flatnonzero(np.diff(np.concatenate(([0], m.astype(np.int8), [0]))))
        if edges.size:
            best = max(best, int((edges[1::2] - edges[0::2]).max()))
    return best


def _pcm_case(name):
    for n, pcm, sr, ch, q in lossy_cases.pcm_cases():
        if n == name:
            return pcm, sr, ch, q
    raise KeyError(name)


def test_all_zero_vectors_are_three_bytes_at_every_candidate(ctx):
    pcm = np.zeros(5000 * 2, np.float32)
    assert not _vectors(ctx, pcm, 44100, 2, 1.0).any()
    curve = _curve(ctx, [pcm], 44100, 2, GRID_X)
    hops = (5000 + 1024 + 1023) // 1024
    assert (curve == 74 + 20 * hops + hops * (12 + 54 * 2 + 2 * 3)).all()
    _same(curve, _own_sizes(ctx, [pcm], 44100, 2, GRID_X), "zeros")


def test_non_zero_runs_beyond_255(ctx):
    pcm = signals.fast_noise(6000 * 2, 5, 1.0)
    assert _longest_run(_vectors(ctx, pcm, 44100, 2, 1.0), True) > 255      # the 255-cap continuation records
    _same(_curve(ctx, [pcm], 44100, 2, GRID_X), _own_sizes(ctx, [pcm], 44100, 2, GRID_X), "noise")
    mono = signals.fast_noise(6000, 6, 1.0)
    assert _longest_run(_vectors(ctx, mono, 44100, 1, 1.0), True) > 255
    _same(_curve(ctx, [mono], 44100, 1, GRID_X), _own_sizes(ctx, [mono], 44100, 1, GRID_X), "noise mono")


def test_zero_runs_of_128_and_more_across_lanes(ctx):
    for ch in (1, 2):
        pcm = signals.sine(440.0, 44100, 9000, 0.5, ch)
        rows = _vectors(ctx, pcm, 44100, ch, 0.5)
        assert rows.any() and _longest_run(rows[rows.any(axis=1)], False) >= 128     # inside vectors that hold non-zeros
        _same(_curve(ctx, [pcm], 44100, ch, GRID_X), _own_sizes(ctx, [pcm], 44100, ch, GRID_X), f"sine ch{ch}")


@pytest.mark.parametrize("name, there_for", [("square_full_scale", "two_caps"), ("impulse", "tiny"), ("level_x1e-8_q1.0", "kept_tiny"),
                                             ("fade_to_zero_q1.0", "tiny")])
def test_dense_vectors_and_coefficients_at_or_below_1e_minus_10(ctx, name, there_for):
    """What each case is there for, measured with the oracle on the CPU and asserted here from the device's own integers:
    the square wave's vectors are non-zero over runs of 777 (two 255-cap continuations in one run); the impulse and the fade
    hold whole frames of exact zeros next to dense ones (|c| <= 1e-10 with nothing to keep); at 1e-8 of full scale quality
    1.0 KEEPS coefficients of |c| <= 1e-10 (736 of 2722 in the oracle), which only the dB expression of the exact-threshold
    branch does."""
    pcm, sr, ch, _ = _pcm_case(name)
    a = ctx.lossy_analyze(pcm, sr, ch, 1.0)
    tiny = np.abs(a["coeffs"]) <= 1e-10
    if there_for == "two_caps":
        assert _longest_run(a["q"].reshape(-1, 1024), True) > 2 * 255
    else:
        assert tiny.any()
    if there_for == "kept_tiny":
        assert (a["q"][tiny] != 0).any()
    grid = [1.0, 0.99, 0.9899, 0.5, 0.0]
    _same(_curve(ctx, [pcm], sr, ch, grid), _own_sizes(ctx, [pcm], sr, ch, grid), name)


def test_nan_and_inf_in_the_pcm(ctx):
    x = signals.fast_noise(8192, 2)
    x[100], x[2000], x[3001] = np.nan, np.inf, -np.inf
    for ch in (1, 2):
        _same(_curve(ctx, [x], 44100, ch, GRID_X), _own_sizes(ctx, [x], 44100, ch, GRID_X), f"nan/inf ch{ch}")


# ---------------------------------------------------------------------------------------------- 3. independence
def test_the_batchs_own_quality_plays_no_part(ctx):
    clips, sr, ch = _ragged_stereo()
    clips = clips[2:6]
    assert np.array_equal(_curve(ctx, clips, sr, ch, GRID, q=0.1), _curve(ctx, clips, sr, ch, GRID, q=0.9))


def _results(b):
    import torch
    n = b.data_bytes()
    files = [b.fetch(i) for i in range(b.n_clips)]
    buf = torch.zeros(sum(len(f) + 16 for f in files) + 64, dtype=torch.uint8, device="cuda:0")
    offs = b.pack_files(buf.data_ptr(), buf.numel())
    b.sync()
    packed = buf.cpu().numpy().tobytes()
    pcm = torch.zeros(sum(flofile.parse(f).total_samples for f in files) * b.channels + 64, dtype=torch.float32, device="cuda:0")
    poffs = b.decode_to(pcm.data_ptr(), pcm.numel())
    b.sync()
    return n, files, offs, packed, poffs, pcm.cpu().numpy().tobytes()


def test_curve_leaves_an_encoded_batch_alone_and_encode_after_curve_is_fresh(ctx):
    clips, sr, ch = _ragged_stereo()
    clips = clips[1:7]
    a, b = _batch(ctx, clips, sr, ch, 0.55), _batch(ctx, clips, sr, ch, 0.55)
    try:
        for x in (a, b):
            x.encode(0)
            x.sync()
        curve = b.size_curve(GRID)           # behind encode + sync: fetch, sizes, packed files and decode stay as they were
        assert _results(a) == _results(b)
        assert _results(b)[1] == [ctx.encode_lossy(c, sr, ch, 0.55) for c in clips]
        b.encode(0)                          # and an encode behind the curve gives the files of a batch that never ran it
        b.sync()
        assert _results(a) == _results(b)
        assert np.array_equal(b.size_curve(GRID), curve)
    finally:
        a.close()
        b.close()


def test_candidate_order_duplicates_and_counts(ctx):
    clips, sr, ch = _ragged_stereo()
    clips = clips[3:6]
    base = _curve(ctx, clips, sr, ch, GRID)
    col = {q: base[:, j] for j, q in enumerate(GRID)}
    perm = [GRID[j] for j in (5, 16, 0, 5, 9, 9, 1, 16, 12)]
    got = _curve(ctx, clips, sr, ch, perm)
    for j, q in enumerate(perm):
        assert np.array_equal(got[:, j], col[q]), (j, q)
    one = _curve(ctx, clips, sr, ch, [0.4375])
    assert one.shape == (3, 1) and np.array_equal(one[:, 0], col[0.4375])
    g32 = [(i % 17) / 16 for i in range(32)]
    many = _curve(ctx, clips, sr, ch, g32)
    assert many.shape == (3, 32)
    for j, q in enumerate(g32):
        assert np.array_equal(many[:, j], col[q]), (j, q)


_CHILD = r"""
import json, sys
sys.path[:0] = [%r, %r]
import flo_amd, signals
lens = [700, 5000, 44100, 3072, 9000, 1, 20000]
clips = [signals.music_like(44100, n, 2, seed=300 + i) for i, n in enumerate(lens)]
grid = [i / 16 for i in range(17)]
ctx = flo_amd.Context(0)
b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [c.size for c in clips], 44100, 2, 0.5)
for i, c in enumerate(clips):
    b.upload(i, c)
ctx.profile_enable(True)
ctx.profile_reset()
out = b.size_curve(grid)
_, launches = ctx.profile_query("size_curve")
print(json.dumps({"launches": int(launches), "curve": out.tolist()}))
b.close()
ctx.close()
"""


def test_groups_of_clips_give_the_same_array(ctx):
    # 7 clips of 2, 6, 45, 4, 10, 2 and 21 frames; a frame takes 3 buffers x 2 channels x 128 bytes of scratch, so 20 KiB
    # hold 26 frames: four groups, one of them a single clip larger than the limit
    env = dict(os.environ, FLO_SIZE_CURVE_GROUP_BYTES=str(20 * 1024))
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["launches"] >= 3
    lens = [700, 5000, 44100, 3072, 9000, 1, 20000]
    clips = [signals.music_like(44100, n, 2, seed=300 + i) for i, n in enumerate(lens)]
    ctx.profile_enable(True)
    ctx.profile_reset()
    whole = _curve(ctx, clips, 44100, 2, GRID)
    _, launches = ctx.profile_query("size_curve")
    ctx.profile_enable(False)
    assert launches == 1
    assert np.array_equal(np.array(res["curve"], np.uint64), whole)


# ---------------------------------------------------------------------------------------------- 4, 5. against the oracle
ORACLE_CLIPS = [("stereo_44100", 44100, 2, 12000, 5), ("mono_44100", 44100, 1, 3000, 6), ("stereo_48000", 48000, 2, 9000, 7)]
_oracle_cache = {}


def _oracle_case(name):
    if name not in _oracle_cache:
        _, sr, ch, n, seed = next(c for c in ORACLE_CLIPS if c[0] == name)
        pcm = signals.music_like(sr, n, ch, seed=seed)
        files = [O.encode_lossy(pcm, sr, ch, q) for q in GRID16]
        _oracle_cache[name] = (pcm, sr, ch, [len(f) for f in files], [flofile.parse(f).data_size for f in files])
    return _oracle_cache[name]


@pytest.mark.parametrize("name", [c[0] for c in ORACLE_CLIPS])
def test_curve_against_the_oracle(ctx, name):
    pcm, sr, ch, o_file, o_data = _oracle_case(name)
    assert all(b > a for a, b in zip(o_file, o_file[1:])), o_file          # the oracle's sizes grow over the grid
    curve = _curve(ctx, [pcm], sr, ch, GRID16)[0]
    hops = (pcm.size // ch + 1024 + 1023) // 1024
    for j, q in enumerate(GRID16):
        data = int(curve[j]) - 74 - 20 * hops
        print(f"{name} q={q}: curve DATA {data}, oracle DATA {o_data[j]}")
        assert abs(data - o_data[j]) <= 0.005 * o_data[j] + 8, (name, q, data, o_data[j])


@pytest.mark.parametrize("name", [c[0] for c in ORACLE_CLIPS])
def test_selection_lands_where_the_oracle_says(ctx, name):
    pcm, sr, ch, o_file, o_data = _oracle_case(name)
    # precondition, from the oracle's numbers alone: every gap is wider than twice the device-oracle tolerance, so the
    # midpoint lies outside it on both sides and the lower candidate is the only right answer
    for j in range(15):
        gap = o_file[j + 1] - o_file[j]
        assert gap > 2 * (0.005 * o_data[j + 1] + 8), (name, j, gap)
    budgets = [(o_file[j] + o_file[j + 1]) // 2 for j in range(15)]
    files, chosen, fits = ctx.encode_batch_to_size([pcm] * 15, sr, ch, GRID16, budgets)
    assert chosen == list(range(15)) and all(fits), (chosen, fits)
    for j in range(15):
        assert len(files[j]) <= budgets[j] and files[j] == ctx.encode_lossy(pcm, sr, ch, GRID16[j])
    # the Python route: analysis META is merged, so the budget for the audio is the target minus that META
    meta_len = len(flofile.parse(flo_amd.encode_to_bitrate(pcm, sr, ch, 10 ** 6, GRID16)).meta)
    frames = pcm.size // ch
    kbps = [Fraction((b + meta_len) * sr, 125 * frames) for b in budgets]
    _, infos = flo_amd.encode_to_bitrate_many([pcm] * 15, sr, ch, kbps, GRID16, with_info=True)
    assert [i["target_bytes"] for i in infos] == [b + meta_len for b in budgets]
    assert [i["index"] for i in infos] == list(range(15)) and all(i["fits"] for i in infos)


# ---------------------------------------------------------------------------------------------- 6. end to end
def _level(q):
    return min(4, int(math.floor(4 * q + 0.5)))


def test_rate_targeted_encode_end_to_end(ctx):
    sr, ch = 44100, 2
    lens = [3000, 1, 1023, 1024, 5000, 44100, 30001, 3 * 1024, 12000]
    clips = [signals.music_like(sr, n, ch, seed=500 + i) for i, n in enumerate(lens)]
    curve = _curve(ctx, clips, sr, ch, GRID)
    # clip 3's META is as long as the step from its wanted candidate (8) to the next larger size on the grid
    step = next(int(curve[3, j]) - int(curve[3, 8]) for j in range(9, 17) if curve[3, j] > curve[3, 8])
    metas = [b"", b"\x81\xa5title\xa3abc", b"", b"x" * step, b"", b"", b"\x80", b"", b""]
    order = sorted(range(len(GRID)), key=lambda j: GRID[j])
    # targets: exactly the size at a wanted candidate (META included), one below the smallest file, one far above the largest
    want = [2, None, 5, 8, 11, 14, 7, "max", 3]
    targets = []
    for i, w in enumerate(want):
        if w is None:
            targets.append(int(curve[i].min()) + len(metas[i]) - 1)
        elif w == "max":
            targets.append(int(curve[i].max()) + len(metas[i]) + 10 ** 6)
        else:
            targets.append(int(curve[i, w]) + len(metas[i]))
    files, chosen, fits = ctx.encode_batch_to_size(clips, sr, ch, GRID, targets, metas)
    assert fits == [w is not None for w in want]
    assert chosen[1] == 0 and chosen[7] == 16
    assert len(set(chosen)) >= 4, chosen
    for i, f in enumerate(files):
        q = GRID[chosen[i]]
        assert f == ctx.encode_lossy(clips[i], sr, ch, q, metas[i]), i
        p = flofile.parse(f)
        assert p.crc_valid and p.is_lossy and p.lossy_quality == _level(q) and p.meta == metas[i]
        if fits[i]:
            assert len(f) <= targets[i] and len(f) == int(curve[i, chosen[i]]) + len(metas[i])
            # a candidate of larger quality value that also fitted would have been the choice
            budget = targets[i] - len(metas[i])
            assert all(int(curve[i, j]) > budget for j in order if GRID[j] > q), i
        else:
            assert all(int(curve[i, j]) + len(metas[i]) > targets[i] for j in range(len(GRID)))
        dec = ctx.decode(f)
        assert dec.size == (len(p.frames) - 1) * 1024 * ch and np.isfinite(dec).all()
    # with META given its length counts against the target: the same target without that META reaches a higher quality
    plain, chosen2, _ = ctx.encode_batch_to_size([clips[3]], sr, ch, GRID, [targets[3]])
    assert GRID[chosen2[0]] > GRID[chosen[3]] and len(plain[0]) <= targets[3]

    # the Python route (analysis META merged): kbps per clip, the batch call against the one-clip call
    kbps = [64, 96, 128, 200, 32, 1, 500, 160, 80]
    many, infos = flo_amd.encode_to_bitrate_many(clips, sr, ch, kbps, metadata=metas, with_info=True)
    for i, (f, info) in enumerate(zip(many, infos)):
        p = flofile.parse(f)
        target = kbps[i] * 125 * lens[i] // sr
        assert info["target_bytes"] == target and info["file_bytes"] == len(f) and info["quality"] == GRID[info["index"]]
        assert f == ctx.encode_lossy(clips[i], sr, ch, info["quality"], p.meta), i
        assert p.lossy_quality == _level(info["quality"]) and len(p.meta) >= len(metas[i])
        budget = target - len(p.meta)
        if info["fits"]:
            assert len(f) <= target
            assert all(int(curve[i, j]) > budget for j in order if GRID[j] > info["quality"]), i
        else:
            assert info["index"] == 0 and all(int(curve[i, j]) > budget for j in range(len(GRID)))
    assert not infos[5]["fits"] and infos[6]["fits"]
    for i in (0, 4, 8):
        one, info = flo_amd.encode_to_bitrate(clips[i], sr, ch, kbps[i], metadata=metas[i], with_info=True)
        assert one == many[i] and info == infos[i]
    assert flo_amd.encode_to_bitrate_many([], sr, ch, 128) == []
    assert np.array_equal(flo_amd.size_curve(clips[4], sr, ch), curve[4])


# ---------------------------------------------------------------------------------------------- 7. misuse
def test_misuse_is_reported_and_the_context_stays_usable(ctx):
    L = ctx._L
    q = np.array(GRID, np.float32)
    out = np.zeros(64, np.uint64)
    pcm = signals.music_like(44100, 3000, 2, seed=9)
    ll = flo_amd.Batch(ctx, flo_amd.MODE_LOSSLESS, [pcm.size], 44100, 2, 5)
    ll.upload(0, pcm)
    assert L.flo_batch_size_curve(ll._h, 4, q.ctypes.data, out.ctypes.data) == 1           # FLO_ERR_ARG
    assert L.flo_batch_set_quality(ll._h, 0.5) == 1
    ll.close()
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [pcm.size], 44100, 2, 0.5)
    assert L.flo_batch_size_curve(b._h, 4, q.ctypes.data, out.ctypes.data) == 4            # FLO_ERR_STATE: nothing uploaded
    with pytest.raises(flo_amd.FloError):
        b.size_curve(GRID)
    b.upload(0, pcm)
    assert L.flo_batch_size_curve(b._h, 0, q.ctypes.data, out.ctypes.data) == 1
    assert L.flo_batch_size_curve(b._h, 33, q.ctypes.data, out.ctypes.data) == 1
    assert L.flo_batch_size_curve(b._h, 4, q.ctypes.data, None) == 1
    assert L.flo_batch_size_curve(b._h, 4, None, out.ctypes.data) == 1
    assert L.flo_batch_size_curve(None, 4, q.ctypes.data, out.ctypes.data) == 1
    assert L.flo_batch_set_quality(None, 0.5) == 1
    ptrs, lens = (C.c_void_p * 1)(pcm.ctypes.data), (C.c_size_t * 1)(pcm.size)
    outs, olens = (C.c_void_p * 1)(), (C.c_size_t * 1)()
    tb, ch_, ft = np.array([10 ** 6], np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.int32)
    args = lambda nq, o: (ctx._h, 1, ptrs, lens, 44100, 2, nq, q.ctypes.data, tb.ctypes.data, None, None, o, olens, ch_.ctypes.data, ft.ctypes.data)
    assert L.flo_encode_batch_to_size(*args(0, outs)) == 1
    assert L.flo_encode_batch_to_size(*args(33, outs)) == 1
    assert L.flo_encode_batch_to_size(*args(4, None)) == 1
    with pytest.raises(flo_amd.FloError):
        ctx.encode_batch_to_size([signals.music_like(44100, 100, 9, seed=1)], 44100, 9, GRID, [1000])     # 9 channels
    # everything still works
    assert np.array_equal(b.size_curve(GRID)[0], _own_sizes(ctx, [pcm], 44100, 2, GRID)[0])
    b.set_quality(0.25)
    b.encode(0)
    b.sync()
    assert b.fetch(0) == ctx.encode_lossy(pcm, 44100, 2, 0.25)
    b.close()


# ---------------------------------------------------------------------------------------------- 8. CLI
def test_cli_target_kbps_and_curve(tmp_path, capsys, ctx):
    wav = tmp_path / "audio.wav"
    wav.write_bytes(example_bytes("audio.wav"))
    out = tmp_path / "t.flo"
    assert cli.main(["encode", str(wav), str(out), "--lossy", "--target-kbps", "96"]) == 0
    text = capsys.readouterr().out
    assert "Quality:" in text and "Achieved:" in text
    got = out.read_bytes()
    p = flofile.parse(got)
    assert p.crc_valid and p.is_lossy and len(got) <= 96 * 125 * 44100 // 44100
    assert ctx.decode(got).size == (len(p.frames) - 1) * 1024 * 2
    assert cli.main(["curve", str(wav), "--json"]) == 0
    rows = json.loads(capsys.readouterr().out)
    from flo_amd.wav import read_wav_bytes
    samples, sr, ch = read_wav_bytes(wav.read_bytes())
    sizes = flo_amd.size_curve(samples, sr, ch)
    assert len(rows) == len(GRID) and [r["bytes"] for r in rows] == [int(s) for s in sizes]
    assert [r["quality"] for r in rows] == GRID
    assert cli.main(["curve", str(wav)]) == 0 and "quality" in capsys.readouterr().out
