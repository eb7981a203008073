"""Quality ladders on the device (flo_batch_encode_ladder, flo_ladder_*, flo_encode_batch_ladder and their Python / CLI
faces): every clip of a batch as a finished file at each of K qualities, from one transform pass. The criterion throughout
is byte equality with the project's own single-quality encoder (ctx.encode_lossy), which test_gpu_lossy.py pins to the
oracle and the reference; no tolerance appears anywhere."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import flo_amd
import flofile
import lossy_cases
import signals
from conftest import ROOT, example_bytes
from flo_amd import cli
from gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

GRID = list(flo_amd.DEFAULT_RATE_GRID)
GRID_X = GRID + [0.99, 0.9899]          # 19 rungs, both sides of the exact-threshold switch at quality 0.99, 1.0 included
LADDER5 = [0.0, 0.5, 0.9899, 0.99, 1.0]
ERR_ARG, ERR_STATE = 1, 4


def _batch(ctx, clips, sr, ch, q=0.5):
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [c.size for c in clips], sr, ch, q)
    for i, c in enumerate(clips):
        b.upload(i, c)
    return b


def _ladder_files(ctx, clips, sr, ch, rungs, q=0.5):
    """(files[clip][rung], file_bytes, size_curve of the same batch)"""
    b = _batch(ctx, clips, sr, ch, q)
    try:
        with b.encode_ladder(rungs) as lad:
            assert (lad.n_clips, lad.n_rungs) == (len(clips), len(rungs))
            files = [[lad.fetch(i, j) for j in range(len(rungs))] for i in range(len(clips))]
            return files, lad.file_bytes.copy(), b.size_curve(rungs)
    finally:
        b.close()


def _check(ctx, clips, sr, ch, rungs, tag):
    files, sizes, curve = _ladder_files(ctx, clips, sr, ch, rungs)
    assert sizes.shape == (len(clips), len(rungs)) and sizes.dtype == np.uint64
    for i, c in enumerate(clips):
        for j, q in enumerate(rungs):
            own = ctx.encode_lossy(c, sr, ch, q)
            assert files[i][j] == own, (tag, "clip", i, "rung", j, q, len(files[i][j]), len(own))
            assert int(sizes[i, j]) == len(own), (tag, i, j)
    assert np.array_equal(sizes, curve), tag
    return files


# ---------------------------------------------------------------------------------------------- 1. every rung is the encoder's file
def _ragged_stereo():
    lens = [0, 1, 1023, 1024, 5000, 44100, 70001, 3 * 1024]
    return [signals.music_like(44100, n, 2, seed=40 + i) for i, n in enumerate(lens)], 44100, 2


EXACT_CASES = {
    "ragged_stereo": _ragged_stereo,
    "mono_edges": lambda: ([signals.music_like(44100, n, 1, seed=60 + i) for i, n in enumerate([0, 1, 1025, 4097])], 44100, 1),
    "ch3": lambda: ([signals.music_like(44100, 12000, 3, seed=73)], 44100, 3),
    "ch8": lambda: ([signals.music_like(44100, 12000, 8, seed=78)], 44100, 8),
    "rate8000": lambda: ([signals.music_like(8000, 20000, 2, seed=8000)], 8000, 2),
    "rate96000": lambda: ([signals.music_like(96000, 20000, 2, seed=96000)], 96000, 2),
    "rate384000": lambda: ([signals.music_like(384000, 20000, 2, seed=384000)], 384000, 2),
    # 70 clips of one to three frames: more clips than kFewClips
    "many_short": lambda: ([signals.music_like(44100, 1 + (37 * i) % 2000, 2, seed=200 + i) for i in range(70)], 44100, 2),
}


@pytest.mark.parametrize("case", list(EXACT_CASES))
def test_every_rung_is_the_encoders_own_file(ctx, case):
    clips, sr, ch = EXACT_CASES[case]()
    files = _check(ctx, clips, sr, ch, GRID_X, case)
    p = flofile.parse(files[-1][GRID_X.index(1.0)])
    assert p.crc_valid and p.is_lossy and p.lossy_quality == 4


# ---------------------------------------------------------------------------------------------- 2. packer branches under a changing mask
def _pcm_case(name):
    for n, pcm, sr, ch, q in lossy_cases.pcm_cases():
        if n == name:
            return pcm, sr, ch
    raise KeyError(name)


def _nan_inf():
    x = signals.fast_noise(8192, 2)
    x[100], x[2000], x[3001] = np.nan, np.inf, -np.inf
    return x


PACKER_CASES = {
    "all_zero": lambda: (np.zeros(5000 * 2, np.float32), 44100, 2),
    "noise_runs_beyond_255": lambda: (signals.fast_noise(6000 * 2, 5, 1.0), 44100, 2),
    "noise_mono": lambda: (signals.fast_noise(6000, 6, 1.0), 44100, 1),
    "sine_zero_runs_mono": lambda: (signals.sine(440.0, 44100, 9000, 0.5, 1), 44100, 1),
    "sine_zero_runs_stereo": lambda: (signals.sine(440.0, 44100, 9000, 0.5, 2), 44100, 2),
    "square_full_scale": lambda: _pcm_case("square_full_scale"),        # non-zero runs of 777: two 255-cap continuations
    "impulse": lambda: _pcm_case("impulse"),
    "kept_tiny": lambda: _pcm_case("level_x1e-8_q1.0"),                 # |c| <= 1e-10 kept at transparent quality
    "fade_to_zero": lambda: _pcm_case("fade_to_zero_q1.0"),
    "nan_inf_mono": lambda: (_nan_inf(), 44100, 1),
    "nan_inf_stereo": lambda: (_nan_inf(), 44100, 2),
}


@pytest.mark.parametrize("case", list(PACKER_CASES))
def test_packer_branches_under_a_changing_mask(ctx, case):
    pcm, sr, ch = PACKER_CASES[case]()
    _check(ctx, [pcm], sr, ch, LADDER5, case)


# ---------------------------------------------------------------------------------------------- 3. rung count and order, misuse
def test_rung_count_order_and_misuse(ctx):
    clips, sr, ch = _ragged_stereo()
    clips = clips[3:6]
    own = {q: [ctx.encode_lossy(c, sr, ch, q) for c in clips] for q in GRID}
    one, _, _ = _ladder_files(ctx, clips, sr, ch, [0.4375])
    assert [f[0] for f in one] == own[0.4375]
    g32 = [GRID[i % 17] for i in range(32)]
    for rungs in (g32, GRID[::-1], [0.5, 0.25, 0.5, 1.0, 0.25]):
        files, _, _ = _ladder_files(ctx, clips, sr, ch, rungs)
        for j, q in enumerate(rungs):
            assert [f[j] for f in files] == own[q], (len(rungs), j, q)
    L = ctx._L
    q = np.array(g32 + [0.5], np.float32)
    pcm = clips[0]
    h = C.c_void_p()
    b = _batch(ctx, [pcm], sr, ch)
    assert L.flo_batch_encode_ladder(b._h, 33, q.ctypes.data, C.byref(h)) == ERR_ARG and not h.value
    assert L.flo_batch_encode_ladder(b._h, 0, q.ctypes.data, C.byref(h)) == ERR_ARG and not h.value
    assert L.flo_batch_encode_ladder(b._h, 4, None, C.byref(h)) == ERR_ARG
    assert L.flo_batch_encode_ladder(b._h, 4, q.ctypes.data, None) == ERR_ARG
    assert L.flo_batch_encode_ladder(None, 4, q.ctypes.data, C.byref(h)) == ERR_ARG
    with pytest.raises(flo_amd.FloError):
        b.encode_ladder([])
    assert ctx.encode_lossy(pcm, sr, ch, 0.5) == own[0.5][0]
    ll = flo_amd.Batch(ctx, flo_amd.MODE_LOSSLESS, [pcm.size], sr, ch, 5)
    ll.upload(0, pcm)
    assert L.flo_batch_encode_ladder(ll._h, 4, q.ctypes.data, C.byref(h)) == ERR_ARG and not h.value
    ll.close()
    assert ctx.encode_lossy(pcm, sr, ch, 0.5) == own[0.5][0]
    empty = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [pcm.size], sr, ch, 0.5)
    assert L.flo_batch_encode_ladder(empty._h, 4, q.ctypes.data, C.byref(h)) == ERR_STATE and not h.value     # nothing uploaded
    with pytest.raises(flo_amd.FloError):
        empty.encode_ladder(GRID)
    empty.close()
    assert ctx.encode_lossy(pcm, sr, ch, 0.5) == own[0.5][0]
    with b.encode_ladder([0.5]) as lad:
        assert L.flo_ladder_fetch(lad._h, 1, 0, None, 0, C.byref(h), C.byref(C.c_size_t())) == ERR_ARG        # clip out of range
        assert L.flo_ladder_fetch(lad._h, 0, 1, None, 0, C.byref(h), C.byref(C.c_size_t())) == ERR_ARG        # rung out of range
        assert L.flo_ladder_device_files(lad._h, 1, None, None, None) == ERR_ARG
        assert lad.fetch(0, 0) == own[0.5][0]
    b.close()


# ---------------------------------------------------------------------------------------------- 4, 5. groups; one transform whatever K
_CHILD = r"""
import hashlib, json, sys
sys.path[:0] = [%r, %r]
import flo_amd, signals
lens = [0, 1, 1023, 1024, 5000, 44100, 70001, 3 * 1024]
clips = [signals.music_like(44100, n, 2, seed=40 + i) for i, n in enumerate(lens)]
rungs = [0.0, 0.5, 0.9899, 0.99, 1.0]
ctx = flo_amd.Context(0)
b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [c.size for c in clips], 44100, 2, 0.5)
for i, c in enumerate(clips):
    b.upload(i, c)
ctx.profile_enable(True)
ctx.profile_reset()
lad = b.encode_ladder(rungs)
launches = {k: int(ctx.profile_query(k)[1]) for k in ("ladder_bands", "ladder_scan", "lossy_ladder")}
files = [[lad.fetch(i, j) for j in range(len(rungs))] for i in range(len(clips))]
print(json.dumps({"launches": launches, "sha": [[hashlib.sha256(f).hexdigest() for f in row] for row in files],
                  "sizes": lad.file_bytes.tolist()}))
lad.close()
b.close()
ctx.close()
"""


def _launches(ctx):
    return {k: int(ctx.profile_query(k)[1]) for k in ("ladder_bands", "ladder_scan", "lossy_ladder")}


def test_groups_of_clips_give_the_same_files(ctx):
    # 8 clips of 1, 2, 2, 2, 6, 45, 70 and 4 frames. A stereo frame takes, at 5 rungs, 5 slots of 4352 bytes with a size and an
    # offset word each (12 bytes) and three level rows of 2 x 128 bytes: room for 12 frames makes five groups - the first
    # four clips, then one clip each, the clips of 45 and of 70 frames larger than the limit
    limit = 12 * (5 * (4352 + 12) + 3 * 2 * 128)
    env = dict(os.environ, FLO_LADDER_GROUP_BYTES=str(limit))
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["launches"] == {"ladder_bands": 5, "ladder_scan": 5, "lossy_ladder": 5}
    clips, sr, ch = _ragged_stereo()
    ctx.profile_enable(True)
    ctx.profile_reset()
    files, sizes, _ = _ladder_files(ctx, clips, sr, ch, LADDER5)
    whole = _launches(ctx)
    ctx.profile_enable(False)
    assert whole == {"ladder_bands": 1, "ladder_scan": 1, "lossy_ladder": 1}
    assert res["sha"] == [[hashlib.sha256(f).hexdigest() for f in row] for row in files]
    assert np.array_equal(np.array(res["sizes"], np.uint64), sizes)


@pytest.mark.parametrize("k", [1, 8])
def test_one_transform_whatever_the_number_of_rungs(ctx, k):
    clips, sr, ch = _ragged_stereo()
    clips = clips[2:6]
    rungs = [i / 8 for i in range(1, k + 1)]
    b = _batch(ctx, clips, sr, ch)
    try:
        ctx.profile_enable(True)
        ctx.profile_reset()
        with b.encode_ladder(rungs) as lad:
            got = _launches(ctx)
            others = {name: int(ctx.profile_query(name)[1]) for name in ("lossy_bands", "lossy_frames", "lossy_chain", "lossy_chain2q", "size_curve")}
            assert lad.fetch(3, k - 1) == ctx.encode_lossy(clips[3], sr, ch, rungs[-1])
    finally:
        ctx.profile_enable(False)
        b.close()
    assert got == {"ladder_bands": 1, "ladder_scan": 1, "lossy_ladder": 1}, got      # not K encodes behind the new interface
    assert not any(others.values()), others


# ---------------------------------------------------------------------------------------------- 6. the batch is left alone
def _results(b):
    import torch
    n = b.data_bytes()
    files = [b.fetch(i) for i in range(b.n_clips)]
    buf = torch.zeros(sum(len(f) + 16 for f in files) + 64, dtype=torch.uint8, device="cuda:0")
    offs = b.pack_files(buf.data_ptr(), buf.numel())          # (the device files, packed)
    b.sync()
    packed = buf.cpu().numpy().tobytes()
    pcm = torch.zeros(sum(flofile.parse(f).total_samples for f in files) * b.channels + 64, dtype=torch.float32, device="cuda:0")
    poffs = b.decode_to(pcm.data_ptr(), pcm.numel())
    b.sync()
    return n, files, offs, packed, poffs, pcm.cpu().numpy().tobytes()


def test_ladder_leaves_the_batch_alone_and_outlives_it(ctx):
    clips, sr, ch = _ragged_stereo()
    clips = clips[1:7]
    a, b = _batch(ctx, clips, sr, ch, 0.55), _batch(ctx, clips, sr, ch, 0.55)
    lad = None
    try:
        for x in (a, b):
            x.encode(0)
            x.sync()
        lad = b.encode_ladder(LADDER5)       # behind encode + sync: fetch, sizes, packed device files and decode stay as they were
        assert _results(a) == _results(b)
        assert _results(b)[1] == [ctx.encode_lossy(c, sr, ch, 0.55) for c in clips]
        b.encode(0)                          # and an encode behind the ladder gives the files of a batch that never ran one
        b.sync()
        assert _results(a) == _results(b)
        # the batch's own quality plays no part
        c2 = _batch(ctx, clips, sr, ch, 0.05)
        with c2.encode_ladder(LADDER5) as other:
            assert all(other.fetch(i, j) == lad.fetch(i, j) for i in range(len(clips)) for j in range(5))
        c2.close()
        # the ladder's data is its own: the batch goes, the files stay
        b.close()
        a.close()
        flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [c.size for c in clips], sr, ch, 0.3).close()     # (the pool hands the blocks out again)
        for i, c in enumerate(clips):
            assert lad.fetch(i, 3, b"\x80") == ctx.encode_lossy(c, sr, ch, LADDER5[3], b"\x80"), i
    finally:
        if lad is not None:
            lad.close()
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------- 7. device files
def test_device_files_of_a_rung(ctx):
    clips, sr, ch = _ragged_stereo()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    b = _batch(ctx, clips, sr, ch)
    try:
        with b.encode_ladder(LADDER5) as lad:
            spans = []
            for j in range(5):
                base, offs, sizes = lad.device_files(j)
                assert all(o % 16 == 0 for o in offs) and base % 16 == 0
                assert sizes == [int(x) for x in lad.file_bytes[:, j]]
                for i in range(len(clips)):
                    got = np.empty(sizes[i], np.uint8)
                    assert hip.hipMemcpy(got.ctypes.data, base + offs[i], sizes[i], 2) == 0
                    assert got.tobytes() == lad.fetch(i, j), (i, j)
                    spans.append((base + offs[i], base + offs[i] + sizes[i]))
            spans.sort()
            assert all(a[1] <= b_[0] for a, b_ in zip(spans, spans[1:]))                     # no two files overlap
            # what stays resident is the files' bytes and their alignment, not K worst-case regions
            assert spans[-1][1] - spans[0][0] <= int(lad.file_bytes.sum()) + 16 * len(spans)
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------- 8. top level
def test_free_functions_match_encode_lossy_at_the_five_presets():
    sr, ch = 44100, 2
    x = signals.music_like(sr, 9000, ch, seed=801)
    m = b"\x81\xa5title\xa3abc"
    presets = [0.0, 0.35, 0.55, 0.75, 1.0]
    files = flo_amd.encode_ladder(x, sr, ch, presets, metadata=m)
    assert len(files) == 5
    for p in range(5):
        assert files[p] == flo_amd.encode_lossy(x, sr, ch, 16, p, m), p
    assert flo_amd.encode_ladder(x, sr, ch, presets)[2] == flo_amd.encode_lossy(x, sr, ch, 16, 2)
    clips = [signals.music_like(sr, n, 1, seed=810 + i) for i, n in enumerate([6000, 1401, 2])]      # (read as interleaved stereo)
    assert clips[1].size % ch == 1                                                        # a trailing partial sample-frame
    metas = [b"", m, b"\x80"]
    many = flo_amd.encode_ladder_many(clips, sr, ch, presets, metas)
    assert [len(r) for r in many] == [5, 5, 5]
    for i, c in enumerate(clips):
        assert many[i] == flo_amd.encode_ladder(c, sr, ch, presets, metadata=metas[i]), i
        # rung p is the file of the project's own batched route at that preset; for a clip of whole sample-frames that is
        # encode_lossy's file too (a trailing partial sample-frame is analysed by the batched route, as the reference does,
        # and read as zeros by the one-clip route: test_gpu_batch_analysis.py)
        for p in range(5):
            assert many[i][p] == flo_amd.encode_lossy_many([c], sr, ch, 16, p, [metas[i]])[0], (i, p)
            if c.size % ch == 0:
                assert many[i][p] == flo_amd.encode_lossy(c, sr, ch, 16, p, metas[i]), (i, p)
    assert flo_amd.encode_ladder_many([], sr, ch, presets) == []


def test_c_entry_point_on_host_buffers(ctx):
    sr, ch = 44100, 2
    clips = [signals.music_like(sr, n, ch, seed=820 + i) for i, n in enumerate([3000, 1, 12000])]
    clips[2] = clips[2][:-1]                                                              # n % ch != 0
    metas = [b"", b"\x81\xa5title\xa3abc", b"\x80"]
    rungs = np.array([0.9, 0.1, 1.0, 0.1], np.float32)
    k, K = len(clips), rungs.size
    L = ctx._L
    ptrs = (C.c_void_p * k)(*[c.ctypes.data for c in clips])
    lens = (C.c_size_t * k)(*[c.size for c in clips])
    keep = [C.create_string_buffer(m, len(m)) if m else None for m in metas]
    mp = (C.c_void_p * k)(*[C.addressof(x) if x is not None else None for x in keep])
    ml = (C.c_size_t * k)(*[len(m) for m in metas])
    outs, olens = (C.c_void_p * (k * K))(), (C.c_size_t * (k * K))()
    assert L.flo_encode_batch_ladder(ctx._h, k, ptrs, lens, sr, ch, K, rungs.ctypes.data, mp, ml, outs, olens) == 0
    for i in range(k):
        for j in range(K):
            got = C.string_at(outs[i * K + j], olens[i * K + j])
            L.flo_free(outs[i * K + j])
            assert got == ctx.encode_lossy(clips[i], sr, ch, float(rungs[j]), metas[i]), (i, j)
    assert L.flo_encode_batch_ladder(ctx._h, k, ptrs, lens, sr, ch, K, rungs.ctypes.data, None, None, outs, olens) == 0
    for i in range(k):
        for j in range(K):
            got = C.string_at(outs[i * K + j], olens[i * K + j])
            L.flo_free(outs[i * K + j])
            assert got == ctx.encode_lossy(clips[i], sr, ch, float(rungs[j])), (i, j)
    assert L.flo_encode_batch_ladder(ctx._h, k, ptrs, lens, sr, ch, 0, rungs.ctypes.data, None, None, outs, olens) == ERR_ARG
    assert L.flo_encode_batch_ladder(ctx._h, k, ptrs, lens, sr, ch, 33, rungs.ctypes.data, None, None, outs, olens) == ERR_ARG
    assert L.flo_encode_batch_ladder(ctx._h, k, ptrs, lens, sr, ch, K, rungs.ctypes.data, mp, None, outs, olens) == ERR_ARG
    assert L.flo_encode_batch_ladder(ctx._h, k, ptrs, lens, sr, ch, K, rungs.ctypes.data, None, None, None, olens) == ERR_ARG
    assert ctx.encode_lossy(clips[0], sr, ch, 0.5)


def test_cli_ladder(tmp_path, capsys, monkeypatch):
    from flo_amd import meta
    real = meta.time.strftime
    monkeypatch.setattr(meta.time, "strftime", lambda fmt, *a: "2024-05-06T07:08:09Z" if fmt.endswith("Z") else real(fmt, *a))
    wav = tmp_path / "audio.wav"
    wav.write_bytes(example_bytes("audio.wav"))
    names = ["low", "transparent", "high", "medium", "veryhigh"]
    outdir = tmp_path / "rungs"
    assert cli.main(["ladder", str(wav), str(outdir), "--qualities", ",".join(names), "--json", "--title", "T"]) == 0
    rows = json.loads(capsys.readouterr().out)
    assert [r["rung"] for r in rows] == list(range(5)) and [r["quality"] for r in rows] == [cli.QUALITY[n] for n in names]
    from flo_amd.wav import read_wav_bytes
    samples, sr, ch = read_wav_bytes(wav.read_bytes())
    for j, name in enumerate(names):
        got = (outdir / f"audio.r{j}.flo").read_bytes()
        one = tmp_path / f"one{j}.flo"
        assert cli.main(["encode", str(wav), str(one), "--lossy", "--quality", name, "--title", "T"]) == 0
        assert got == one.read_bytes(), name
        assert rows[j]["bytes"] == len(got)
        assert rows[j]["kbps"] == pytest.approx(len(got) * 8 / 1000 / (samples.size / ch / sr))
        assert flofile.parse(got).crc_valid
    capsys.readouterr()
    assert cli.main(["ladder", str(wav), str(outdir), "--qualities", "med,med"]) == 0 and "quality" in capsys.readouterr().out
    assert (outdir / "audio.r0.flo").read_bytes() == (outdir / "audio.r1.flo").read_bytes() != got
    assert cli.main(["ladder", str(wav), str(outdir), "--qualities", "loud"]) == 1
