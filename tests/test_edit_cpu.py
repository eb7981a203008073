"""The host side of the batch editing stage on CPU: flo_amd/csrc/edit_plan.cpp against the cases of
tests/native/edit_plan_test.cpp (built here with g++, sanitizers on, run stand-alone); the new symbols in the header, the
export list, the Python package and the command line; flo_edit_tile_frames through the C ABI against the model; the Python
helpers that build segments and matrices. None of this needs a device. (The entries in the recycled-memory registry are
tests/edit_recycled.py's, which only tests/test_gpu_edit.py imports: DESIGN 4.15.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import edit_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flo_amd", "csrc")
SYMBOLS = ["flo_batch_edit", "flo_batch_active_range", "flo_edit", "flo_edit_tile_frames"]


def test_edit_plan_native(tmp_path):
    exe = str(tmp_path / "edit_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "edit_plan_test.cpp"), os.path.join(CSRC, "edit_plan.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.startswith("ok"), r.stdout


def test_symbols_are_declared_listed_and_exported():
    import flo_amd
    from flo_amd import _native, cli
    header = open(os.path.join(ROOT, "include", "flo_hip.h")).read()
    lib = _native.lib()
    for s in SYMBOLS:
        assert re.search(r"\b%s\(" % s, header), s
        assert s in _native.EXPORTS and hasattr(lib, s), s
    assert C.sizeof(_native.EditSegment) == 40
    assert re.search(r"\}\s*flo_edit_segment;\s*/\* 40 bytes \*/", header)
    assert [f[0] for f in _native.EditSegment._fields_] == ["start", "frames", "clip", "pad_head", "pad_tail", "fade_in", "fade_out", "reserved"]
    for name in ("edit", "edit_many", "remix", "remix_many", "trim_silence", "trim_silence_many", "active_range", "active_range_many",
                 "edit_tile_frames"):
        assert hasattr(flo_amd, name), name
    for name in ("edit", "remix", "to_mono", "active_ranges", "trim_silence"):
        assert hasattr(flo_amd.Batch, name), name
    assert hasattr(flo_amd.Context, "edit")
    for name in ("edit_options", "apply_edit", "edit_wav"):
        assert hasattr(cli, name), name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for word in ("edit_kernels", "edit_plan", " edit "):
        assert word in mk, word


def test_the_model_restates_the_constants():
    hpp = open(os.path.join(CSRC, "edit_plan.hpp")).read()
    for name, value in (("kEditThreads", M.THREADS), ("kEditTileFloats", M.TILE_FLOATS), ("kEditMaxMix", M.MAX_MIX)):
        assert re.search(r"\b%s = %d\b" % (name, value), hpp), name
    assert "kEditMaxFade = 1u << 24" in hpp and M.MAX_FADE == 1 << 24
    assert "kEditInterior = 0, kEditEdge = 1, kEditFaded = 2" in hpp and (M.INTERIOR, M.EDGE, M.FADED) == (0, 1, 2)


def test_tile_frames_through_the_abi_equals_the_model():
    import flo_amd
    from flo_amd import _native
    for cin in (1, 2, 3, 8, 200):
        for cout in range(1, 256):
            assert flo_amd.edit_tile_frames(cin, cout) == M.tile_frames(cin, cout), (cin, cout)
    n = C.c_uint32()
    L = _native.lib()
    assert L.flo_edit_tile_frames(0, 1, C.byref(n)) == 1 and L.flo_edit_tile_frames(1, 0, C.byref(n)) == 1   # FLO_ERR_ARG
    assert L.flo_edit_tile_frames(1, 1, None) == 1
    with pytest.raises(flo_amd.FloError):
        flo_amd.edit_tile_frames(2, 0)


def test_segments_and_matrices_of_the_python_faces():
    from flo_amd import _native, api
    segs = api._edit_segments([dict(clip=1), dict(clip=0, start=4, frames=3, pad_head=1, pad_tail=2, fade_in=3, fade_out=1),
                               dict(clip=1, start=90), _native.EditSegment(1, 2, 0, 3, 4, 0, 0, 0)], [10, 50])
    got = [(g.start, g.frames, g.clip, g.pad_head, g.pad_tail, g.fade_in, g.fade_out, g.reserved) for g in segs]
    assert got == [(0, 50, 1, 0, 0, 0, 0, 0), (4, 3, 0, 1, 2, 3, 1, 0), (90, 0, 1, 0, 0, 0, 0, 0), (1, 2, 0, 3, 4, 0, 0, 0)]
    assert len(api._edit_segments([], [])) == 0
    with pytest.raises(api.FloError, match="unknown keys"):
        api._edit_segments([dict(clip=0, fade=3)], [10])
    assert api._edit_matrix(2, None, None) == (2, None) and api._edit_matrix(2, 5, None) == (5, None)
    cout, m = api._edit_matrix(2, None, [[0.5, 0.5]])
    assert cout == 1 and m.dtype == np.float32 and m.tolist() == [0.5, 0.5]
    cout, m = api._edit_matrix(1, 2, [1.0, -1.0])
    assert cout == 2 and m.tolist() == [1.0, -1.0]
    for bad in (([[1, 2, 3]], 2, None), ([[1, 2]], 2, 3), ([1, 2, 3], 2, None)):
        with pytest.raises(api.FloError, match="matrix"):
            api._edit_matrix(bad[1], bad[2], bad[0])


def test_trim_segments_are_the_models():
    from flo_amd import api
    frames = [48000, 48000, 100, 0, 30]
    ranges = [(1000, 40000), (0, 0), (5, 100), (0, 0), (29, 30)]
    for pre, post, fade in ((0.0, 0.0, 0.0), (10.0, 25.0, 5.0), (1e6, 1e6, 1e6), (0.01, 0.011, 0.5)):
        got = api.trim_segments(np.array(ranges, np.uint64), frames, 48000, pre, post, fade)
        for i, g in enumerate(got):
            want = M.trim_segment(i, ranges[i][0], ranges[i][1], frames[i], 48000, pre, post, fade)
            assert dict(want, **g) == want, (i, g, want)
            assert g["fade_in"] <= g["frames"] and g["fade_in"] < M.MAX_FADE
    assert api.trim_segments([(0, 0)], [10], 8000)[0]["frames"] == 0


def test_the_fade_bound():
    """fades of 2^24 and above are refused, 2^24 - 1 is the longest: u and v below it convert to f32 exactly"""
    clip = [1 << 25]
    assert M.refusal(clip, 1, False, [M.seg(0, 0, 1 << 24, fade_in=1 << 24)], 1, None) == "fade_in"
    assert M.refusal(clip, 1, False, [M.seg(0, 0, 1 << 24, fade_out=1 << 24)], 1, None) == "fade_out"
    assert M.refusal(clip, 1, False, [M.seg(0, 0, 1 << 24, fade_in=(1 << 24) - 1, fade_out=(1 << 24) - 1)], 1, None) is None
    u = np.array([(1 << 24) - 2, (1 << 24) - 1], np.int64)
    assert np.array_equal(u.astype(np.float32).astype(np.int64), u)
    assert int(np.float32((1 << 24) + 1)) != (1 << 24) + 1


def test_cli_knows_the_options():
    from flo_amd import cli
    assert cli.edit_options() is None
    o = cli.edit_options(mono=True, trim_silence=-50.0)
    assert o["mono"] and o["trim_silence"] == -50.0 and o["matrix"] is None
    assert cli.edit_options(channels=2, matrix="1,0, 0,1")["matrix"] == [1.0, 0.0, 0.0, 1.0]
    with pytest.raises(ValueError):
        cli.edit_options(mono=True, channels=1, matrix="1,1")
    with pytest.raises(ValueError):
        cli.edit_options(channels=2)
    with pytest.raises(SystemExit):
        cli.main(["edit", "a.wav"])   # the output is required
    with pytest.raises(SystemExit):
        cli.main(["encode", "a.wav", "b.flo", "--trim-silence"])   # the threshold is required
