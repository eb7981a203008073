"""The host side of the mixing stage on CPU: flo_amd/csrc/mix_plan.cpp against the cases of tests/native/mix_plan_test.cpp
(built here with g++, sanitizers on, run stand-alone); the new symbols in the header, the export list, the library, the
Makefile, the Python package and the command line; the Python helpers that build parts and output lengths. None of this
needs a device. (The entry in the recycled-memory registry is tests/mix_recycled.py's, which tests/test_gpu_batch_mix.py
imports: DESIGN 4.17.)"""
import ctypes as C
import os
import re
import subprocess

import pytest

import mix_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flo_amd", "csrc")
SYMBOLS = ["flo_batch_mix", "flo_mix"]


def test_mix_plan_native(tmp_path):
    exe = str(tmp_path / "mix_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "mix_plan_test.cpp"), os.path.join(CSRC, "mix_plan.cpp")], check=True)
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
    assert C.sizeof(_native.MixPart) == 48
    assert re.search(r"\}\s*flo_mix_part;\s*/\* 48 bytes \*/", header)
    fields = ["start", "frames", "at", "out", "batch", "clip", "fade_in", "fade_out", "gain"]
    assert [f[0] for f in _native.MixPart._fields_] == fields
    offsets = [getattr(_native.MixPart, f).offset for f in fields]
    assert offsets == [0, 8, 16, 24, 28, 32, 36, 40, 44]   # no padding
    body = re.search(r"typedef struct flo_mix_part \{(.*?)\}", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(start|frames|at|out|batch|clip|fade_in|fade_out|gain)\b", body) == fields
    for name in ("mix", "concat", "concat_parts"):
        assert hasattr(flo_amd, name), name
    for name in ("mix", "concat"):
        assert hasattr(flo_amd.Batch, name), name
    assert hasattr(flo_amd.Context, "mix")
    for name in ("mix_options", "mix_wavs", "concat_wavs"):
        assert hasattr(cli, name), name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for word in ("mix_kernels mix mix_plan", " mix\n", " mix_plan\n"):
        assert word in mk, word


def test_the_kernel_shares_the_plans_constants():
    hpp = open(os.path.join(CSRC, "mix_plan.hpp")).read()
    assert "kMixNone = 0, kMixWhole = 1, kMixPartial = 2" in hpp and (M.NONE, M.WHOLE, M.PARTIAL) == (0, 1, 2)
    assert "kMixThreads = kEditThreads" in hpp and 'static_assert(sizeof(MixPart) == 64' in hpp
    hip = open(os.path.join(CSRC, "mix_kernels.hip")).read()
    assert "mix_part_in_tile(" in hip and "edit_tile_frames(" in hip and "tile_clip(" in hip and "__shared__" not in hip


def test_parts_and_output_lengths_of_the_python_faces():
    from flo_amd import _native, api
    parts = api._mix_parts([dict(out=0, clip=1), dict(out=0, batch=1, clip=0, start=4, frames=3, at=60, gain=0.5, fade_in=3, fade_out=1),
                            dict(out=2, clip=1, start=90), dict(out=2, batch=5, clip=0), _native.MixPart(1, 2, 3, 4, 0, 1, 0, 0, -1.0)], [[10, 50], [7]])
    got = [(g.start, g.frames, g.at, g.out, g.batch, g.clip, g.fade_in, g.fade_out, g.gain) for g in parts]
    assert got == [(0, 50, 0, 0, 0, 1, 0, 0, 1.0), (4, 3, 60, 0, 1, 0, 3, 1, 0.5), (90, 0, 0, 2, 0, 1, 0, 0, 1.0), (0, 0, 0, 2, 5, 0, 0, 0, 1.0),
                   (1, 2, 3, 4, 0, 1, 0, 0, -1.0)]
    assert api._mix_out_frames(parts) == [63, 0, 0, 0, 5]
    assert len(api._mix_parts([], [[]])) == 0 and api._mix_out_frames(api._mix_parts([], [[]])) == []
    with pytest.raises(api.FloError, match="unknown keys"):
        api._mix_parts([dict(out=0, clip=0, pad_head=3)], [[10]])
    with pytest.raises(api.FloError, match="required"):
        api._mix_parts([dict(clip=0)], [[10]])


def test_the_fade_bound():
    """fades of 2^24 and above are refused, 2^24 - 1 is the longest: the edit stage's bound, for the same reason"""
    clips = [[1 << 25]]
    assert M.refusal(clips, 1, 1, [9], [M.part(0, 0, 0, 0, 1 << 24, fade_in=1 << 24)]) == "fade_in"
    assert M.refusal(clips, 1, 1, [9], [M.part(0, 0, 0, 0, 1 << 24, fade_out=1 << 24)]) == "fade_out"
    assert M.refusal(clips, 1, 1, [9], [M.part(0, 0, 0, 0, 1 << 24, fade_in=(1 << 24) - 1, fade_out=(1 << 24) - 1)]) is None


def test_cli_knows_the_commands():
    from flo_amd import cli
    assert cli.mix_options(2) == ([1.0, 1.0], [0.0, 0.0])
    assert cli.mix_options(3, "1,0.5,-1", "0,10.5,250") == ([1.0, 0.5, -1.0], [0.0, 10.5, 250.0])
    assert cli.mix_options(2, [0.25, 2], (5, 0)) == ([0.25, 2.0], [5.0, 0.0])
    with pytest.raises(ValueError):
        cli.mix_options(2, "1,2,3")
    with pytest.raises(ValueError):
        cli.mix_options(2, None, "0,-1")
    with pytest.raises(SystemExit):
        cli.main(["mix", "a.wav", "b.wav"])      # the output is required
    with pytest.raises(SystemExit):
        cli.main(["concat", "--out", "c.wav"])   # and so is an input
    from flo_amd.wav import write_wav_bytes
    import numpy as np
    a, b = write_wav_bytes(np.zeros(8, np.float32), 48000, 2), write_wav_bytes(np.zeros(8, np.float32), 44100, 2)
    for call in (lambda: cli.mix_wavs([a, b]), lambda: cli.concat_wavs([a, b])):   # refused before any device is touched
        with pytest.raises(ValueError, match="resample"):
            call()
