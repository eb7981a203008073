"""The host side of the partitioned FFT convolution on CPU: flo_amd/csrc/fftconv_plan.cpp (with conv_plan.cpp, whose checks
it shares) against the cases of tests/native/fftconv_plan_test.cpp, built here with g++, sanitizers on, and run stand-alone;
the struct of the geometry; the new names in the header, the export list, the library, the Makefile, the Python package and
the command line; how `method` picks the path. None of this needs a device. (The entry in the recycled-memory registry is
tests/fftconv_recycled.py's, which tests/test_gpu_fftconv.py imports: DESIGN 4.19.)"""
import ctypes as C
import os
import re
import subprocess

import pytest

import fftconv_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flo_amd", "csrc")
SYMBOLS = ["flo_batch_convolve_fft", "flo_convolve_fft", "flo_conv_fft_geometry"]


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fftconv") / "fftconv_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "fftconv_plan_test.cpp"), os.path.join(CSRC, "fftconv_plan.cpp"),
                    os.path.join(CSRC, "conv_plan.cpp")], check=True)
    return exe


def test_fftconv_plan_native(native):
    r = subprocess.run([native], capture_output=True, text=True, timeout=300)
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
    fields = ["block_frames", "lane_blocks", "max_taps", "crossover_taps"]
    assert [f[0] for f in _native.ConvFftInfo._fields_] == fields and C.sizeof(_native.ConvFftInfo) == 16
    assert [getattr(_native.ConvFftInfo, f).offset for f in fields] == [0, 4, 8, 12]
    assert re.search(r"\}\s*flo_conv_fft_info;\s*/\* 16 bytes \*/", header)
    body = re.search(r"typedef struct flo_conv_fft_info \{(.*?)\}", header, re.S).group(1)
    assert re.findall(r"\b(block_frames|lane_blocks|max_taps|crossover_taps)\b", body) == fields
    assert re.search(r"#define FLO_CONV_FFT_MAX_TAPS 1048576u", header) and _native.CONV_FFT_MAX_TAPS == M.MAX_TAPS == 1048576
    assert hasattr(flo_amd, "conv_fft_geometry")
    api = open(os.path.join(ROOT, "flo_amd", "api.py")).read()
    for s in SYMBOLS:
        assert s in api, s
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for word in (" fftconv ", " fftconv_plan ", "fftconv_kernels fftconv fftconv_plan"):
        assert word in mk, word
    assert "--method" in open(os.path.join(ROOT, "flo_amd", "cli.py")).read()
    import inspect
    for fn in (flo_amd.Batch.convolve, flo_amd.Context.convolve, flo_amd.convolve, cli.convolve_wavs):
        assert inspect.signature(fn).parameters["method"].default == "direct", fn
    assert "method" not in inspect.signature(flo_amd.Batch.filter).parameters


def test_the_geometry_is_the_plans_and_the_kernels():
    import flo_amd
    hpp = open(os.path.join(CSRC, "fftconv_plan.hpp")).read()
    B = int(re.search(r"#define FLO_FFTCONV_BLOCK (\d+)", hpp).group(1))
    LB = int(re.search(r"#define FLO_FFTCONV_LANE_BLOCKS (\d+)", hpp).group(1))
    cross = int(re.search(r"kFcCrossoverTaps = (\d+);", hpp).group(1))
    assert B in (256, 512, 1024)
    for ch in range(1, 9):
        for ir_ch in {1, ch}:
            assert flo_amd.conv_fft_geometry(ch, ir_ch) == dict(block_frames=B, lane_blocks=LB, max_taps=M.MAX_TAPS, crossover_taps=cross)
    for ch, ir_ch in ((0, 1), (9, 1), (4, 2), (2, 0)):
        with pytest.raises(flo_amd.FloError):
            flo_amd.conv_fft_geometry(ch, ir_ch)
    assert "static_assert(sizeof(FcSpecJob) == 64" in hpp and "static_assert(sizeof(FcMacJob) == 64" in hpp
    hip = open(os.path.join(CSRC, "fftconv_kernels.hip")).read()
    assert "tile_clip(" in hip and "__builtin_fmaf" in hip
    assert "atomic" not in hip.lower().replace("no atomics", "") and "asm" not in hip


def test_cli_takes_the_method():
    from flo_amd import cli
    with pytest.raises(SystemExit):
        cli.main(["convolve", "a.wav", "ir.wav", "out.wav", "--method", "overlap-add"])


def test_method_picks_the_path():
    import flo_amd
    from flo_amd import api
    cross = flo_amd.conv_fft_geometry()["crossover_taps"]
    ir_frames = [cross - 1, cross, 4 * cross, 0]
    jobs = lambda *irs: api._conv_jobs([dict(clip=0, ir=i) for i in irs], [100], ir_frames)   # noqa: E731
    assert not api._conv_takes_fft("direct", jobs(2), ir_frames) and api._conv_takes_fft("fft", jobs(3), ir_frames)
    assert not api._conv_takes_fft("auto", jobs(0), ir_frames) and api._conv_takes_fft("auto", jobs(1), ir_frames)
    assert api._conv_takes_fft("auto", jobs(0, 3, 2), ir_frames) and not api._conv_takes_fft("auto", jobs(), ir_frames)
    # K, not taps and not the response's length: ir_start and the cap count
    cut = api._conv_jobs([dict(clip=0, ir=2, ir_start=3 * cross + 1)], [100], ir_frames)
    assert not api._conv_takes_fft("auto", cut, ir_frames)
    cut = api._conv_jobs([dict(clip=0, ir=2, taps=cross - 1)], [100], ir_frames)
    assert not api._conv_takes_fft("auto", cut, ir_frames)
    with pytest.raises(api.FloError, match="unknown method"):
        api._conv_takes_fft("overlap-add", jobs(0), ir_frames)
