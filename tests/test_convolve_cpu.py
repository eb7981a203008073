"""The host side of the FIR stage on CPU: flo_amd/csrc/conv_plan.cpp and fir_design.cpp against the cases of
tests/native/conv_plan_test.cpp (built here with g++, sanitizers on, run stand-alone); flo_fir_design against a numpy f64
restatement of its definition and its frequency response; the new symbols in the header, the export list, the library, the
Makefile, the Python package and the command line; the Python helpers that build jobs. None of this needs a device. (The
entry in the recycled-memory registry is tests/convolve_recycled.py's, which tests/test_gpu_convolve.py imports: DESIGN 4.18.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import convolve_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flo_amd", "csrc")
SYMBOLS = ["flo_batch_convolve", "flo_convolve", "flo_conv_geometry", "flo_fir_design"]
DESIGNS = [(M.LOWPASS, 48000, 0.0, 4000.0, 255, 9.0), (M.HIGHPASS, 48000, 80.0, 0.0, 255, 9.0), (M.BANDPASS, 44100, 300.0, 3400.0, 511, 9.0),
           (M.BANDSTOP, 48000, 950.0, 1050.0, 1001, 6.5), (M.LOWPASS, 8000, 0.0, 3999.0, 3, 0.0), (M.BANDPASS, 384000, 1.0, 191999.0, 65535, 16.0),
           (M.HIGHPASS, 22050, 5000.0, 0.0, 33, 16.0), (M.BANDSTOP, 96000, 10.0, 47000.0, 4097, 0.5)]


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("conv") / "conv_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "conv_plan_test.cpp"), os.path.join(CSRC, "conv_plan.cpp"),
                    os.path.join(CSRC, "fir_design.cpp")], check=True)
    return exe


def test_conv_plan_native(native):
    r = subprocess.run([native], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.startswith("ok"), r.stdout


def test_the_design_equals_its_definition_within_one_ulp(native):
    """every kind against numpy's f64 restatement (np.sinc, np.i0), within one f32 ulp: the bound test_resample_cpu.py uses
    for the resampler's table (the two I0 and sin implementations differ in the last f64 bits, which moves a rounding to f32
    by at most one step)"""
    text = "".join("%d %d %r %r %d %r\n" % d for d in DESIGNS)
    r = subprocess.run([native, "design"], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(DESIGNS)
    for d, line in zip(DESIGNS, lines):
        got = np.array([int(w, 16) for w in line.split()], np.uint32).view(np.float32)
        want64 = M.fir_design64(*d)
        want = want64.astype(np.float32)
        assert got.size == d[4]
        ulp = np.spacing(np.abs(want)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        assert (err <= ulp).all(), (d, int(np.argmax(err / ulp)), float((err / ulp).max()))
        assert np.array_equal(got, got[::-1]), d   # linear phase


def test_the_library_designs_the_same_tables(native):
    import flo_amd
    for d in DESIGNS[:5]:
        r = subprocess.run([native, "design"], input="%d %d %r %r %d %r\n" % d, capture_output=True, text=True, timeout=300)
        want = np.array([int(w, 16) for w in r.stdout.split()], np.uint32)
        got = flo_amd.fir_design(d[0], d[1], d[2], d[3], d[4], d[5])
        assert np.array_equal(got.view(np.uint32), want), d
    assert np.array_equal(flo_amd.fir_design("lowpass", 48000, f_hi=4000.0), flo_amd.fir_design(0, 48000, 0.0, 4000.0, 255, 9.0))
    assert np.array_equal(flo_amd.fir_design("lowpass", 48000, 4000.0), flo_amd.fir_design("lowpass", 48000, f_hi=4000.0))   # its one frequency
    assert np.array_equal(flo_amd.fir_design("highpass", 48000, f_hi=80.0), flo_amd.fir_design("highpass", 48000, 80.0))
    for args, word in ((("lowpass", 48000, None, 4000.0, 254), "taps"), (("lowpass", 48000, None, 24000.0), "f_hi"), (("bandpass", 48000, 500.0, 400.0), "f_lo"),
                       (("highpass", 48000, 0.0), "f_lo"), (("lowpass", 48000, None, 4000.0, 255, 17.0), "beta"), (("lowpass", 0, None, 4000.0), "rate"),
                       ((7, 48000, 1.0, 2.0), "kind")):
        with pytest.raises(flo_amd.FloError, match=word):
            flo_amd.fir_design(*args)
    with pytest.raises(flo_amd.FloError, match="unknown filter kind"):
        flo_amd.fir_design("notch", 48000, 1.0, 2.0)


def test_the_frequency_response_of_the_definition():
    """The f64 definition at the defaults (beta 9, 255 taps) at 48 kHz, by FFT. Kaiser's estimates for beta = 9: attenuation
    A = 9 / 0.1102 + 8.7 = 90.4 dB, transition width (A - 8) / (2.285 (taps - 1)) rad = 1084 Hz, centred on the cut-off. Beyond
    half of that from a cut-off the stop band must lie at least 80 dB down (10 dB for the looseness of the estimate).
    Measured here: low-pass 4 kHz 90.35 dB, high-pass 4 kHz 88.91 dB, band-pass 3 .. 8 kHz 89.29 dB, band-stop 3 .. 8 kHz
    89.88 dB; pass-band ripple at most 0.0003 dB in all four."""
    rate, taps, beta = 48000, 255, 9.0
    A = beta / 0.1102 + 8.7
    half = (A - 8.0) / (2.285 * (taps - 1)) / (2 * np.pi) * rate / 2
    assert 540 < half < 545
    n = 1 << 18
    f = np.arange(n // 2 + 1) * rate / n
    ny = rate / 2
    cases = [(M.LOWPASS, None, 4000.0, [(4000 + half, ny)], [(0, 4000 - half)], 90.35),
             (M.HIGHPASS, 4000.0, None, [(0, 4000 - half)], [(4000 + half, ny)], 88.91),
             (M.BANDPASS, 3000.0, 8000.0, [(0, 3000 - half), (8000 + half, ny)], [(3000 + half, 8000 - half)], 89.29),
             (M.BANDSTOP, 3000.0, 8000.0, [(3000 + half, 8000 - half)], [(0, 3000 - half), (8000 + half, ny)], 89.88)]
    for kind, lo, hi, stops, passes, measured in cases:
        db = 20 * np.log10(np.maximum(np.abs(np.fft.rfft(M.fir_design64(kind, rate, lo, hi, taps, beta), n)), 1e-300))
        stop = -max(db[(f >= a) & (f <= b)].max() for a, b in stops)
        ripple = max(np.abs(db[(f >= a) & (f <= b)]).max() for a, b in passes)
        print("kind %d: stop band %.2f dB down, pass band within %.5f dB" % (kind, stop, ripple))
        assert stop >= 80.0, (kind, stop)
        assert abs(stop - measured) < 0.05 and ripple < 0.001, (kind, stop, ripple)


def test_symbols_are_declared_listed_and_exported():
    import flo_amd
    from flo_amd import _native, cli
    header = open(os.path.join(ROOT, "include", "flo_hip.h")).read()
    lib = _native.lib()
    for s in SYMBOLS:
        assert re.search(r"\b%s\(" % s, header), s
        assert s in _native.EXPORTS and hasattr(lib, s), s
    assert C.sizeof(_native.ConvJob) == 40
    assert re.search(r"\}\s*flo_conv_job;\s*/\* 40 bytes \*/", header)
    fields = ["frames", "skip", "ir_start", "clip", "ir", "taps", "reserved"]
    assert [f[0] for f in _native.ConvJob._fields_] == fields
    assert [getattr(_native.ConvJob, f).offset for f in fields] == [0, 8, 16, 24, 28, 32, 36]   # no padding
    body = re.search(r"typedef struct flo_conv_job \{(.*?)\}", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(frames|skip|ir_start|clip|ir|taps|reserved)\b", body) == fields
    assert [f[0] for f in _native.ConvInfo._fields_] == ["tile_frames", "tap_chunk", "lane_outputs"] and C.sizeof(_native.ConvInfo) == 12
    assert re.search(r"#define FLO_CONV_MAX_TAPS 65536u", header) and _native.CONV_MAX_TAPS == M.MAX_TAPS == 65536
    for name, v in (("LOWPASS", 0), ("HIGHPASS", 1), ("BANDPASS", 2), ("BANDSTOP", 3)):
        assert re.search(r"#define FLO_FIR_%s %du" % (name, v), header) and getattr(_native, "FIR_" + name) == getattr(M, name) == v
    for name in ("convolve", "fir_design", "fir_filter", "conv_geometry", "conv_mode"):
        assert hasattr(flo_amd, name), name
    for name in ("convolve", "filter"):
        assert hasattr(flo_amd.Batch, name), name
    assert hasattr(flo_amd.Context, "convolve") and not hasattr(flo_amd.Context, "filter")
    for name in ("filter_options", "filter_wav", "convolve_wavs"):
        assert hasattr(cli, name), name
    api = open(os.path.join(ROOT, "flo_amd", "api.py")).read()
    for s in SYMBOLS:
        assert s in api, s
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for word in ("conv_kernels convolve conv_plan fir_design", " convolve ", " conv_plan fir_design "):
        assert word in mk, word


def test_the_geometry_is_the_models_and_the_kernels():
    import flo_amd
    for ch in range(1, 9):
        for ir_ch in {1, ch}:
            assert flo_amd.conv_geometry(ch, ir_ch) == dict(tile_frames=M.TILE, tap_chunk=M.CHUNK, lane_outputs=M.LANE)
    for ch, ir_ch in ((0, 1), (9, 1), (4, 2), (2, 0)):
        with pytest.raises(flo_amd.FloError):
            flo_amd.conv_geometry(ch, ir_ch)
    hpp = open(os.path.join(CSRC, "conv_plan.hpp")).read()
    assert "kConvLaneOutputs = %d;" % M.LANE in hpp and "kConvTapChunk = %d;" % M.CHUNK in hpp and "kConvThreads = 256;" in hpp
    assert "static_assert(sizeof(ConvJob) == 64" in hpp and "static_assert(sizeof(flo_conv_job) == 40" in hpp
    hip = open(os.path.join(CSRC, "conv_kernels.hip")).read()
    assert "tile_clip(" in hip and "conv_lds_index(" in hip and "__builtin_fmaf" in hip and "__builtin_elementwise_fma" in hip
    assert "atomic" not in hip.lower() and "mfma" not in hip.lower() and "asm" not in hip


def test_jobs_and_modes_of_the_python_faces():
    from flo_amd import _native, api
    assert api.conv_mode("head", 10, 4) == (0, 10) and api.conv_mode("full", 10, 4) == (0, 13) and api.conv_mode("centered", 10, 4) == (1, 10)
    assert api.conv_mode("centered", 10, 255) == (127, 10) and api.conv_mode("centered", 10, 1) == (0, 10)
    for mode in ("head", "full", "centered"):   # N == 0 and K == 0
        assert api.conv_mode(mode, 0, 4) == ((1 if mode == "centered" else 0), 0)
        assert api.conv_mode(mode, 10, 0) == (0, 0 if mode == "full" else 10)
        assert api.conv_mode(mode, 0, 0) == (0, 0)
        for n, k in ((0, 0), (0, 5), (7, 0), (7, 5), (7, 6)):
            g = M.mode_job(mode, n, k)
            assert api.conv_mode(mode, n, k) == (g["skip"], g["frames"])
    with pytest.raises(api.FloError, match="unknown mode"):
        api.conv_mode("same", 1, 1)
    jobs = api._conv_jobs([dict(clip=1), dict(clip=0, ir=1, frames=3, skip=4, ir_start=5, taps=6), dict(clip=9), _native.ConvJob(1, 2, 3, 4, 5, 6, 0)], [10, 50], [7])
    got = [(g.frames, g.skip, g.ir_start, g.clip, g.ir, g.taps, g.reserved) for g in jobs]
    assert got == [(50, 0, 0, 1, 0, M.ALL, 0), (3, 4, 5, 0, 1, 6, 0), (0, 0, 0, 9, 0, M.ALL, 0), (1, 2, 3, 4, 5, 6, 0)]
    every = api._conv_jobs(None, [10, 0, 3], [4, 0, 9], [0, 1, 2], "full", 6)
    assert [(g.frames, g.skip, g.clip, g.ir, g.taps) for g in every] == [(13, 0, 0, 0, 6), (0, 0, 1, 1, 6), (8, 0, 2, 2, 6)]
    every = api._conv_jobs(None, [10, 3], [4, 9], 1, "centered")
    assert [(g.frames, g.skip, g.clip, g.ir, g.taps) for g in every] == [(10, 4, 0, 1, M.ALL), (3, 4, 1, 1, M.ALL)]
    assert len(api._conv_jobs([], [1], [1])) == 0 and len(api._conv_jobs(None, [], [1])) == 0
    with pytest.raises(api.FloError, match="unknown keys"):
        api._conv_jobs([dict(clip=0, gain=0.5)], [10], [4])
    with pytest.raises(api.FloError, match="required"):
        api._conv_jobs([dict(ir=0)], [10], [4])
    with pytest.raises(api.FloError, match="entries"):
        api._conv_jobs(None, [10, 3], [4], [0])
    with pytest.raises(api.FloError, match="unknown mode"):
        api._conv_jobs(None, [], [4], 0, "same")


def test_the_models_refusals_follow_the_order_of_the_checks():
    src, irs = [1000, 0, 10], [5, 0, 70, 70000]
    assert M.refusal(src, 2, irs, 1, [M.job(0, 0, 5)]) is None
    assert M.refusal(src, 2, irs, 1, [M.job(0, 0, 5)], same_rate=False) == "sample_rate"
    assert M.refusal(src, 9, irs, 1, []) == "channels" and M.refusal(src, 4, irs, 2, []) == "ir_channels"
    assert M.refusal(src, 2, irs, 1, [M.job(3, 9, 5, reserved=1)]) == "clip" and M.refusal(src, 2, irs, 1, [M.job(0, 4, 5, reserved=1)]) == "ir"
    assert M.refusal(src, 2, irs, 1, [M.job(0, 3, 5, reserved=1)]) == "reserved" and M.refusal(src, 2, irs, 1, [M.job(0, 3, 5)]) == "taps"
    assert M.refusal(src, 2, irs, 1, [M.job(0, 3, 5, taps=65536)]) is None and M.refusal(src, 2, irs, 1, [M.job(0, 3, 5, ir_start=4464)]) is None
    assert M.refusal(src, 2, irs, 1, [M.job(0, 0, 5, skip=2 ** 64 - 5)]) == "frames + skip"
    assert M.refusal(src, 2, irs, 1, [M.job(0, 0, (2 ** 64 - 1) // 16 + 1)]) == "frames"
    assert M.refusal(src, 2, irs, 1, [M.job(0, 0, 1 << 45)]) == "tiles"


def test_cli_knows_the_commands():
    from flo_amd import cli
    assert cli.filter_options(lowpass=4000) == ("lowpass", None, 4000.0) and cli.filter_options(highpass=80.5) == ("highpass", 80.5, None)
    assert cli.filter_options(bandpass="300,3400") == ("bandpass", 300.0, 3400.0) and cli.filter_options(bandstop=(49, 51)) == ("bandstop", 49.0, 51.0)
    for kw in ({}, dict(lowpass=1, highpass=2), dict(bandpass="300"), dict(bandstop="1,2,3")):
        with pytest.raises(ValueError):
            cli.filter_options(**kw)
    with pytest.raises(SystemExit):
        cli.main(["filter", "a.wav", "b.wav"])                                   # a kind is required
    with pytest.raises(SystemExit):
        cli.main(["filter", "a.wav", "b.wav", "--lowpass", "1", "--highpass", "2"])   # and only one
    with pytest.raises(SystemExit):
        cli.main(["convolve", "a.wav", "ir.wav"])                                # the output is required
    from flo_amd.wav import write_wav_bytes
    a, slow = write_wav_bytes(np.zeros(8, np.float32), 48000, 1), write_wav_bytes(np.zeros(8, np.float32), 44100, 1)
    wide = write_wav_bytes(np.zeros(8, np.float32), 48000, 2)
    with pytest.raises(ValueError, match="resample"):     # refused before any device is touched
        cli.convolve_wavs(a, slow)
    with pytest.raises(ValueError, match="edit"):
        cli.convolve_wavs(a, wide)
    with pytest.raises(Exception, match="f_hi"):
        cli.filter_wav(a, "lowpass", None, 30000.0)
