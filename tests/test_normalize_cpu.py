"""The host side of loudness normalisation on CPU: flo_amd/csrc/normalize_plan.cpp against the cases of
tests/native/normalize_plan_test.cpp (built here with g++, sanitizers on); flo_normalize_gain and flo_normalize_lookahead
through the C ABI against the model's restatement; the new symbols in the header, the export list, the Python package and
the command line. None of this needs a device."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import normalize_model as M
import normalize_recycled  # noqa: F401  (the normalisation's entries in the recycled-memory registry)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["flo_batch_true_peak", "flo_normalize_gain", "flo_normalize_lookahead", "flo_batch_normalize", "flo_normalize"]
CSRC = os.path.join(ROOT, "flo_amd", "csrc")


def test_normalize_plan_native(tmp_path):
    exe = str(tmp_path / "normalize_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "normalize_plan_test.cpp"), os.path.join(CSRC, "normalize_plan.cpp"),
                    os.path.join(CSRC, "resample_plan.cpp")], check=True)
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
    for name in ("normalize", "normalize_many", "true_peak", "normalize_gain", "normalize_lookahead"):
        assert hasattr(flo_amd, name), name
    for name in ("normalize", "true_peaks"):
        assert hasattr(flo_amd.Batch, name), name
    assert hasattr(flo_amd.Context, "normalize") and hasattr(flo_amd.Context, "true_peak")
    assert C.sizeof(_native.NormalizeOpts) == 32 and C.sizeof(_native.NormalizeReport) == 56
    assert hasattr(cli, "normalize_wav")
    assert (_native.NORM_GAIN, _native.NORM_LIMIT) == (M.GAIN, M.LIMIT) == (0, 1)
    for word, value in (("FLO_NORM_GAIN", 0), ("FLO_NORM_LIMIT", 1), ("FLO_NORM_STATUS_SILENT", "1u"), ("FLO_NORM_STATUS_NONFINITE", "2u")):
        assert re.search(r"#define %s %s\b" % (word, value), header), word


def test_the_model_restates_the_constants():
    hpp = open(os.path.join(CSRC, "normalize_plan.hpp")).read()
    for name, value in (("kNormMaxLookahead", M.MAX_LOOKAHEAD), ("kNormThreads", M.THREADS), ("kNormMinTile", M.MIN_TILE)):
        assert re.search(r"\b%s = %d\b" % (name, value), hpp), name
    assert "kNormLdsBytes = 100 * 1024" in hpp and M.LDS_BYTES == 100 * 1024
    assert "kNormMaxScaledPeak = 0x1p100" in hpp and M.MAX_SCALED_PEAK == 2.0 ** 100
    assert "kNormGainMargin = 1.0 - 0x1p-15" in hpp and M.GAIN_MARGIN == 1.0 - 2.0 ** -15
    for A in (1, 12, 72, 576, 1024):
        assert M.lds_bytes(A) <= M.LDS_BYTES


@pytest.mark.parametrize("rate,frames", [(8000, 12), (44100, 66), (48000, 72), (192000, 288), (384000, 576)])
def test_lookahead_defaults(rate, frames):
    import flo_amd
    assert flo_amd.normalize_lookahead(rate) == frames == M.lookahead(rate)
    assert flo_amd.normalize_lookahead(rate, 1024) == 1024 and flo_amd.normalize_lookahead(rate, 1) == 1
    with pytest.raises(flo_amd.FloError, match="lookahead_frames"):
        flo_amd.normalize_lookahead(rate, 1025)


def _same(a, b):
    return (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b)) or a == b


def test_gain_through_the_abi_is_the_models():
    """flo_normalize_gain against gain_plan() on a grid: equal to the bit, the dB figures included (both sides call the C
    library's pow and log10 on the same f64 arguments)"""
    import flo_amd
    nan, inf = float("nan"), float("inf")
    n = 0
    for lufs in (-70.0, -23.0, -20.5, -14.0, -3.25, 5.0, nan, -inf):
        for peak_dbfs in (-150.0, -12.0, 0.0, nan):
            for tp in (0.0, 1e-7, 0.25, 0.8912509, 0.9, 1.7, 3e30, nan, inf):
                for mode in (M.GAIN, M.LIMIT):
                    for target, ceil_db, mx in ((-14.0, -1.0, 30.0), (-23.0, -0.1, 6.0), (-9.0, -3.0, 0.0)):
                        got = flo_amd.normalize_gain(lufs, peak_dbfs, tp, target, ceil_db, mode == M.LIMIT, mx)
                        want = M.gain_plan(lufs, peak_dbfs, tp, target, ceil_db, mode, mx)
                        assert got["status_bits"] == want["status"], (lufs, peak_dbfs, tp, mode)
                        for k in ("input_lufs", "input_true_peak_dbtp", "gain_db", "ceiling_reduction_db"):
                            assert _same(got[k], want[k]), (k, got[k], want[k], lufs, peak_dbfs, tp, mode, target)
                        assert np.float32(got["gain"]).view(np.uint32) == np.float32(want["gain"]).view(np.uint32)
                        assert got["min_gain_q24"] == M.UNITY and got["limited_frames"] == 0
                        n += 1
    assert n == 8 * 4 * 9 * 2 * 3


def test_refusals_name_the_quantity():
    import flo_amd
    for kw, word in ((dict(target_lufs=float("nan")), "target_lufs"), (dict(ceiling_dbtp=100.0), "ceiling_dbtp"), (dict(max_gain_db=-3.0), "max_gain_db"),
                     (dict(lookahead_frames=5000), "lookahead_frames")):
        with pytest.raises(flo_amd.FloError, match=word):
            flo_amd.normalize_gain(-20.0, -3.0, 0.5, **kw)
    from flo_amd import _native
    L = _native.lib()
    opts, rep, err = _native.NormalizeOpts(-14.0, -1.0, 30.0, 7, 0), _native.NormalizeReport(), C.create_string_buffer(256)
    assert L.flo_normalize_gain(-20.0, -3.0, 0.5, C.byref(opts), C.byref(rep), err, 256) == 1 and b"mode" in err.value   # FLO_ERR_ARG
    assert L.flo_normalize_gain(-20.0, -3.0, 0.1, None, C.byref(rep), None, 0) == 0 and abs(rep.gain_db - 6.0) < 1e-6   # NULL: the defaults


def test_cli_knows_the_options():
    from flo_amd import cli
    assert cli.level_options(None) is None
    assert cli.level_options(-16, -2, True) == dict(target_lufs=-16.0, ceiling_dbtp=-2.0, limit=True)
    with pytest.raises(SystemExit):
        cli.main(["normalize", "a.wav", "b.wav"])   # --lufs is required
