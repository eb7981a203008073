"""The host side of sample-rate conversion on CPU: flo_amd/csrc/resample_plan.cpp against the cases of
tests/native/resample_plan_test.cpp (built here with g++, sanitizers on); the filter table flo_resample_filter returns
against a numpy f64 evaluation of its definition; the definition itself against analytic sines; the new symbols in the
header, the export list and the Python package. None of this needs a device."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RESAMPLE_SYMBOLS = ["flo_resample_filter", "flo_resample_out_frames", "flo_batch_resample", "flo_resample"]
PAIRS = [(48000, 44100), (44100, 48000), (96000, 44100), (8000, 44100), (44100, 8000), (44100, 22050), (22050, 44100), (48000, 48000)]
REJECTED = [(44100, 44101, "L"), (384000, 8000, "taps")]
RHO, BETA, ZEROS = 0.91, 9.0, 32.0


def ref_filter(in_rate, out_rate):
    """the definition, in numpy f64: (L, M, T, h[L][T] as f64, rows normalised to a sum of 1)"""
    g = math.gcd(in_rate, out_rate)
    L, M = out_rate // g, in_rate // g
    c = min(1.0, L / M)
    W = ZEROS / c
    T = 2 * (32 if L >= M else -((-32 * M) // L))
    k = np.arange(T, dtype=np.float64)[None, :]
    p = np.arange(L, dtype=np.float64)[:, None]
    d = (k - T // 2 + 1) - p / L
    u = d / W
    inside = np.abs(u) <= 1.0
    h = RHO * c * np.sinc(RHO * c * d) * np.i0(BETA * np.sqrt(np.where(inside, 1.0 - u * u, 0.0))) / np.i0(BETA)
    h = np.where(inside, h, 0.0)
    return L, M, T, h / h.sum(axis=1, keepdims=True)


def ref_resample(x, in_rate, out_rate, h=None):
    """one channel through the definition in f64: y[j] = sum_k h[p][k] x[i + k - T/2 + 1], x zero outside the clip"""
    L, M, T, hd = ref_filter(in_rate, out_rate)
    h = hd if h is None else np.asarray(h, np.float64)
    n_in = x.size
    n_out = -((-n_in * L) // M)
    j = np.arange(n_out, dtype=np.int64)
    i, p = (j * M) // L, (j * M) % L
    xp = np.concatenate([np.zeros(T, np.float64), x.astype(np.float64), np.zeros(T + M, np.float64)])
    idx = (i - T // 2 + 1 + T)[:, None] + np.arange(T)[None, :]
    return (h[p] * xp[idx]).sum(axis=1)


def test_resample_plan_native(tmp_path):
    exe = str(tmp_path / "resample_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "resample_plan_test.cpp"),
                    os.path.join(ROOT, "flo_amd", "csrc", "resample_plan.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.startswith("ok"), r.stdout


@pytest.mark.parametrize("in_rate,out_rate", PAIRS)
def test_filter_table_is_the_definition(in_rate, out_rate):
    """Both sides evaluate the definition in f64 to about 1e-15 relative, except sin near its zeros, where the error is
    absolute and about 1e-16: after rounding to f32 they differ by at most one f32 ulp of the reference (+ 2^-40)."""
    import flo_amd
    info, table = flo_amd.resample_filter(in_rate, out_rate)
    L, M, T, h = ref_filter(in_rate, out_rate)
    assert (info["L"], info["M"], info["taps"]) == (L, M, T)
    assert info["tile_outputs"] >= L and info["tile_outputs"] % L == 0
    assert table.shape == (L, T) and table.dtype == np.float32
    ulp = np.spacing(np.abs(h).astype(np.float32)).astype(np.float64)
    err = np.abs(table.astype(np.float64) - h)
    worst = float((err - ulp).max())
    print(f"{in_rate}->{out_rate}: max |table - ref| = {err.max():.3e}, worst excess over one ulp = {worst:.3e}")
    assert np.all(err <= ulp + 2.0 ** -40)
    assert np.all(np.abs(table.astype(np.float64).sum(axis=1) - 1.0) <= T * 2.0 ** -24)


def test_filter_limits_name_the_quantity():
    import flo_amd
    from flo_amd import _native
    L = _native.lib()
    for a, b, word in REJECTED + [(0, 44100, "in_rate"), (44100, 384001, "out_rate"), (369000, 90090, "table")]:
        err = C.create_string_buffer(256)
        tab, info = C.c_void_p(), _native.ResampleInfo()
        assert L.flo_resample_filter(a, b, C.byref(info), C.byref(tab), err, 256) == 1 and not tab.value   # FLO_ERR_ARG
        assert word in err.value.decode(), (a, b, err.value)
        with pytest.raises(flo_amd.FloError):
            flo_amd.resample_filter(a, b)
        n = C.c_uint64(7)
        assert L.flo_resample_out_frames(a, b, 100, C.byref(n)) == 1
    assert L.flo_resample_filter(48000, 44100, None, None, None, 0) == 0


def test_out_frames():
    import flo_amd
    for a, b in PAIRS:
        g = math.gcd(a, b)
        L, M = b // g, a // g
        for n in (0, 1, M - 1, M, M + 1, 2 ** 40):
            assert flo_amd.resample_out_frames(a, b, n) == -((-n * L) // M)


@pytest.mark.parametrize("in_rate,out_rate,f_pass,f_stop", [(48000, 44100, 1000.0, 23000.0), (44100, 8000, 1000.0, 5000.0)])
def test_definition_passes_and_stops(in_rate, out_rate, f_pass, f_stop):
    """The reference alone: a tone in the pass band comes out as the analytic sine at the output instants j / out_rate
    (a timing convention off by one sample would give 0.13), a tone above the new Nyquist frequency comes out below 1e-4."""
    L, M, T, _ = ref_filter(in_rate, out_rate)
    n_in = 40 * max(T, 64) * max(1, M // L + 1)
    t_in = np.arange(n_in, dtype=np.float64) / in_rate
    y = ref_resample(np.sin(2 * np.pi * f_pass * t_in), in_rate, out_rate)
    t_out = np.arange(y.size, dtype=np.float64) / out_rate
    inner = slice(T, y.size - T)
    assert y.size - 2 * T > 200
    e_pass = float(np.abs(y - np.sin(2 * np.pi * f_pass * t_out))[inner].max())
    e_stop = float(np.abs(ref_resample(np.sin(2 * np.pi * f_stop * t_in), in_rate, out_rate))[inner].max())
    print(f"{in_rate}->{out_rate}: {f_pass:g} Hz off the analytic sine by {e_pass:.2e}; {f_stop:g} Hz comes out at {e_stop:.2e}")
    assert e_pass <= 1e-4
    assert e_stop <= 1e-4


def test_resample_symbols_are_declared_listed_and_exported():
    import flo_amd
    from flo_amd import _native, cli
    header = open(os.path.join(ROOT, "include", "flo_hip.h")).read()
    lib = _native.lib()
    for s in RESAMPLE_SYMBOLS:
        assert re.search(r"\b%s\(" % s, header), s
        assert s in _native.EXPORTS and hasattr(lib, s), s
    assert "typedef struct flo_resample_info { uint32_t L, M, taps, tile_outputs; } flo_resample_info;" in header
    for name in ("resample", "resample_many", "resample_filter", "resample_out_frames"):
        assert hasattr(flo_amd, name), name
    assert hasattr(flo_amd.Batch, "resample") and hasattr(flo_amd.Context, "resample")
    assert C.sizeof(_native.ResampleInfo) == 16
    assert hasattr(cli, "resample_wav")
