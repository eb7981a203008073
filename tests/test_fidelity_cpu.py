"""Fidelity reports without a GPU: the C ABI's structs against their ctypes and NumPy mirrors (a C snippet prints sizeof and
offsetof), the new symbols' exports, the NumPy model (tests/fidelity_ref.py) against a literal restatement of the documented
order and its edge rules, and the CLI's refusal of a WAV whose format does not match the file."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fidelity_ref as M
from conftest import EXAMPLES, ROOT

import flo_amd
from flo_amd import _native


def test_structs_match_the_c_abi(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    mirrors = {"flo_fidelity": _native.Fidelity, "flo_fidelity_block": _native.FidelityBlock}
    lines = []
    for name, cls in mirrors.items():
        lines.append(f'printf("{name} size %zu\\n", sizeof({name}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{name} {f} %zu\\n", offsetof({name}, {f}));')
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "flo_hip.h"\nint main(void) {\n' + "\n".join(lines) +
                   "\nreturn 0;\n}\n")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        s, f, v = line.split()
        got[(s, f)] = int(v)
    for name, cls in mirrors.items():
        assert got[(name, "size")] == __import__("ctypes").sizeof(cls), name
        for f, _ in cls._fields_:
            assert got[(name, f)] == getattr(cls, f).offset, (name, f)
    assert flo_amd.FIDELITY_DTYPE.itemsize == got[("flo_fidelity", "size")] == 88
    assert flo_amd.FIDELITY_BLOCK_DTYPE.itemsize == got[("flo_fidelity_block", "size")] == 32
    for f, _ in _native.Fidelity._fields_:
        assert flo_amd.FIDELITY_DTYPE.fields[f][1] == got[("flo_fidelity", f)], f
    for f, _ in _native.FidelityBlock._fields_:
        assert flo_amd.FIDELITY_BLOCK_DTYPE.fields[f][1] == got[("flo_fidelity_block", f)], f
    assert M.BLOCK_DTYPE == flo_amd.FIDELITY_BLOCK_DTYPE


def test_new_symbols_are_exported():
    L = _native.lib()
    for s in ("flo_batch_fidelity", "flo_compare"):
        assert s in _native.EXPORTS and hasattr(L, s)


def _literal_block(x, y, n_in, n_dec):
    """one block of one channel, position by position in the documented order, with Python floats (IEEE f64)"""
    lanes = []
    for l in range(64):
        s = e = t = 0.0
        for k in range(16):
            j = l + 64 * k
            if j < n_in:
                xd, yd = float(x[j]), float(y[j])
                s = s + xd * xd
                e = e + (yd - xd) * (yd - xd)
            elif j < n_dec:
                t = t + float(y[j]) * float(y[j])
        lanes.append([s, e, t])
    for o in (32, 16, 8, 4, 2, 1):
        lanes = [[a + b for a, b in zip(lanes[l], lanes[l ^ o])] for l in range(64)]
    return lanes[0]


def test_model_follows_the_documented_order():
    rng = np.random.default_rng(5)
    ch = 2
    for n_src, n_dec in ((3000, 3072), (1024, 1024), (700, 1024), (2100, 1500)):
        x = (rng.standard_normal(n_src * ch) * 0.3).astype(np.float32)
        y = (rng.standard_normal(n_dec * ch) * 0.3).astype(np.float32)
        r, blocks = M.fidelity(x, y, ch)
        cmp = min(n_src, n_dec)
        assert r["compared_frames"] == cmp and blocks.shape == (-(-cmp // 1024), ch)
        tail = [0.0] * ch
        for b in range(-(-n_dec // 1024)):
            for c in range(ch):
                xs = x.reshape(-1, ch)[1024 * b:1024 * (b + 1), c] if 1024 * b < n_src else np.zeros(0, np.float32)
                ys = y.reshape(-1, ch)[1024 * b:1024 * (b + 1), c]
                s, e, t = _literal_block(xs, ys, max(0, min(cmp - 1024 * b, 1024)), min(n_dec - 1024 * b, 1024))
                tail[c] = tail[c] + t
                if b < blocks.shape[0]:
                    assert blocks[b, c]["signal"] == s and blocks[b, c]["error"] == e, (n_src, n_dec, b, c)
        assert list(r["tail_energy"]) == tail


def test_model_edge_rules():
    ch = 1
    z = np.zeros(5000, np.float32)
    r, _ = M.fidelity(z, z, ch)                                   # silence: error 0 -> +inf, no block qualifies -> NaN
    assert r["snr_db"][0] == np.inf and np.isnan(r["seg_snr_db"][0]) and r["seg_blocks"][0] == 0
    y = np.full(5000, 0.5, np.float32)
    r, _ = M.fidelity(z, y, ch)                                   # signal 0 < error -> -inf
    assert r["snr_db"][0] == -np.inf and r["seg_blocks"][0] == 0
    x = np.full(5000, 0.5, np.float32)
    r, b = M.fidelity(x, x, ch)                                   # exact: every block at the clamp's top, 60 dB
    assert r["error"][0] == 0.0 and r["seg_snr_db"][0] == 60.0 and r["seg_blocks"][0] == 5 and list(b["n"][:, 0]) == [1024] * 4 + [904]
    r, _ = M.fidelity(x, -x, ch)                                  # error 4 x signal: -6 dB in every block
    assert abs(r["seg_snr_db"][0] - 10 * np.log10(0.25)) < 1e-12
    r, _ = M.fidelity(x, x * 1000, ch)                            # clamped at -10 dB; clipped counts |y| > 1
    assert r["seg_snr_db"][0] == -10.0 and r["clipped"][0] == 5000 and r["peak_out"][0] == np.float32(500.0)
    dec = np.concatenate([x, np.full(120, 0.25, np.float32)])     # a decoded tail past the source
    r, _ = M.fidelity(x, dec, ch)
    assert r["tail_energy"][0] == 120 * 0.0625 and r["decoded_frames"] == 5120 and r["compared_frames"] == 5000
    r2, _ = M.fidelity(np.concatenate([x, np.float32([0.9])]), np.concatenate([x, x]), 2)   # a partial frame is not compared
    assert r2["source_frames"] == 2500 and r2["compared_frames"] == 2500


def test_cli_refuses_a_wav_of_another_format(tmp_path, capsys):
    from flo_amd import cli
    from flo_amd.wav import write_wav_bytes
    flo = os.path.join(EXAMPLES, "audio_lossy.flo")
    info = flo_amd.probe_container(open(flo, "rb").read())
    wav = tmp_path / "w.wav"
    wav.write_bytes(write_wav_bytes(np.zeros(1000 * info.channels, np.float32), info.sample_rate + 1000, info.channels))
    assert cli.main(["compare", str(wav), flo]) == 1
    assert f"{info.sample_rate + 1000} Hz" in capsys.readouterr().err
    other = 1 if info.channels != 1 else 2
    wav.write_bytes(write_wav_bytes(np.zeros(1000 * other, np.float32), info.sample_rate, other))
    assert cli.main(["compare", str(wav), flo]) == 1
    assert f"{other} channels" in capsys.readouterr().err
