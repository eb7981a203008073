"""Fidelity reports without a GPU: the C ABI's structs against their ctypes and NumPy mirrors (a C snippet prints sizeof and
offsetof), the new symbols' exports, the NumPy model (tests/fidelity_ref.py) against a literal restatement of the documented
order and its edge rules, the non-finite rule, the named cases of the device's path tests (fidelity_cases.py), and the
CLI's refusal of a WAV whose format does not match the file."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fidelity_cases as C
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


# ---- the non-finite rule (include/flo_hip.h) and the named cases of the device's path tests (fidelity_cases.py) ----------
def _literal_report(x, y):
    """one channel, cmp = len(x) <= len(y), position by position with Python floats: the clip's sums, the maxima by the
    fmax rule (a comparison with NaN is false, so a NaN term is never taken), the dB values by the header's cases"""
    nan, inf = float("nan"), float("inf")
    cmp, s, e, pe, po, cl, seg, seg_n = len(x), 0.0, 0.0, 0.0, 0.0, 0, 0.0, 0
    for b in range(-(-cmp // 1024)):
        n = min(cmp - 1024 * b, 1024)
        sb, eb, _ = _literal_block(x[1024 * b:], y[1024 * b:], n, n)
        for j in range(1024 * b, 1024 * b + n):
            d = abs(float(y[j]) - float(x[j]))           # (inf - inf: NaN)
            pe = d if d > pe else pe
            po = abs(float(y[j])) if abs(float(y[j])) > po else po
            cl += 1 if abs(float(y[j])) > 1.0 else 0
        s, e = s + sb, e + eb
        if sb / n >= 1e-10:
            if eb == 0.0:
                v = 60.0
            elif eb != eb or sb != sb or (sb == inf and eb == inf):
                v = nan
            elif sb == inf:
                v = 60.0                      # +inf dB, clamped
            elif eb == inf:
                v = -10.0                     # -inf dB, clamped
            else:
                v = min(max(10.0 * np.log10(sb / eb), -10.0), 60.0)
            seg, seg_n = seg + v, seg_n + 1
    if e == 0.0:
        snr = inf
    elif s == 0.0:
        snr = -inf
    elif e != e or s != s or (s == inf and e == inf):
        snr = nan
    elif s == inf:
        snr = inf
    elif e == inf:
        snr = -inf
    else:
        snr = 10.0 * np.log10(s / e)
    return dict(signal=s, error=e, peak_error=np.float32(pe), peak_out=np.float32(po), clipped=cl, snr_db=snr,
                seg_snr_db=seg / seg_n if seg_n else nan, seg_blocks=seg_n)


def _same(a, b):
    a, b = np.float64(a), np.float64(b)
    return bool(a == b or (np.isnan(a) and np.isnan(b)))


@pytest.mark.parametrize("name, put", [
    ("nan_in_decode", lambda x, y: y.__setitem__(1500, np.nan)),
    ("nan_in_source", lambda x, y: x.__setitem__(10, np.nan)),
    ("plus_inf_in_decode", lambda x, y: y.__setitem__(2047, np.inf)),
    ("minus_inf_in_decode", lambda x, y: y.__setitem__(0, -np.inf)),
    ("plus_inf_in_source", lambda x, y: x.__setitem__(2100, np.inf)),
    ("minus_inf_in_source", lambda x, y: x.__setitem__(2499, -np.inf)),
    ("inf_on_both_sides", lambda x, y: (x.__setitem__(700, np.inf), y.__setitem__(700, np.inf))),
    ("nan_and_a_loud_sample", lambda x, y: (y.__setitem__(5, np.nan), y.__setitem__(6, 2.5))),
    ("all_nan_decode", lambda x, y: y.__setitem__(slice(None), np.nan)),
])
def test_model_nonfinite_rule_by_a_literal_restatement(name, put):
    rng = np.random.default_rng(8)
    x = (rng.standard_normal(2500) * 0.3).astype(np.float32)
    y = (x + rng.standard_normal(2500).astype(np.float32) * np.float32(0.01)).astype(np.float32)
    put(x, y)
    r, _ = M.fidelity(x, y, 1)
    want = _literal_report(x, y)
    for k, v in want.items():
        assert _same(r[k][0], v), (name, k, r[k][0], v)
    if name in ("nan_in_decode", "all_nan_decode"):      # the defect the device had: a NaN error is not 60 dB
        assert np.isnan(r["seg_snr_db"][0]) and r["seg_blocks"][0] == 3 and np.isnan(r["snr_db"][0])
    if name == "nan_and_a_loud_sample":                  # NaN takes no part: the maxima and the count are the other samples'
        assert r["peak_out"][0] == np.float32(2.5) and r["clipped"][0] == 1 and np.isfinite(r["peak_error"][0])
    if name == "all_nan_decode":
        assert r["peak_out"][0] == 0.0 and r["peak_error"][0] == 0.0 and r["clipped"][0] == 0


def _pair_inputs(p):
    f = p.file()
    if isinstance(f, bytes):
        return f, p.source(None)
    stand_in = f if not p.derived else np.random.default_rng(3).standard_normal(f.size).astype(np.float32)
    return f, p.source(stand_in)


@pytest.mark.parametrize("name", list(C.PAIRS))
def test_pair_cases_build_are_deterministic_and_small(name):
    p = C.PAIRS[name]
    assert set(p.there_for) <= set(C.PREDICATES) and p.there_for and 1 <= p.ch <= C.MAX_PAIR_CHANNELS
    (f, s), (f2, s2) = _pair_inputs(p), _pair_inputs(C.pair_cases()[list(C.PAIRS).index(name)])
    assert s.dtype == np.float32 and s.tobytes() == s2.tobytes()
    assert s.size <= C.MAX_PAIR_BLOCKS * 1024 * p.ch
    if isinstance(f, bytes):
        assert f == f2 and p.forms == ("ready",) and flo_amd.probe_container(f).channels == p.ch
    else:
        assert f.dtype == np.float32 and f.tobytes() == f2.tobytes() and "ready" not in p.forms
        assert f.size % p.ch == 0 and f.size <= C.MAX_PAIR_BLOCKS * 1024 * p.ch
        if not p.derived:   # the tags that depend on lengths and on the source alone hold with the file's PCM as the decode
            w, b = M.fidelity(s, f, p.ch)
            for tag in p.there_for:
                if tag in ("in_end_zero_blocks", "nb_in_an_earlier_chunk", "empty_source", "compared_is_decoded",
                           "partial_decoded_last_block", "excluded_between_included", "partial_last_block_by_its_n",
                           "nonfinite_sums") or tag.startswith("decoded_blocks_"):
                    if "lossless" in p.forms:
                        assert C.PREDICATES[tag](w, b), tag


@pytest.mark.parametrize("name", list(C.BATCHES))
def test_batch_cases_build_are_deterministic_and_small(name):
    bc = C.BATCHES[name]
    a, b = bc.clips(), {x.name: x for x in C.batch_cases()}[name].clips()
    assert len(a) == len(b) and all(x.dtype == np.float32 and x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert sum(x.size for x in a) <= C.MAX_BATCH_FLOATS and set(bc.there_for) <= set(C.BATCH_PREDICATES) and bc.there_for
    ws = [M.fidelity(x, x, bc.ch)[0] for x in a]          # lengths and sources: the clip as its own decode
    if name != "nonfinite_batch":                          # (that one's tag is about the sums of a real decode too)
        for tag in bc.there_for:
            assert C.BATCH_PREDICATES[tag](ws, bc.ch), tag
    if name.startswith("channels_"):
        assert any(x.size % bc.ch for x in a)
    if name == "many_short":
        assert [x.size // 2 for x in a] == [C.many_short_frames(i) for i in range(C.MANY)]


def test_threshold_blocks_qualify_exactly_the_intended_blocks():
    """which blocks qualify depends on the source alone: from the model's own block sums, against the intended pattern"""
    src = C.threshold_source()
    _, blocks = M.fidelity(src, np.zeros((C.THRESHOLD_BLOCKS + 1) * 2048, np.float32), 2)
    assert blocks.shape == (C.THRESHOLD_BLOCKS + 1, 2) and list(blocks["n"][:, 0]) == [1024] * C.THRESHOLD_BLOCKS + [C.THRESHOLD_LAST]
    q = blocks["signal"] / blocks["n"] >= C.SEG_FLOOR
    want = np.array([[(b + c) % 2 == 1 for c in range(2)] for b in range(C.THRESHOLD_BLOCKS)] + [[True, True]])
    assert np.array_equal(q, want)
    r, _ = M.fidelity(src, np.zeros((C.THRESHOLD_BLOCKS + 1) * 2048, np.float32), 2)
    assert list(r["seg_blocks"]) == [C.THRESHOLD_BLOCKS // 2 + 1] * 2
    # the margins: no rounding of a sum can move a block across the floor
    mean = blocks["signal"] / blocks["n"]
    assert np.all((mean < 0.85 * C.SEG_FLOOR) | (mean > 1.15 * C.SEG_FLOOR))


def test_partial_last_block_qualifies_only_by_the_division_by_its_n():
    src = C.threshold_source()
    _, blocks = M.fidelity(src, np.zeros((C.THRESHOLD_BLOCKS + 1) * 2048, np.float32), 2)
    s, n = blocks["signal"][-1], blocks["n"][-1]
    assert np.all(n == C.THRESHOLD_LAST) and np.all(s / n >= C.SEG_FLOOR) and np.all(s / 1024.0 < C.SEG_FLOOR)
    assert np.all(s / n > 10 * C.SEG_FLOOR) and np.all(s / 1024.0 < 0.5 * C.SEG_FLOOR)   # far from the floor either way
    # a model that divided by 1024 would count one block fewer per channel
    by_1024 = (blocks["signal"] / 1024.0 >= C.SEG_FLOOR).sum(axis=0)
    by_n = (blocks["signal"] / blocks["n"] >= C.SEG_FLOOR).sum(axis=0)
    assert list(by_n - by_1024) == [1, 1]
