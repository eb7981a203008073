"""tests/edit_model.py checked on CPU before the device is held to it:
1. edit() equals a scalar restatement of the definition, sample by sample (rational arithmetic for the FMA steps, f32 scalars
   for the products and the divisions), on a few hundred random small cases: every mix shape, cuts that reach past the
   source, pads, fades that overlap, special values;
2. active_range() equals a scalar loop;
3. the model's tile classes equal the dump of the native plan (tests/native/edit_plan_test.cpp, built with g++ and the
   sanitizers) on a sweep around the tile boundaries;
4. the device cases reach what they claim: every alignment class, every tile class, the special values."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import edit_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flo_amd", "csrc")
F32 = np.float32


def _round_f32(v):
    """the Fraction v rounded to the nearest f32, ties to even, as an f32 (overflow to infinity)"""
    if v == 0:
        return None
    s, v = (-1.0 if v < 0 else 1.0), abs(v)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1
    e = max(e, -126)
    q = v / Fraction(2) ** (e - 23)
    n, rem = divmod(q.numerator, q.denominator)
    if 2 * rem > q.denominator or (2 * rem == q.denominator and n & 1):
        n += 1
    if n * Fraction(2) ** (e - 23) >= Fraction(2) ** 128:
        return F32(s * math.inf)
    return F32(s * math.ldexp(float(n), e - 23))


def _fma(m, x, a):
    m, x, a = float(m), float(x), float(a)
    if not (math.isfinite(m) and math.isfinite(x) and math.isfinite(a)):
        with np.errstate(all="ignore"):
            return F32(np.float64(m) * np.float64(x) + np.float64(a))   # infinities and NaN: no rounding to get wrong
    r = _round_f32(Fraction(m) * Fraction(x) + Fraction(a))
    if r is None:   # an exact zero: the sign of the sum of the product's zero and a's
        p = math.copysign(0.0, m) * math.copysign(1.0, x) if (m == 0 or x == 0) else None
        if p is not None and a == 0:
            return F32(p + a)
        return F32(0.0)
    return r


def _scalar_edit(x, cin, g, cout, matrix):
    n_src = len(x) // cin
    out = []
    for t in range(M.out_frames(g)):
        u = t - g["pad_head"]
        if u < 0 or u >= g["frames"] or g["start"] + u >= n_src:
            out += [F32(0.0)] * cout
            continue
        n = g["start"] + u
        for j in range(cout):
            if matrix is None:
                y = x[n * cin + j]
            else:
                with np.errstate(all="ignore"):
                    y = F32(matrix[j][0]) * x[n * cin]
                for i in range(1, cin):
                    y = _fma(matrix[j][i], x[n * cin + i], y)
            v = g["frames"] - 1 - u
            with np.errstate(all="ignore"):
                w_in = F32(u) / F32(g["fade_in"]) if u < g["fade_in"] else None
                w_out = F32(v) / F32(g["fade_out"]) if v < g["fade_out"] else None
                if w_in is not None and w_out is not None:
                    y = y * (w_in * w_out)
                elif w_in is not None:
                    y = y * w_in
                elif w_out is not None:
                    y = y * w_out
            out.append(F32(y))
    return np.array(out, F32)


def _random_case(rng):
    cin, cout = int(rng.integers(1, 5)), int(rng.integers(1, 5))
    matrix = None
    if rng.random() < 0.3:
        cout = cin
    else:
        matrix = rng.uniform(-2, 2, (cout, cin)).astype(F32)
        if rng.random() < 0.3:
            matrix[rng.integers(0, cout), rng.integers(0, cin)] = F32(rng.choice([0.0, -0.0, 1.0, -1.0]))
    n = int(rng.integers(0, 24))
    x = (rng.standard_normal(n * cin) * rng.choice([1.0, 1e-20, 1e20])).astype(F32)
    for _ in range(int(rng.integers(0, 4))):
        if x.size:
            x[rng.integers(0, x.size)] = F32(rng.choice(M.SPECIALS + [0.0]))
    frames = int(rng.integers(0, 30))
    g = M.seg(0, int(rng.integers(0, n + 6)), frames, int(rng.integers(0, 4)), int(rng.integers(0, 4)),
              int(rng.integers(0, frames + 1)) if rng.random() < 0.7 else 0, int(rng.integers(0, frames + 1)) if rng.random() < 0.7 else 0)
    return x, cin, g, cout, matrix


def test_model_equals_the_scalar_restatement():
    rng = np.random.default_rng(415)
    both = past = 0
    for k in range(400):
        x, cin, g, cout, matrix = _random_case(rng)
        got, want = M.edit(x, cin, g, cout, matrix), _scalar_edit(x, cin, g, cout, matrix)
        assert M.same(got, want) is None, (k, g, cin, cout, matrix, M.same(got, want))
        both += g["fade_in"] + g["fade_out"] > g["frames"] > 0
        past += g["start"] + g["frames"] > x.size // cin
    assert both > 40 and past > 40, (both, past)


def test_the_zeros_of_the_definition():
    """pads and frames past the source are +0.0 whatever the matrix; inside, m = [[1]] keeps -0.0 and m = [[-1]] turns +0.0"""
    x = np.array([0.0, -0.0, 1.0], F32)
    for m, inside in (([[1.0]], [0x00000000, 0x80000000]), ([[-1.0]], [0x80000000, 0x00000000]), (None, [0x00000000, 0x80000000])):
        got = M.edit(x, 1, M.seg(0, 0, 5, 1, 1), 1, m).view(np.uint32).tolist()
        assert got[0] == 0 and got[1:3] == inside and got[4:] == [0, 0, 0], (m, got)
    # a fade weight of 0 on a negative sample makes -0.0: the fade is a multiplication
    got = M.edit(np.array([-1.0, -1.0], F32), 1, M.seg(0, 0, 2, fade_in=2), 1, None).view(np.uint32).tolist()
    assert got == [0x80000000, np.array(-0.5, F32).view(np.uint32)]


def test_active_range_equals_a_scalar_loop():
    rng = np.random.default_rng(9)
    for k in range(300):
        ch, n = int(rng.integers(1, 4)), int(rng.integers(0, 12))
        x = (rng.standard_normal(n * ch) * 0.01).astype(F32)
        x[rng.random(x.size) < 0.6] = 0
        if x.size and rng.random() < 0.2:
            x[rng.integers(0, x.size)] = F32(np.nan)
        thr = F32(rng.choice([0.0, 0.005, 0.02, np.inf]))
        act = [f for f in range(n) if any(not (abs(x[f * ch + c]) <= thr) for c in range(ch))]
        want = (act[0], act[-1] + 1) if act else (0, 0)
        assert M.active_range(x, ch, thr) == want, (k, x, thr)
    t = F32(0.001)
    assert M.active_range(np.array([0, t, 0], F32), 1, t) == (0, 0)
    assert M.active_range(np.array([0, np.nextafter(t, F32(1)), 0], F32), 1, t) == (1, 2)
    assert M.active_range(np.array([-0.0, 0.0], F32), 1, 0.0) == (0, 0)
    assert M.active_range(np.array([0, np.nan, 0, 0], F32), 2, np.inf) == (0, 1)
    assert float(M.threshold(-60.0)) == float(F32(0.001))


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("edit_plan") / "edit_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "edit_plan_test.cpp"), os.path.join(CSRC, "edit_plan.cpp")], check=True)
    return exe


def test_tile_classes_equal_the_native_dump(plan_exe):
    sweep = []
    for cout in (1, 2, 3, 8):
        F = M.tile_frames(cout, cout)
        n = 2 * F + 5
        near = (0, 1, F - 1, F, F + 1)
        for start in (0, 3, n - 1, n, n + 5):
            for frames in (0, 1, F - 1, F, F + 1, 2 * F + 5):
                for ph in near:
                    for fi, fo in ((0, 0), (1, 1), (F - 1, 2), (F, F + 1), (F + 1, F), (frames, frames)):
                        if fi <= frames and fo <= frames:
                            sweep.append((n, start, frames, ph, (ph * 7) % (F + 2), fi, fo, cout))
    r = subprocess.run([plan_exe, "dump"], input="".join("%d %d %d %d %d %d %d %d\n" % s for s in sweep), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(sweep)
    seen = set()
    for s, line in zip(sweep, lines):
        n, start, frames, ph, pt, fi, fo, cout = s
        g = M.seg(0, start, frames, ph, pt, fi, fo)
        F = M.tile_frames(cout, cout)
        want = [F, M.tiles_of(M.out_frames(g), F)] + M.tile_classes(g, n, F)
        assert [int(v) for v in line.split()] == want, (s, line, want)
        seen |= set(want[2:])
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("name", [f[0] for f in M.FORMS])
def test_the_device_cases_reach_what_they_claim(name):
    cin, cout, matrix, clips, segs = M.form_case(name)
    F = M.tile_frames(cin, cout)
    assert [c.size // cin for c in clips] == M.source_lengths(F) and max(c.size // cin for c in clips) <= 3 * F + 5
    residues, classes, pads = set(), set(), set()
    for g in segs:
        assert M.refusal([c.size // cin for c in clips], cin, False, [g], cout, matrix) is None
        n = clips[g["clip"]].size // cin
        for t, cls in enumerate(M.tile_classes(g, n, F)):
            classes.add(cls)
            if cls == M.INTERIOR and (min(F, M.out_frames(g) - t * F) * cout >= 8):   # at least two 16-byte units
                residues.add(((g["start"] + t * F - g["pad_head"]) * cin) % 4)
        pads |= {("head", g["pad_head"]), ("tail", g["pad_tail"])}
    assert residues == {(s * cin) % 4 for s in range(4)}, residues
    assert {M.INTERIOR, M.EDGE} <= classes
    assert pads >= {(w, p) for w in ("head", "tail") for p in (0, 1, F + 3)}
    flat = np.concatenate(clips)
    assert np.isnan(flat).any() and np.isinf(flat).any() and (np.abs(flat) == M.FLT_MAX).any()
    assert ((flat != 0) & (np.abs(flat) < 2.0 ** -126)).any() and (flat.view(np.uint32) == 0x80000000).any()
    assert len(segs) < 260
