"""resample_model pinned to the native plan and to the sources, its FMA emulation pinned to exact rational arithmetic, and
the reach table of the sample-rate conversion's paths (no GPU needed).

1. tests/native/resample_plan_test.cpp, built with g++ and the sanitizers, still passes its own cases; its dump equals
   resample_model.plan / n_out_of / tiles_of on every coprime (M, L) with M <= 4200 and L in 1 .. 129 or one of 147, 160,
   320, 441, 640, 999, 1024, and the rejected pairs are rejected with the message word the model names.
2. The constants the model restates are the header's.
3. resample_model.fma is the correctly rounded f32 FMA: against exact rational arithmetic on 30 000 random triples and on
   triples built so that h x + acc lies 2^-30 ulp from an f32 rounding tie, on either side (where the naive f64 evaluation
   rounds twice and is wrong).
4. Every path of resample_model.PATHS has a case, or a reason in NOT_REACHED_ALLOWED; the reach of the older inputs is
   printed beside the new one.
5. No partial sum of any chain of any case is a non-zero subnormal (the one denormal clip excepted): the device comparison
   may be exact without deciding whether the hardware flushes.
"""
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import resample_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flo_amd", "csrc")
REQUIRED = [p for group in M.PATHS.values() for p in group]
GRID_L = list(range(1, 130)) + [147, 160, 320, 441, 640, 999, 1024]
GRID_N_IN = (0, 1, 2, 1000, 123457)
REJECTED = [(0, 44100, "in_rate"), (384001, 44100, "in_rate"), (44100, 0, "out_rate"), (44100, 384001, "out_rate"), (44100, 44101, "L"),
            (384000, 8000, "taps"), (1, 1025, "L"), (369000, 90090, "table"), (33, 1, "taps")]


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resample_plan") / "resample_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "resample_plan_test.cpp"), os.path.join(CSRC, "resample_plan.cpp")], check=True)
    return exe


def test_the_native_checks_still_print_ok(plan_exe):
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert re.fullmatch(r"ok \d+\n", r.stdout), r.stdout


def test_the_native_geometry_checks_hold_for_every_case_pair(plan_exe):
    """every output made exactly once, every read inside the staged span, every LDS index inside the plane: at the rate pairs
    of the cases, before any of them runs on a device"""
    pairs = sorted({(c["in_rate"], c["out_rate"]) for c in M.cases()})
    r = subprocess.run([plan_exe, "check"], input="".join("%d %d\n" % p for p in pairs), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and re.fullmatch(r"ok \d+\n", r.stdout), (r.stdout, r.stderr[-4000:])


def test_model_equals_the_native_dump_on_the_grid(plan_exe):
    grid = [(m, l) for m in range(1, 4201) for l in GRID_L if math.gcd(m, l) == 1]
    grid += [(c["in_rate"], c["out_rate"]) for c in M.cases()] + M.OLD_PAIRS + [(a, b) for a, b, _ in REJECTED]
    tail = " " + " ".join(str(n) for n in GRID_N_IN) + "\n"
    r = subprocess.run([plan_exe, "dump"], input="".join("%d %d%s" % (a, b, tail) for a, b in grid), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(grid)
    words, seen_ppw = {}, set()
    for (a, b), line in zip(grid, lines):
        P = M.plan(a, b)
        if isinstance(P, str):
            assert line.startswith("rejected: ") and P in line, (a, b, P, line)
            words[P] = words.get(P, 0) + 1
            continue
        head, clips = line.split("|")
        assert [int(v) for v in head.split()] == [P[k] for k in M.DUMP_FIELDS], (a, b, head, P)
        want = ["%d:%d" % (M.n_out_of(P, n), M.tiles_of(P, M.n_out_of(P, n))) for n in GRID_N_IN]
        assert clips.split() == want, (a, b, clips, want)
        seen_ppw.add(P["phases_per_wave"])
    print(f"{len(grid)} pairs, rejected by word: {words}, phases per wave seen: {sorted(seen_ppw)}")
    for a, b, word in REJECTED:
        assert M.plan(a, b) == word, (a, b, M.plan(a, b))
    assert seen_ppw == {1, 2, 4, 8, 16, 32, 64}
    # within the table limit the span of a single slot always fits: the plan's last refusal is never given
    assert "LDS" not in words and words.get("taps") and words.get("table")
    # what DESIGN 4.13 states
    assert [M.plan(a, b)["slots"] for a, b in ((48000, 44100), (44100, 48000), (96000, 44100), (44100, 8000))] == [61, 64, 16, 16]


def test_model_constants_equal_the_header():
    hdr = open(os.path.join(CSRC, "resample_plan.hpp")).read()

    def const(name):
        m = re.search(r"\b%s = ([^,;]+)[,;]" % name, hdr)
        assert m, name
        t = m.group(1).replace("u", "").split()   # "512", "80 * 1024", "1u << 20"
        v = int(t[0])
        for op, w in zip(t[1::2], t[2::2]):
            assert op in ("*", "<<"), (name, m.group(1))
            v = v * int(w) if op == "*" else v << int(w)
        return v

    assert const("kResampleLdsBytes") == M.LDS_BYTES
    assert const("kResampleBlock") == M.BLOCK
    assert const("kResampleTargetUnits") == M.TARGET_UNITS
    assert const("kResampleThreads") == M.THREADS
    assert const("kResampleFrameBytes") == M.FRAME_BYTES
    assert (const("kResampleMaxRate"), const("kResampleMaxPhases"), const("kResampleMaxTaps"), const("kResampleMaxTableBytes")) == \
        (M.MAX_RATE, M.MAX_PHASES, M.MAX_TAPS, M.MAX_TABLE_BYTES)


# ---- the FMA emulation -----------------------------------------------------------------------------------------------------
def _round_f32(v):
    """the Fraction v rounded to the nearest f32, ties to even (finite range), as a Python float"""
    if v == 0:
        return 0.0
    s, v = (-1.0 if v < 0 else 1.0), abs(v)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1
    assert Fraction(2) ** e <= v < Fraction(2) ** (e + 1)
    e = max(e, -126)
    q = v / Fraction(2) ** (e - 23)
    n, rem = divmod(q.numerator, q.denominator)
    if 2 * rem > q.denominator or (2 * rem == q.denominator and n & 1):
        n += 1
    return s * math.ldexp(float(n), e - 23)


def _exact_fma(h, x, a):
    return np.array([_round_f32(Fraction(float(p)) * Fraction(float(q)) + Fraction(float(r))) for p, q, r in zip(h, x, a)], np.float32)


def _naive(h, x, a):
    return (h.astype(np.float64) * x.astype(np.float64) + a.astype(np.float64)).astype(np.float32)


def test_fma_is_exact_on_random_triples():
    rng = np.random.default_rng(1)
    n = 30000
    h = (rng.uniform(-1, 1, n) * 2.0 ** rng.integers(-30, 1, n)).astype(np.float32)
    x = rng.uniform(-1, 1, n).astype(np.float32)
    a = (rng.uniform(-1, 1, n) * 2.0 ** rng.integers(-30, 1, n)).astype(np.float32)
    a[:200] = 0
    x[200:400] = 0
    h[400:500] = np.float32(2.0 ** -100)   # products deep in the f32 subnormal range
    x[400:500] *= np.float32(2.0 ** -30)
    a[400:450] = 0
    a[450:500] = (rng.uniform(-1, 1, 50) * 2.0 ** -128).astype(np.float32)
    got, want = M.fma(h, x, a), _exact_fma(h, x, a)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    print("random triples on which the naive f64 evaluation differs:", int((_naive(h, x, a).view(np.uint32) != want.view(np.uint32)).sum()))


def _tie_triples(n, rng):
    """h x = ((2 m + 1) 2^29 + s) units and acc = A 2^30 units with 2^23 <= A + m < 2^24 - 1: the sum lies 2^-30 ulp above
    (s = 1) or below (s = -1) the middle of two f32 values"""
    out = []
    while len(out) < n:
        s = 1 if len(out) % 2 else -1
        H = int(rng.integers(1 << 22, 1 << 23)) * 2 + 1
        X = ((1 << 29) + s) * pow(H, -1, 1 << 30) % (1 << 30)
        if not (1 << 23) <= X < (1 << 24):
            continue
        m = (H * X) >> 30
        assert H * X == ((2 * m + 1) << 29) + s
        A = int(rng.integers((1 << 23) - m, (1 << 24) - m - 1))
        sign = -1.0 if len(out) % 4 >= 2 else 1.0
        k = int(rng.integers(-40, 20))
        out.append((sign * math.ldexp(H, k - 40), math.ldexp(X, -k - 14), sign * math.ldexp(A, 30 - 54), s))
    return out


def test_fma_is_exact_next_to_rounding_ties():
    t = _tie_triples(400, np.random.default_rng(2))
    h, x, a = (np.array([v[i] for v in t]) for i in range(3))
    assert np.array_equal(h.astype(np.float32).astype(np.float64), h) and np.array_equal(x.astype(np.float32).astype(np.float64), x)
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    h, x, a = h.astype(np.float32), x.astype(np.float32), a.astype(np.float32)
    want = _exact_fma(h, x, a)
    got = M.fma(h, x, a)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the sum needs 55 bits: f64 rounds it onto the tie, and the second rounding goes to even whatever the side
    up = np.abs(want.astype(np.float64)) > np.abs(a.astype(np.float64) + h.astype(np.float64) * x.astype(np.float64))
    side = np.array([v[3] for v in t]) > 0
    assert np.array_equal(up, side), "above the tie rounds up in magnitude, below it rounds down"
    wrong = int((_naive(h, x, a).view(np.uint32) != want.view(np.uint32)).sum())
    print(f"tie triples on which the naive f64 evaluation is wrong: {wrong} of {len(t)}")
    assert wrong > len(t) // 4


def test_fma_carries_signed_zeros_infinities_and_nan():
    f = np.float32
    h = np.array([0.5, -0.5, 0.5, 0.0, 0.5, 0.5, -0.5, 0.0], f)
    x = np.array([-0.0, -0.0, 0.0, np.inf, np.inf, np.nan, np.inf, -0.0], f)
    a = np.array([0.0, 0.0, -0.0, 1.0, 1.0, 1.0, np.inf, -0.0], f)
    got = M.fma(h, x, a)
    want = np.array([0.0, 0.0, 0.0, np.nan, np.inf, np.nan, np.nan, -0.0], f)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), got


# ---- reach -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reach():
    table = {}
    for c in M.cases():
        for p in M.case_paths(c):
            table.setdefault(p, []).append(c["name"])
    return table


def test_every_named_path_has_a_case(reach):
    old = M.old_paths()
    print("%-16s %-46s %-4s %s" % ("group", "path", "old", "new"))
    for group, names in M.PATHS.items():
        for p in names:
            print("%-16s %-46s %-4s %3d  %s" % (group, p, "yes" if p in old else "-", len(reach.get(p, [])), "; ".join(reach.get(p, [])[:2])))
    assert len(set(REQUIRED)) == len(REQUIRED)
    assert not [p for p in reach if p not in REQUIRED] and not [p for p in old if p not in REQUIRED], "a predicate value outside the table"
    not_reached = [p for p in REQUIRED if not reach.get(p)]
    assert sorted(not_reached) == sorted(M.NOT_REACHED_ALLOWED), (not_reached, "against the list of paths that cannot be reached")
    assert all(len(reason) > 20 for reason in M.NOT_REACHED_ALLOWED.values())
    names = [c["name"] for c in M.cases()]
    assert len(set(names)) == len(names)
    missed = [p for p in REQUIRED if p not in old and p not in M.NOT_REACHED_ALLOWED]
    print(f"{len(REQUIRED)} paths, the older inputs reach {len([p for p in REQUIRED if p in old])}, the cases {len(REQUIRED) - len(not_reached)}")
    for p in ("phases_per_wave=2", "phases_per_wave=64", "uniform_idle_lanes=31", "plane_uniform_last_pass=one_plane_behind_pairs",
              "plane_side_pass=two_planes", "uniform_L=3", "L=1024", "taps=2048", "shift=7_or_more", "batch=over_512_clips",
              "value=nan_first_frame", "windows=24_or_more_apart"):
        assert p in missed, p


def test_cases_are_small_and_say_what_they_are_for():
    for c in M.cases():
        P = c["plan"]
        assert c["why"] and isinstance(P, dict)
        for name, x in c["clips"]:
            n_out = M.n_out_of(P, x.size // c["ch"])
            assert M.tiles_of(P, n_out) <= 4, (c["name"], name, "a clip holds a few tiles")
            lane = M.lane_of(P, max(n_out - 1, 0))
            assert lane["slot"] < P["slots"] and lane["lane"] < 64 and lane["unit"] < P["units"], (c["name"], name, lane)


def test_no_partial_sum_is_subnormal():
    """on every clip but the denormal ones; those are held to the f64 bound alone on the device"""
    import flo_amd
    for c in M.cases():
        _, table = flo_amd.resample_filter(c["in_rate"], c["out_rate"])
        for name, x in c["clips"]:
            y, sub = M.chain(c["plan"], table, x, c["ch"])
            assert y.size == M.n_out_of(c["plan"], x.size // c["ch"]) * c["ch"]
            if M.is_denormal_clip(x):
                assert sub, (c["name"], name, "the denormal clip makes subnormal partial sums")
            else:
                assert not sub, (c["name"], name)
