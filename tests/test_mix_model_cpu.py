"""tests/mix_model.py checked on the CPU: against a scalar restatement of the definition in rational arithmetic (one rounding per
FMA), against tests/edit_model.py where the two definitions meet, the order of summation, flo_amd.concat_parts against a direct
restatement, the tile classes against the library's own mix_part_in_tile (the native test's dump), and what the device cases
of tests/test_gpu_batch_mix.py reach. No device needed."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import edit_model as E
import mix_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flo_amd", "csrc")
F32 = np.float32


def _round_f32(q):
    """the rational q rounded once to f32, ties to even (finite results; an exact zero is +0.0)"""
    if q == 0:
        return F32(0.0)
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n = a / quantum
    lo = n.numerator // n.denominator
    rest = n - lo
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and lo % 2):
        lo += 1
    v = float(lo * quantum)   # exact: at most 24 bits times a power of two
    assert v <= float(M.FLT_MAX)
    return F32(-v if q < 0 else v)


def _scalar(sources, ch, parts, T):
    """the definition sample by sample"""
    out = np.zeros((T, ch), F32)
    for t in range(T):
        for c in range(ch):
            a = F32(0.0)
            for g in parts:
                x = sources[g["batch"]][g["clip"]]
                n_src = x.size // ch
                if not (g["at"] <= t < g["at"] + g["frames"] and g["start"] + (t - g["at"]) < n_src):
                    continue
                u = t - g["at"]
                v = g["frames"] - 1 - u
                k = F32(g["gain"])
                w = None
                if u < g["fade_in"]:
                    w = F32(u) / F32(g["fade_in"])
                if v < g["fade_out"]:
                    w_out = F32(v) / F32(g["fade_out"])
                    w = w_out if w is None else F32(w * w_out)
                if w is not None:
                    k = F32(k * w)
                a = _round_f32(Fraction(float(k)) * Fraction(float(x[(g["start"] + u) * ch + c])) + Fraction(float(a)))
            out[t, c] = a
    return out.reshape(-1)


def test_the_model_equals_the_scalar_definition_in_rational_arithmetic():
    rng = np.random.default_rng(17)
    cases = 0
    for _ in range(300):
        ch = int(rng.integers(1, 4))
        sources = [[(rng.standard_normal(int(n) * ch) * 10.0 ** rng.integers(-3, 4)).astype(F32) for n in rng.integers(0, 12, 2)] for _ in range(2)]
        T = int(rng.integers(0, 16))
        parts = []
        for _ in range(int(rng.integers(0, 6))):
            frames = int(rng.integers(0, 14))
            parts.append(M.part(0, int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.integers(0, 13)), frames, int(rng.integers(0, 14)),
                                float(F32(rng.choice([1.0, -1.0, 0.5, 0.3, 1e-3, 7.25]))), int(rng.integers(0, frames + 1)), int(rng.integers(0, frames + 1))))
        got, want = M.mix_clip(sources, ch, parts, T), _scalar(sources, ch, parts, T)
        assert M.same(got, want) is None, (parts, T, M.same(got, want))
        cases += bool(parts and T)
    assert cases > 150


@pytest.mark.parametrize("ch", [1, 2, 3])
def test_one_part_at_gain_one_is_the_edit_models_cut(ch):
    """this ties the two independent models together: fl32(w * x) + 0, and -0.0 becomes +0.0"""
    F = M.tile_frames(ch)
    x = E.noise(2 * F + 5, ch, 9, F)
    for g in (E.seg(0, 0, 2 * F + 5), E.seg(0, 3, F + 9, 5, 7), E.seg(0, 3, F + 9, 5, 7, 40, F), E.seg(0, F, 2 * F, 0, 0, 2 * F, 2 * F), E.seg(0, 7, 100, 1, 0, 100, 0)):
        p = M.part(0, 0, 0, g["start"], g["frames"], g["pad_head"], 1.0, g["fade_in"], g["fade_out"])
        with np.errstate(all="ignore"):
            want = E.edit(x, ch, g, ch, None) + F32(0)
        got = M.mix_clip([[x]], ch, [p], E.out_frames(g))
        assert M.same(got, want) is None, (g, M.same(got, want))
    assert (E.edit(x, ch, E.seg(0, 0, 5), ch, None).view(np.uint32) == 0x80000000).any()          # the source has a -0.0 ...
    assert not (M.mix_clip([[x]], ch, [M.part(0, 0, 0, 0, 5)], 5).view(np.uint32) == 0x80000000).any()   # ... the mix has none


def test_list_order_is_summation_order():
    src = [[np.array([1e8], F32), np.array([1.0], F32)]]
    a = M.mix_clip(src, 1, [M.part(0, 0, 0, 0, 1), M.part(0, 1, 0, 0, 1), M.part(0, 0, 0, 0, 1, 0, -1.0)], 1)
    b = M.mix_clip(src, 1, [M.part(0, 0, 0, 0, 1), M.part(0, 0, 0, 0, 1, 0, -1.0), M.part(0, 1, 0, 0, 1)], 1)
    assert a.tolist() == [0.0] and b.tolist() == [1.0]


def test_concat_parts_against_a_direct_restatement():
    import flo_amd
    rng = np.random.default_rng(4)
    for rate, ms in ((48000, 0.0), (48000, 10.0), (44100, 2.5), (8000, 1e6), (48000, 0.01)):
        for _ in range(20):
            frames = [int(n) for n in rng.integers(0, 2000, int(rng.integers(0, 6)))]
            order = [int(i) for i in rng.permutation(len(frames))][:int(rng.integers(0, len(frames) + 1))] if frames else []
            parts, T = flo_amd.concat_parts(frames, rate, ms, out=3, clips=order, batch=1)
            want_xf = int(np.floor(ms * rate / 1000.0 + 0.5))
            at, prev_xf = 0, 0
            assert len(parts) == len(order)
            for j, (p, i) in enumerate(zip(parts, order)):
                n = frames[i]
                xf = min(want_xf, n, frames[order[j + 1]]) if j + 1 < len(order) else 0
                assert p == dict(out=3, batch=1, clip=i, start=0, frames=n, at=at, gain=1.0, fade_in=prev_xf, fade_out=xf), (j, p)
                at, prev_xf = at + n - xf, xf
            assert T == (at if order else 0)
            assert M.refusal([[], frames], 1, 4, [0, 0, 0, T], parts) is None
    assert flo_amd.concat_parts([5, 6], 1000)[0] == flo_amd.concat_parts([5, 6], 1000, clips=[0, 1])[0]
    # the weights of a linear crossfade sum to (xf - 1) / xf
    parts, T = flo_amd.concat_parts([8, 8], 1000, 4.0)
    ones = [[np.ones(8, F32), np.ones(8, F32)]]
    assert M.mix_clip(ones, 1, parts, T)[4:8].tolist() == [0.75] * 4 and T == 12


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """the native test's dump mode: lines of parts in, the library's class of every tile out"""
    exe = str(tmp_path_factory.mktemp("mix_plan") / "mix_plan_dump")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "mix_plan_test.cpp"),
                    os.path.join(CSRC, "mix_plan.cpp")], check=True)

    def run(lines):
        r = subprocess.run([exe, "dump"], input="".join(lines), capture_output=True, text=True, timeout=120, check=True)
        return [[int(v) for v in row.split()] for row in r.stdout.splitlines()]
    return run


def _part_classes(ch):
    """(part, n_src, T, classes by the model) of every part of the device case whose output has frames"""
    sources, parts, T = M.device_case(ch)
    F = M.tile_frames(ch)
    rows = []
    for g in parts:
        n_src = sources[g["batch"]][g["clip"]].size // ch
        if T[g["out"]]:
            rows.append((g, n_src, T[g["out"]], M.tile_classes(g, n_src, T[g["out"]], F)))
    return rows


@pytest.mark.parametrize("ch", [1, 2, 3, 8])
def test_tile_classes_equal_the_librarys(dump, ch):
    rows = _part_classes(ch)
    F = M.tile_frames(ch)
    got = dump(["%d %d %d %d %d %d %d %d\n" % (n, g["start"], g["frames"], g["at"], g["fade_in"], g["fade_out"], T, ch) for g, n, T, _ in rows])
    assert len(got) == len(rows)
    for (g, n, T, want), row in zip(rows, got):
        assert row[0] == F and row[1] == len(want) and row[2:] == want, (g, n, T, row, want)


@pytest.mark.parametrize("ch", [1, 2, 3, 8])
def test_the_device_cases_reach_every_path(ch):
    sources, parts, T = M.device_case(ch)
    F = M.tile_frames(ch)
    assert max(x.size // ch for b in sources for x in b) <= 3 * F + 5 and max(T) <= 3 * F + 5
    seen, aligned, ragged_whole = set(), set(), 0
    for g, n, t, classes in _part_classes(ch):
        seen |= set(classes)
        for k, c in enumerate(classes):
            if c == M.WHOLE:
                aligned.add((g["start"] - g["at"]) * ch % 4)
                ragged_whole += min(F, t - k * F) * ch % 4 != 0
        if M.WHOLE in classes and M.PARTIAL in classes:
            seen.add("whole then partial")
    assert seen == {M.NONE, M.WHOLE, M.PARTIAL, "whole then partial"}
    assert aligned == {(d * ch) % 4 for d in range(4)}           # every alignment a source of ch channels can have
    assert ragged_whole > 0 or ch % 4 == 0                       # a whole part on a last tile that does not fill its units
    counts = [sum(1 for g in parts if g["out"] == k) for k in range(len(T))]
    assert {63, 64, 65, 130} <= set(counts) and 0 in counts and 0 in T
    for k in [i for i, n in enumerate(counts) if n in (63, 64, 65, 130)]:   # both rounds of the scan, and a third
        mine = [g for g in parts if g["out"] == k]
        live = [j for j, g in enumerate(mine) if M.part_in_tile(g, sources[g["batch"]][g["clip"]].size // ch, T[k], F, F) != M.NONE]
        assert live == [j for j in (0, 64, 129) if j < len(mine)]
        assert all(M.part_in_tile(g, sources[g["batch"]][g["clip"]].size // ch, T[k], 2 * F, F) == M.NONE for g in mine)
    assert {g["batch"] for g in parts} == {0, 1} and {float(g["gain"]) for g in parts} >= {1.0, -1.0, 0.0, 0.5, 1e-3}
    assert any(g["fade_in"] == M.MAX_FADE - 1 for g in parts)
    M.mix(sources, ch, parts, T, strict=True)   # no coefficient and no partial sum is a non-zero subnormal
