"""analysis_model pinned to the native geometry and to the sources, the oracle's block-energy references, and the reach
table of the analysis paths (no GPU needed).

1. tests/native/analysis_plan_test.cpp, built with g++ and the sanitizers, passes its own cases; its dump equals
   analysis_model.geometry / items / workgroups on a sweep of rates, channel counts, lengths around every threshold and
   peak rates - the integers and, bit for bit, the filter coefficients, M^L and the true-peak taps.
2. The constants the model restates equal the ones in the sources.
3. Every path of analysis_model.PATHS has a case; what has none is named in analysis_model.NOT_REACHED, with the reason.
4. flo_o_integrated_lufs, now built on flo_o_block_energies, is unchanged bit for bit; the long-double twin lies within
   a few 1e-14 of it; flo_o_loudness_range gives the range of flo_o_loudness_metrics.
5. The conditions the GPU tests' bounds rest on hold for every case: no block energy within 1e-9 of a gate; the chained
   sum of squares must walk at most 5 % of the chunks (but for the stalled sum).
"""
import os
import re
import subprocess

import numpy as np
import pytest

import analysis_model as M
import signals
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flo_amd", "csrc")
REQUIRED = [p for group in M.PATHS.values() for p in group]


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("analysis_plan") / "analysis_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "analysis_plan_test.cpp"), os.path.join(CSRC, "analysis_plan.cpp")], check=True)
    return exe


def test_analysis_plan_native(plan_exe):
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("ok"), r.stdout


def _sweep():
    lengths = [1, 2, 255, 256, 257, 341, 342, 343, 512, 513, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 65535, 65536, 65537, 76799, 76800, 76801,
               81920, 81921, 140000, 153599, 153600, 153601, 524287, 524288, 524289, 2097151, 2097152, 2097153, 8388607, 8388608, 8388609]
    out = []
    for sr in (2000, 3400, 4000, 8000, 11025, 16000, 22050, 44100, 48000, 96000, 192000):
        for ch in (1, 2, 3, 6, 64, 65, 255):
            for fr in lengths:
                if fr * ch > 9_000_000 and not (ch == 1 or fr <= 153601):
                    continue
                for extra in ((0, ch - 1) if ch > 1 else (0,)):
                    for pps in (1, 50, 200, 100000):
                        if pps != 50 and (fr > 153601 or ch > 3):
                            continue
                        out.append((fr * ch + extra, sr, ch, pps))
    out += [(c["n"], c["sr"], c["ch"], c["pps"]) for c in M.cases()]
    return out


def test_model_geometry_equals_the_native_dump(plan_exe):
    sweep = _sweep()
    r = subprocess.run([plan_exe, "dump"], input="".join("%d %d %d %d\n" % s for s in sweep), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(sweep)
    for s, line in zip(sweep, lines):
        head, it, wg, fl = (part.split() for part in line.split("|"))
        mh, mi, mw, mf = M.dump_line(M.geometry(*s))
        assert [int(v) for v in head] == mh, (s, head, mh)
        assert [int(v) for v in it] == mi and [int(v) for v in wg] == mw, (s, it, mi, wg, mw)
        fl = [float.fromhex(v) for v in fl]   # (M^L of an unstable filter overflows: NaN must meet NaN)
        assert len(fl) == len(mf) and all(M.same_float(a, b) for a, b in zip(fl, mf)), (s, [(i, a, b) for i, (a, b) in enumerate(zip(fl, mf)) if not M.same_float(a, b)][:4])


def test_model_constants_equal_the_sources():
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("analysis_plan.hpp", "analysis_plan.cpp", "analysis_device.hpp", "analysis_batch_kernels.hip")}

    def const(f, name):
        return int(re.search(r"constexpr int %s = (\d+);" % name, src[f]).group(1))

    assert const("analysis_plan.hpp", "kAnTile") == M.TILE
    assert const("analysis_device.hpp", "kAnHalo") == M.HALO
    assert const("analysis_device.hpp", "kSqChunk") == M.SQ_CHUNK
    assert const("analysis_batch_kernels.hip", "kKwStep") == M.KW_STEP
    fast = re.search(r"return frames > (\d+) && hop && ch <= (\d+) && !getenv", src["analysis_plan.cpp"])
    assert (int(fast.group(1)), int(fast.group(2))) == (M.EXACT_FRAMES, M.MAX_FAST_CHANNELS)
    assert re.search(r"A\.seg_frames = (\d+)u > 8u \* A\.hop", src["analysis_plan.cpp"]).group(1) == str(M.EXACT_FRAMES)
    assert "A.sq_seg = 1u << 16;" in src["analysis_plan.cpp"] and M.EXACT_FRAMES == 1 << 16
    per = re.search(r"constexpr unsigned an_batch_per_wg\(int L\) \{\s*return (.*?);\s*\}", src["analysis_plan.hpp"], re.S).group(1)
    table = {m.group(1): int(m.group(2)) for m in re.finditer(r"L == kAnl(\w+) \? (\d+)u", per)}
    assert per.strip().endswith(": 1u") and {k.lower(): v for k, v in table.items()} == M.PER_WG
    enum = re.search(r"enum AnList : int \{(.*?)kAnlCount", src["analysis_plan.hpp"], re.S).group(1)
    assert tuple(n.lower() for n in re.findall(r"kAnl(\w+),", enum)) == M.LISTS
    # the taps and halo of the true-peak FIR, the 100 ms hop, the 1 KiB chunk of the hash
    assert "for (int i = 0; i < 49; i++)" in src["analysis_plan.cpp"] and 2 * M.HALO + 1 == 49


@pytest.fixture(scope="module")
def reach():
    table = {}
    for c in M.cases():
        for p in M.paths(M.geometry(c["n"], c["sr"], c["ch"], c["pps"])):
            table.setdefault(p, []).append(c["name"])
    return table


def test_every_named_path_has_a_case(reach):
    for group, names in M.PATHS.items():
        for p in names:
            print(f"{group:15s} {p:32s} {len(reach.get(p, [])):3d}  {'; '.join(reach.get(p, [])[:2])}")
    assert len(set(REQUIRED)) == len(REQUIRED)
    assert not [p for p in reach if p not in REQUIRED], "a predicate value outside the table"
    not_reached = [p for p in REQUIRED if not reach.get(p)]
    assert sorted(not_reached) == sorted(M.NOT_REACHED), (not_reached, "against the list of paths that cannot be reached")
    names = [c["name"] for c in M.cases()]
    assert len(set(names)) == len(names)


def test_the_older_inputs_reach_few_of_them(reach):
    # what tests/test_gpu_analysis.py and tests/test_gpu_batch_analysis.py feed the analysis, by geometry alone
    old = set()
    for sr, ch, frames in ((44100, 2, 3 * 44100 + 17), (8000, 1, 20000), (22050, 3, 30001), (96000, 6, 50000), (44100, 2, int(12.3 * 44100)),
                           (96000, 1, 480000), (8000, 2, 320000), (44100, 2, 180 * 44100 + 13), (48000, 1, int(48000 * 61.7) + 13),
                           (8000, 3, int(8000 * 33.3) + 13), (192000, 2, int(192000 * 4.1) + 13), (16000, 1, 65537), (44100, 2, 40 * 44100), (44100, 2, 200), (44100, 2, 1),
                           (44100, 2, 65536), (16000, 1, 200)) + tuple((16000, 1, n) for n in (253, 254, 255, 509, 510, 511, 1021, 1022)):
        old |= M.paths(M.geometry(frames * ch, sr, ch, 50))
    missed = [p for p in REQUIRED if p not in old and p not in M.NOT_REACHED]
    print("paths the older inputs miss:", missed)
    for p in ("kseg=2048", "kq_slots=over_3", "max_edges=6", "kw=warmup", "ch=over_64", "one_walk=over_65536_frames", "b3_chunks=128"):
        assert p in missed and reach.get(p), p


# ---- the oracle's references ---------------------------------------------------------------------------------------------
def _oracle_inputs():
    rng = np.random.default_rng(5)
    yield signals.music_like(44100, 3 * 44100 + 17, 2, seed=1), 2, 44100
    yield signals.music_like(8000, 90000, 1, seed=2), 1, 8000
    yield signals.music_like(22050, 30001, 3, seed=3), 3, 22050
    yield np.zeros(88200, np.float32), 2, 44100
    yield rng.uniform(-4, 4, 2 * 30000).astype(np.float32), 2, 48000
    yield np.array([0.25, -0.5], np.float32), 2, 44100
    yield np.array([0.1, np.nan, -np.inf, 0.2] * 3000, np.float32), 2, 44100
    yield M.case("burst across both at once")["make"](), 2, 8000
    yield np.zeros(0, np.float32), 2, 44100


def test_block_energies_leave_the_oracle_loudness_unchanged():
    worst = 0.0
    for x, ch, sr in _oracle_inputs():
        en, ld = O.block_energies(x, ch, sr), O.block_energies(x, ch, sr, long_double=True)
        m = O.loudness_metrics(x, ch, sr)   # (its own K-weighting and block loop, untouched by the refactoring)
        assert M.same_float(O.integrated_lufs(x, ch, sr), m["integrated_lufs"])
        if en.size:
            assert M.same_float(O.gated_lufs(en), m["integrated_lufs"])
        assert M.same_float(O.loudness_range(en), m["loudness_range_lu"])
        g = M.geometry(x.size, sr, ch, 50)
        assert en.size == ld.size == (g["n_blocks"] if x.size else 0)
        ok = np.isfinite(en) & (en >= M.ABS_GATE)
        assert np.array_equal(np.isnan(en), np.isnan(ld))
        if ok.any():
            worst = max(worst, float(np.max(np.abs(en[ok] - ld[ok]) / ld[ok])))
    print("largest relative distance of the f64 block energies from the long-double twin's:", worst)
    assert 0.0 < worst < 1e-12


# ---- the conditions the GPU tests' bounds rest on -----------------------------------------------------------------------
@pytest.mark.parametrize("family", ["kw", "burst", "nonfinite", "peak", "sumsq", "b3", "fft", "wave"])
def test_no_block_energy_sits_on_a_gate(family):
    worst = 0.0
    for c in M.cases():
        if c["family"] != family:
            continue
        e = M.expected(c)
        assert e["gates_ok"], c["name"]
        worst = max(worst, e["E"])
        if family in ("kw", "burst"):
            assert e["n_gated"] >= 1, c["name"]
    print(f"{family}: largest E {worst:.3e}")
    assert worst < 1e-12   # the f64 oracle itself is this close to its twin: the bound is no blanket allowance


def test_sum_of_squares_cases_take_the_fast_paths():
    for c in M.cases():
        if c["family"] != "sumsq":
            continue
        x = c["make"]()
        r = M.sumsq_chain(x)
        share = len(r["must_walk"]) / r["chunks"]
        print(f"{c['name']}: {r['chunks']} chunks, {len(r['must_walk'])} must be walked ({100 * share:.2f} %): "
              f"{sorted(set(r['must_walk'].values()))}")
        assert 0 in r["must_walk"]
        if not c.get("stalled"):
            assert share <= 0.05, c["name"]
        if "16-bit" in c["name"]:   # the material the chain's parity automaton is there for: ties among the increments
            ties = M.sumsq_ties(x)
            print(f"    {ties} additions are rounding ties")
            assert ties > 100, (c["name"], ties)   # (each is a coin toss for a chain that ignores the parity of S)
    st = M.sumsq_chain(M.case("a sum that stalls: loud, then terms below half an ulp")["make"]())
    assert st["result"] == np.cumsum(M.case("a sum that stalls: loud, then terms below half an ulp")["make"]()[:200_000] ** 2, dtype=np.float32)[-1]
