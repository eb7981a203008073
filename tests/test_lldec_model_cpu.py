"""The parallel lossless decoder's model (tests/lldec_model.py) on the CPU:

1. model against the oracle: for every case the integers the model assembles - tile tables, chain, per-tile emission,
   predictor - equal O.decode_lossless_i32, the residuals of every Rice wrapper equal O.rice_decode_i32, and the floats
   of the model's finish equal O.decode bit for bit. This is the kernel header's claim that zero padding stands in for
   the reader's end-of-stream rules, checked before any GPU run;
2. tests/native/decode_plan_test.cpp, built with g++ and the sanitizers, passes its own checks of ll_route and
   LlWrapperList, and its dump of a sweep over every limit of ll_route equals the model line for line;
3. the constants the model restates are the sources';
4. every path of PATHS is reached by a case or named in NOT_REACHED with its reason, never both;
5. the conditions tests/test_gpu_lldecode_paths.py rests on: handovers by escape, by a sample's overflow and by run-on
   only, and cases one step short of each that hand nothing over."""
import os
import re
import subprocess

import numpy as np
import pytest

import lldec_model as M
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flo_amd", "csrc")
NAMES = [c["name"] for c in M.cases()]


# ---- 1. the model against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_model_equals_oracle(name):
    c = M.case(name)
    d = c["model"]
    oi, _, och = O.decode_lossless_i32(c["flo"])
    assert och == d["channels"] and oi.shape == d["i32"].shape
    bad = np.nonzero(oi != d["i32"])[0]
    assert bad.size == 0, (bad[:8], d["i32"][bad[:8]], oi[bad[:8]])
    of, _, _ = O.decode(c["flo"])
    assert np.array_equal(of.view(np.uint32), d["f32"].view(np.uint32))
    for i, w in enumerate(d["list"].ws):
        if not (w["payload"] and (w["coeffs"] or w["shift"] >= 128)):
            continue
        want = O.rice_decode_i32(w["payload"], w["k"], w["samples"])
        r = d["wrappers"][i]["rice"]
        if r is None or r["escaped"]:   # the serial kernel's reader
            got = M.rice_read(w["payload"], w["k"], w["samples"])
        else:
            got = r["residuals"]
            assert None not in got, ("wrapper %d: a residual no tile writes and the chain does not clear" % i, got.index(None))
        assert np.array_equal(np.asarray(got, np.int64), want.astype(np.int64)), ("wrapper", i)
    # a case is one small file: a few hundred tiles and a few thousand samples per wrapper at the most
    assert d["list"].max_tiles <= 520 and d["list"].max_samples <= 16384 and len(c["flo"]) < 100000, (d["list"].max_tiles, d["list"].max_samples, len(c["flo"]))


def test_the_serial_reader_of_the_model_is_the_oracles():
    rng = np.random.default_rng(5)
    for k in (0, 1, 5, 14, 15, 20, 31, 33, 40):
        for payload in (bytes(rng.integers(0, 256, 300, dtype=np.uint8)), b"\xff" * 70 + bytes(rng.integers(0, 256, 50, dtype=np.uint8)), b"\xff" * 32, b""):
            want = O.rice_decode_i32(payload, k, 400)
            assert np.array_equal(np.asarray(M.rice_read(payload, k, 400), np.int64), want.astype(np.int64)), (k, len(payload))


def test_the_writer_of_the_cases_is_the_oracles():
    rng = np.random.default_rng(6)
    for k in (0, 3, 14):
        v = rng.integers(-(100 << k), 100 << k, 500)
        assert M.rice_encode(v, k) == O.rice_encode_i32(v.astype(np.int32), k)


# ---- 2. native routing ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("decode_plan") / "decode_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "decode_plan_test.cpp"), os.path.join(CSRC, "ll_route.cpp")], check=True)
    return exe


def test_decode_plan_native(plan_exe):
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.startswith("ok"), r.stdout


def _sweep():
    taps = ([], [900, -100], [M.CSUM_LIMIT - 5, 4], [-(M.CSUM_LIMIT - 4), 4], [M.CSUM_LIMIT - 1], [M.CSUM_LIMIT], [100] * 12, [1 << 18] * 8)
    for k in (0, 13, M.MAX_K, M.MAX_K + 1, 16, 255):
        for shift in (0, 19, M.SHIFT_LIMIT, M.SHIFT_LIMIT + 1, 63, 64, 64 + M.SHIFT_LIMIT, 65 + M.SHIFT_LIMIT, 127, 128, 129, 133, 128 + 84, 255):
            for ln in (0, 1, 127, 128, 129, 8192, 8193, M.LEN_CAP - 1, M.LEN_CAP, M.LEN_CAP + 1):
                for co in taps:
                    for samples in sorted({0, len(co), len(co) + 1, 1000}):
                        for force in (0, 1) if (k, shift) in ((M.MAX_K, M.SHIFT_LIMIT), (0, 129)) else (0,):
                            yield k, shift, ln, samples, force, co


def test_native_dump_equals_model(plan_exe):
    lines, want = [], []
    L = M.WrapperList()

    def flush():
        lines.append("list")
        want.append("list %d tiles %d max_tiles %d scratch %d" % (len(L.ws), L.tile0[-1], L.max_tiles, L.scratch))
        want.append((" tile0 " + " ".join(map(str, L.tile0))).rstrip())
        want.append((" others " + " ".join(map(str, L.others))).rstrip())
        want.append((" out_off " + " ".join(map(str, L.out_off))).rstrip())
        want.append((" serial " + " ".join(map(str, L.serial))).rstrip())

    n = 0
    for k, shift, ln, samples, force, co in _sweep():
        lines.append("%d %d %d %d %d %d %s" % (k, shift, ln, samples, force, len(co), " ".join(map(str, co))))
        w = M.wrapper(k, co, shift, b"", samples)
        r = M.route(w, bool(force), length=ln)
        L.push(w, r)
        want.append("%d %d %d" % r)
        n += 1
        if n % 37 == 0:
            flush()
            L = M.WrapperList()
    flush()
    seen = {(k, s) for k, s, *_ in _sweep()}
    assert {(M.MAX_K, 0), (M.MAX_K + 1, 0), (0, M.SHIFT_LIMIT), (0, M.SHIFT_LIMIT + 1), (0, 64 + M.SHIFT_LIMIT)} <= seen and n > 5000
    r = subprocess.run([plan_exe, "dump"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    got = [x.rstrip() for x in r.stdout.splitlines()]
    assert len(got) == len(want), (len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)


# ---- 3. the constants ----------------------------------------------------------------------------------------------------------
def test_constants_are_the_sources():
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("ll_route.hpp", "ll_route.cpp", "lldec_kernels.hip", "decode_kernels.hip")}

    def const(f, name):
        m = re.search(r"constexpr (?:int|unsigned|uint32_t) %s = ([^;]+);" % name, src[f])
        assert m, (f, name)
        return m.group(1).strip()

    assert const("ll_route.hpp", "kRiceTileBits") == str(M.TILE_BITS)
    assert const("ll_route.hpp", "kRiceStates") == str(M.STATES)
    assert const("ll_route.hpp", "kRiceMaxK") == "kRiceStates - 2" and M.MAX_K == M.STATES - 2
    k = src["lldec_kernels.hip"]
    assert const("lldec_kernels.hip", "kScanWaves") == str(M.SCAN_WAVES)
    assert re.search(r"#define FLO_SCAN_FRONTIER (\d+)", k).group(1) == str(M.FRONTIER)
    assert const("lldec_kernels.hip", "kScanTiles") == str(M.SCAN_GRID_TILES // M.SCAN_WAVES)
    assert "(max_tiles + kScanWaves * kScanTiles - 1) / (kScanWaves * kScanTiles)" in k
    # the frontier and the leaders, as scan_tile() restates them
    assert "while (__ballot(pos < kScanFrontier) != 0ull) step(words + row * kScanStride, pos < kScanFrontier, pos, n);" in k
    assert "const bool cand = pos < T;" in k and "if (cand && j < st && leader == st && posv[g0 + j] == pos) leader = j;" in k
    assert const("lldec_kernels.hip", "kChainChunk") == str(M.CHAIN_CHUNK)
    assert const("lldec_kernels.hip", "kDecOver") == str(M.DEC_OVER)
    assert const("lldec_kernels.hip", "kSb") == str(M.SB)
    assert "const unsigned t0 = blockIdx.y * 64u;" in k and "(max_tiles + 63) / 64" in k and M.DEC_WAVE_TILES == 64
    assert "const bool esc = !skip && (q2 >= %du || z >= limit);" % M.ESCAPE in k
    assert "const uint32_t limit = 64u * kRiceTileBits + 32u * (kDecOver - 2);" in k
    assert "if (sb >= 2u && 16u * ((uint32_t)kSb * (sb + 1u) + (uint32_t)kSb + 1u) <= nmin)" in k
    assert "const bool bad = !(worst < 2147483648.0);" in k and 2147483648 == -M.INT_MIN
    assert "if (quotient == %du) break;" % M.ESCAPE in src["decode_kernels.hip"]
    r = src["ll_route.cpp"]
    assert "csum >= (1ll << 21)" in r and M.CSUM_LIMIT == 1 << 21
    assert "(d.shift_bits & 63u) > %du" % M.SHIFT_LIMIT in r
    assert "d.len > 16u * 1024u * (unsigned)kRiceTileBits" in r and M.LEN_CAP == 16 * 1024 * M.TILE_BITS
    assert "d.n_coeffs <= 12" in r


# ---- 4. reach --------------------------------------------------------------------------------------------------------------------
def test_every_path_is_reached_or_named_with_its_reason():
    assert sorted(M.PATHS) == ["chain", "finish", "predict", "residual", "route", "scan"]
    every = [p for g in M.PATHS.values() for p in g]
    assert len(set(every)) == len(every)
    reached = {}
    for name in NAMES:
        for p in M.case(name)["paths"]:
            reached.setdefault(p, name)
    assert set(reached) <= set(every), sorted(set(reached) - set(every))
    for p in every:
        assert (p in reached) != (p in M.NOT_REACHED), (p, reached.get(p), M.NOT_REACHED.get(p))
    assert set(M.NOT_REACHED) <= set(every)
    assert all(len(v) > 20 for v in M.NOT_REACHED.values())
    assert "route:ll_decode_kernel<0>" in M.NOT_REACHED and "residual:esc_by_limit" in M.NOT_REACHED
    # every group has a case of its own (test_gpu_lldecode_paths.py takes one of each through the other wrapper lists)
    assert {c["group"] for c in M.cases()} == set(M.PATHS)


def test_a_case_reaches_what_its_name_says():
    def has(name, *paths):
        got = set(M.case(name)["paths"])
        assert set(paths) <= got, (name, sorted(set(paths) - got))

    has("route: k 14 / 15, sum of taps 2^21 - 1 / 2^21, shift 20 / 21 / 84 / 85", "route:k=14", "route:k=15", "route:csum=2^21-1", "route:csum=2^21",
        "route:shift=20", "route:shift=21", "route:shift=84")
    for k in range(M.MAX_K + 1):
        name = next(n for n in NAMES if n.startswith("scan k = %d:" % k))
        has(name, *["scan:k=%d:tiles=%s" % (k, t) for t in ("8tpw-1", "8tpw", "8tpw+1")], "scan:last_wave_partial", "scan:wave_idle_in_active_wg")
    has(next(n for n in NAMES if n.startswith("scan k = 0:")), "scan:wg_leaders>64", "scan:surplus_workgroups")
    has("chain 257 tiles, k = 14, a run over the boundary", "chain:tiles=257", "chain:run_straddles_chunk")
    has("chain 513 tiles, k = 14, a remainder over the boundary", "chain:tiles=513", "chain:code_straddles_chunk")
    has("chain 257 tiles, k = 14, a code on the boundary", "chain:chunk_starts_on_a_code")
    has("residual 63 / 64 / 65 tiles, a remainder in the words behind the 64th", "residual:tiles=63", "residual:tiles=64", "residual:tiles=65",
        "residual:code_in_the_over_words")
    has("ones: 130, 256, 300 bytes of 0xff at tile-aligned and unaligned offsets", "residual:lost", "residual:esc_by_256_ones", "residual:no_code_start")
    has("ones behind the last sample: nobody's run, no handover", "residual:lost", "residual:tile_behind_the_last_sample")
    has("cut: the stream ends inside a run exactly at a tile's end", "residual:stream_ends_in_a_run_at_a_tile_end")
    has("flush: 16 iterations, 1024 codes of one bit, fewer than 16", "residual:wave_iterations<16", "residual:wave_iterations=16",
        "residual:wave_iterations>16")
    for n in (1039, 1040, 1041, 1295, 1296, 1297):
        has("rows: one wrapper of %d samples" % n, "predict:rows_nmin=%d" % n,
            "predict:rows_unpredicated=" + ("0" if n < 1040 else "1" if n < 1296 else "2+"))
    has("rows: 500 and 3000 samples share a wavefront", "predict:rows_nmin_bars_unpredicated", "predict:rows_shorter_row_runs_on")
    has("rows: n = 255, 256, 257, one row of nine taps", "predict:rows_maxo=12_by_one_row", "predict:rows_n=255", "predict:rows_n=256", "predict:rows_n=257")
    has("rows: an idle row in front, an idle row behind, a group of none", "predict:rows_inactive_row_0", "predict:rows_inactive_row_3",
        "predict:group_without_rows", "predict:rows_last_group_partial")
    has("finish: stereo frames of 4 m + 0..3 samples in a row", "finish:vector", "finish:vector_mid_side", "finish:scalar_misaligned_scratch",
        "finish:scalar_odd_out_off", "finish:scalar_mid_side")
    has("finish: mid/side pairs that wrap, odd and negative; samples above 2^24", "finish:vector_mid_side", "finish:scalar_mid_side")


# ---- 5. what the GPU test rests on -----------------------------------------------------------------------------------------------
def test_handovers_and_the_cases_one_step_short_of_them():
    d = M.case("escape: runs of 255, 256 and 257 ones")["model"]
    flags = [w["escaped"] for w in d["wrappers"]]
    assert flags == [False, True, True] * 5 and d["device"] == 10 and d["host"] == 0   # 255 ones hand nothing over
    assert M.case("ones: 130, 256, 300 bytes of 0xff at tile-aligned and unaligned offsets")["device"] == 6
    assert M.case("ones behind the last sample: nobody's run, no handover")["device"] == 0
    cut = M.case("cut: the stream ends inside a run exactly at a tile's end")["model"]
    assert [w["escaped"] for w in cut["wrappers"]] == [False, False, True, False]   # 255 ones up to the end: a value; 300: the escape

    def group0(name):
        m = M.case(name)
        return m, m["model"]["groups"][0]["flagged"]

    m, f = group0("i32: a sample one above INT_MAX")
    assert m["device"] == 1 and f[0] == "sample" and INT_MAX_WRAPS in m["model"]["i32"]
    m, f = group0("i32: a sample one below INT_MIN")
    assert m["device"] == 1 and f[0] == "sample" and M.INT_MAX in m["model"]["i32"]
    m, f = group0("i32: a sample equal to INT_MAX")
    assert m["device"] == 0 and f[0] is None and int(m["model"]["i32"].max()) == M.INT_MAX
    m, f = group0("i32: a sample equal to -INT_MAX")
    assert m["device"] == 0 and f[0] is None and int(m["model"]["i32"].min()) == -M.INT_MAX
    # the magnitude test is symmetric: INT_MIN itself is handed over (a needless serial decode, the value is right)
    m, f = group0("i32: a sample equal to INT_MIN (handed over by magnitude)")
    assert m["device"] == 1 and f[0] == "sample" and int(m["model"]["i32"].min()) == M.INT_MIN
    m, f = group0("run-on: zeros behind the end, not the next wrapper's residuals")
    assert m["device"] == 0 and f == [None, None, None, None] and int(m["model"]["i32"].max()) == M.INT_MAX - 3023
    m, f = group0("run-on: a doubling wrapper of 20 samples alone")
    assert m["device"] == 1 and f[0] == "run-on" and int(np.abs(m["model"]["i32"]).max()) == 1 << 19
    m, f = group0("run-on: a doubling wrapper of 20 samples beside two of 900")
    assert m["device"] == 1 and f == [None, "run-on", None, None]
    # the host's count
    assert M.case("route: k 14 / 15, sum of taps 2^21 - 1 / 2^21, shift 20 / 21 / 84 / 85")["host"] == 6
    assert sum(M.case(n)["host"] for n in NAMES if not n.startswith("route:")) == 0


INT_MAX_WRAPS = M.INT_MIN   # INT_MAX + 1 as the format's wrapping add leaves it


def test_phase_two_only_adds_what_the_leader_walked():
    """the tabs of the two-phase scan equal one walk of every entry state to the tile's end (a restatement of scan_tile
    without the frontier), on random bytes and on long runs"""
    rng = np.random.default_rng(9)
    for k in (0, 1, 6, 14):
        payload = bytes(rng.integers(0, 256, 512, dtype=np.uint8)) + b"\xff" * 200 + bytes(rng.integers(0, 256, 312, dtype=np.uint8))
        s = M.bit_string(payload, 8)
        for t in range(8):
            for st, got in enumerate(M.scan_tile(s, t, k)["tabs"]):
                pos, n = (st, 1) if st <= k else (0, 0)
                while pos < M.T:
                    pos, dn = M._scan_step(s, t * M.T, pos, k)
                    n += dn
                assert got == (pos - M.T, n), (k, t, st)
