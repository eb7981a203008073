"""lossy_model pinned to the oracle and to the sources, and the reach table of the lossy encoder (no GPU needed).

1. The writer: for every spectra case, write_frames(O.lossy_quantize) splits back into the oracle's blobs
   (O.serialize_sparse) and scale words; for silence, where the oracle's file is exact, it is the DATA of O.encode_lossy.
2. Hand-made spectra keep a margin: every coefficient at least 1 dB from its keep threshold (psy_ref), every kept product
   c * sf at least 1e-3 from a half-integer: a device must give the oracle's integers with no exception.
3. Every path of lossy_model.PATHS outside NOT_REACHED_ALLOWED has a case; the cases take the paths they are named for.
4. The constants equal the sources'; plan_lossy as restated gives every row of tests/native/encode_plan_test.cpp.
5. The table "path, old inputs, new cases" (pytest -s; DESIGN.md section 2 holds a copy): the old inputs are lossy_cases.pcm_cases
   and the batches of test_gpu_lossy.py, by the oracle's integers and the batches' lengths.
"""
import os
import re

import numpy as np
import pytest

import flofile
import lossy_model as M
from oracle import oracle as O

REQUIRED = [p for p in M.PATHS if p not in M.NOT_REACHED_ALLOWED]


@pytest.fixture(scope="module")
def reach():
    table = M.spectra_reach()
    for p, names in M.batch_reach().items():
        table.setdefault(p, []).extend(names)
    return table


SPECTRA = M.spectra_cases() + [M.levels_spectra_case()] + M.spectra_cases_other_channels()


@pytest.mark.parametrize("name", [c[0] for c in SPECTRA])
def test_writer_equals_the_oracle_and_spectra_keep_their_margin(name):
    _, c, sr, q = next(x for x in SPECTRA if x[0] == name)
    o = O.lossy_quantize(c, sr, q)
    data, sizes = M.write_frames(o["q"], o["sf_words"])
    n_ch = c.shape[1]
    frames = M.split_frames(data, n_ch)
    assert [len(f) for f, _ in frames] == sizes and len(frames) == c.shape[0]
    for h, (f, blobs) in enumerate(frames):
        for ch in range(n_ch):
            assert blobs[ch] == O.serialize_sparse(o["q"][h, ch]), (name, h, ch)
        nch, sfw, qs = flofile.parse_transform_blob(f[10:])
        assert nch == n_ch and np.array_equal(sfw, o["sf_words"][h]) and np.array_equal(qs, o["q"][h])
    margin, frac = M.margins(c, sr, q)
    assert margin >= 1.0, (name, margin)
    assert frac >= 1e-3, (name, frac)
    # the integers are what the construction says: non-zero exactly where the spectrum is
    if name != "largest_finite_level_then_70_silent":
        assert np.array_equal(o["q"] != 0, c != 0), name


def test_largest_finite_level_has_decayed_when_the_probe_comes():
    name, c, sr, q = M.levels_spectra_case()
    o = O.lossy_quantize(c, sr, q)
    energy = float((c[0, 0].astype(np.float64) ** 2).sum())
    assert 0.9 * 3.4028234e38 < energy * 1.05 and energy < 3.4028234e38   # the largest level f32 holds, still finite
    assert (o["q"][1:71] == 0).all()
    alone = O.lossy_quantize(c[71:], sr, q)
    assert np.array_equal(o["q"][71], alone["q"][0]) and (alone["q"][0] != 0).sum() == 200


def test_writer_equals_the_oracle_file_on_silence():
    for ch, n in ((2, 5000), (2, 0), (1, 1024)):
        f = flofile.parse(O.encode_lossy(np.zeros(n * ch, np.float32), 44100, ch, 0.55))
        hops = M.hops_of(n)
        sfw = np.full((hops, ch, 25), 32768, np.uint16)     # scale factor 1.0
        data, sizes = M.write_frames(np.zeros((hops, ch, 1024), np.int16), sfw)
        assert data == f.data and sizes == [fr[2] for fr in f.toc]


def test_largest_blob_is_the_dense_vector():
    rng = np.random.default_rng(3)
    cands = [np.ones(1024, np.int16), (np.arange(1024) % 2 == 0).astype(np.int16), (np.arange(1024) % 2 == 1).astype(np.int16),
             (np.arange(1024) % 256 != 255).astype(np.int16), (np.arange(1024) % 3 != 0).astype(np.int16)]
    cands += [(rng.uniform(size=1024) < p).astype(np.int16) for p in (0.3, 0.5, 0.7, 0.9, 0.99)]
    sizes = [len(M.sparse_blob(v)) for v in cands]
    assert max(sizes) == sizes[0] == M.MAX_BLOB and sizes[1] == 2050
    assert 120 + 2 * M.MAX_BLOB + 15 <= M.kFrameCap
    # the re-deal area of the general form (1024 halfwords behind kRedealOffset) starts behind the largest channel 0
    # blob with 15 bytes pending, and ends inside the staging buffer (kFrameCap + 64 + 256 bytes)
    assert 15 + 116 + M.MAX_BLOB <= M.kRedealOffset
    assert M.kRedealOffset + 2048 <= M.kFrameCap + 64 + 256


def test_every_named_path_has_a_case(reach):
    assert len(set(M.PATHS)) == len(M.PATHS)
    for p in M.PATHS:
        print(f"{p:48s} {len(reach.get(p, [])):3d}  {', '.join(reach.get(p, [])[:3])}")
    not_reached = [p for p in M.PATHS if not reach.get(p)]
    assert sorted(not_reached) == sorted(M.NOT_REACHED_ALLOWED), not_reached
    unnamed = sorted(p for p in reach if p not in M.PATHS)
    assert not unnamed, unnamed


def test_cases_take_the_paths_they_are_named_for(reach):
    def has(path, case):
        assert case in reach.get(path, []), (path, case, reach.get(path))
    for n in (0, 1, 63, 64):
        has(f"nz:{n}", "nz_0_1_63_64")
    for n in (65, 127, 128, 129):
        has(f"nz:{n}", "nz_65_127_128_129")
    has("decline:runs_gt_126", "nz_65_127_128_129")      # 129 single values: more than kItemCap and more than 126 runs
    has("runs:126_gt_itemcap", "runs_126_127"), has("runs:127_gt_itemcap", "runs_126_127")
    for L in (255, 256, 510, 511):
        has(f"run:{L}", "run_255_256_510_511")
    has("decline:run_gt_255", "run_255_256_510_511")
    for w in ("front", "between", "behind"):
        for z in (127, 128, 129):
            has(f"zrun:{w}_{z}", "zero_runs_127_128_129")
    for a in ("item", "block", "general"):
        for b in ("item", "block", "general"):
            has(f"pair:{a}_{b}", f"pair_{a}_x")
    has("redeal:behind_largest_channel0_pend15", "largest_alternating_pend15")
    has("redeal:behind_dense_channel0", "largest_dense_pend15")
    for i in range(16):
        has(f"pend:{i}", "pend_walk_16")
    has("flush:ends_on_boundary", "pend_walk_16"), has("flush:data_multiple_of_16", "pend_walk_16")
    has("blocks:all_dead", "blocks_0_none"), has("blocks:only_0_alive", "blocks_0_none"), has("blocks:only_7_alive", "block_7_only_8000")
    has("deal:persistent", "ragged_2048"), has("deal:table_parity_flips_between_clips", "ragged_2048_g1")
    for g in range(1, 7):
        has(f"deal:g{g}", f"ragged_2048_g{g}")
    has("deal:g1", "stereo_256"), has("deal:g2", "stereo_257"), has("deal:g3", "stereo_513"), has("deal:g6", "stereo_1281")
    has("deal:pair_whose_first_claim_fails", "stereo_257")
    has("plan:chain:Mono", "auto_ch1_512"), has("plan:frames:Mono1,Mono2", "auto_ch1_511")
    has("plan:chain2q:Dirty44k", "auto_ch2_256"), has("plan:frames:Pair1,Pair2FromCoef", "auto_ch2_255")
    has("walk:h_eq_64", "scan_blocks"), has("scan:blocks_3plus", "scan_blocks_mono")
    has("compact:Fused", "compact_16_clips"), has("compact:Offsets1024", "compact_17_clips"), has("compact:Offsets256", "compact_64_clips")
    has("fused:last_chunk_full", "fused_32_frames"), has("fused:last_chunk_one_frame", "fused_33_frames")
    has("fused:front_sum_second_stride", "fused_2081_frames")
    has("off256:per_gt8", "off256_2049_frames"), has("off1024:per_gt8", "off1024_8193_frames")
    # the fused kernel's copy tail of 0 to 3 bytes: the spectra cases (one clip each, form 2) bring every residue of a frame's length
    sizes = [n for _, c, sr, q in M.spectra_cases() for n in M.write_frames(*[O.lossy_quantize(c, sr, q)[k] for k in ("q", "sf_words")])[1]]
    assert {n & 3 for n in sizes} == {0, 1, 2, 3}
    has("plan:frames:Pair1,Pair2", "handover_32769"), has("plan:frames:Pair1,Pair2FromCoef", "handover_32768")


def test_constants_equal_the_sources():
    src = M.source_constants()
    assert {k: getattr(M, k) for k in src} == src
    assert len(src) == 17


def test_plan_equals_the_rows_of_the_native_test():
    with open(os.path.join(M.ROOT, "tests", "native", "encode_plan_test.cpp")) as f:
        text = f.read()
    block = re.search(r"kRows\[\] = \{(.*?)\n\};", text, re.S).group(1)
    rows = re.findall(r'\{(\d), (\d), (\d), (\d+), (HO \+ 1|HO|\d+), ([01]), ([01]), ([01]), (D44|DANY), ([01]), "([^"]+)"\}', block)
    assert len(rows) >= 60, len(rows)
    ho = (256 << 20) // 8192
    for which, fp, ch, n, frames, ex, inc, dbg, dirty, tail, want in rows:
        tf = ho + 1 if frames == "HO + 1" else ho if frames == "HO" else int(frames)
        got = M.plan_lossy(int(which), int(fp), int(ch), int(n), tf, ex == "1", inc == "1", dbg == "1",
                           M.kDirty44k if dirty == "D44" else 0x7FFF, tail == "1")
        assert got == want, (which, fp, ch, n, frames, ex, inc, dbg, dirty, tail)


def test_level_clips_are_the_ones_measured():
    """the oracle's pattern for the clip of the issue: a band energy that overflows f32 keeps channel 0 empty to the end;
    a NaN level is forgotten (fmaxf) and frame 4 has integers again"""
    for name, ch, v, f in M.level_cases():
        if ch != 2 or name not in ("3e38_ch2", "2e19_ch2", "+inf_ch2", "nan_ch2", "3e38_f150_ch2"):
            continue
        e = M.oracle_empty_pattern(M.level_clip(ch, v, f), ch)
        assert e.shape == (M.LEVEL_FRAMES + 1, 2)
        assert not e[5:, 1].any(), name
        if name == "3e38_ch2":
            assert e[2:, 0].all() and not e[1, 0]
        elif name == "2e19_ch2":
            assert e[3:, 0].all() and not e[2, 0]
        elif name == "3e38_f150_ch2":
            assert e[150:, 0].all() and not e[5:149, 0].any()
        else:
            assert e[2, 0] and e[3, 0] and not e[4:, 0].any()


# ---------------------------------------------------------------- what the older inputs reached
def old_reach():
    """the packer paths of lossy_cases.pcm_cases (stereo ones, by the oracle's integers) and the batch paths of the batches
    of tests/test_gpu_lossy.py (by their lengths: 1 to 6 clips of 6000 to 44,100 sample-frames, forms 1, 2, 5 and auto)"""
    import lossy_cases
    table = {}
    for name, pcm, sr, ch, q in lossy_cases.pcm_cases():
        if ch == 2:
            o = O.lossy_analyze(pcm, sr, ch, q)
            _, sizes = M.write_frames(o["q"], o["sf_words"])
            paths = set()
            for p in M.frame_paths(o["q"], sizes, sr):
                paths |= {x for x in p if not (x.startswith("blocks:one_band") and x not in M.PATHS)}
            for p in paths:
                table.setdefault(p, []).append(name)
        for which in (0, 1, 2, 5):
            for p in M.batch_paths(ch, [pcm.size // ch], which):
                table.setdefault(p, []).append(name)
    for n, lens in ((1, [44100]), (3, [6000, 20000, 44100]), (6, [6000, 9000, 12000, 20000, 30000, 44100])):
        for ch in (1, 2):
            for which in (0, 1, 2, 5):
                for p in M.batch_paths(ch, lens, which):
                    table.setdefault(p, []).append(f"batch_{n}x{ch}")
    return table


OLD_INPUTS_REACH_COUNT = 70     # of 128 (measured; the test fails if it changes)


def test_what_the_older_inputs_reached(reach):
    old = old_reach()
    n_old = sum(1 for p in REQUIRED if p in old)
    for p in M.PATHS:
        print(f"{p:48s} old {len(old.get(p, [])):3d}  new {len(reach.get(p, [])):3d}   {', '.join(old.get(p, [])[:2])}")
    print(f"old inputs reach {n_old} of {len(REQUIRED)} paths, the new cases {sum(1 for p in REQUIRED if p in reach)}")
    assert all(p in reach for p in REQUIRED)
    assert n_old == OLD_INPUTS_REACH_COUNT, n_old
