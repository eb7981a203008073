"""container_model pinned to the oracle and to the sources, and the reach table of the container finish (no GPU needed).

1. For every case the model's writer gives the oracle's header, TOC and CRC field, and zlib.crc32 of DATA is that field.
2. Every path of container_model.REQUIRED_PATHS has at least one case; the list of unreached paths holds nothing but
   what container_model.NOT_REACHED_ALLOWED names. The lengths found by search (container_model.FOUND) still hold. The
   tone clips (container_model.tone_case) count for no path here: their device files are not the oracle's byte for byte.
3. The constants the predicates restate equal the ones in crc_device.hpp, encode_plan.hpp, encode_plan.cpp and
   container_kernels.hip; finish_parts and plan_finish as restated agree with the rows pinned in
   tests/native/encode_plan_test.cpp.
4. The inputs of the older GPU tests that can be rebuilt here (tests/test_gpu_tail_crc.py, lossy_cases.pcm_cases as one
   clip each, ll_model.cases as one clip each) are run through the same predicates and the table "path, old inputs, new
   cases" is printed (pytest -s); DESIGN.md holds a copy. Of the 73 named paths the older inputs reach 36: the residues of
   a length modulo 64 and 4096 fall out of batches of a thousand clips by chance, and nothing else does - no slice-layout
   edge, no length of 4 MiB or more, no run longer than two frames, no second TOC chunk, no empty file.
"""
import os
import re
import zlib

import numpy as np
import pytest

import container_model as M
import flofile
from oracle import oracle as O

REQUIRED = [p for group in M.REQUIRED_PATHS.values() for p in group]


@pytest.fixture(scope="module")
def reach():
    """{path: [case names]} over the whole case list"""
    table = {}
    for c in M.cases():
        for p in M.case_paths(c["name"]):
            table.setdefault(p, []).append(c["name"])
    return table


def _flat(name):
    files = M.oracle_files(name)
    return [f for rung in files for f in rung] if M.case(name)["kind"] == "ladder" else files


@pytest.mark.parametrize("name", [c["name"] for c in M.cases()])
def test_writer_equals_the_oracle(name):
    c = M.case(name)
    for i, f in enumerate(_flat(name)):
        p = flofile.parse(f)
        assert (zlib.crc32(p.data) & 0xFFFFFFFF) == p.data_crc32, (name, i)
        head = M.model_head(f)
        assert len(head) == 74 + 20 * len(p.frames)
        assert M.head_difference(f[:len(head)], head) is None, (name, i, M.head_difference(f[:len(head)], head))
        # the same from the case's own parameters: nothing is taken out of the file's header but what the frames say
        mine = M.model_head(f, M.case_header(c, i))
        assert mine == f[:len(head)], (name, i, M.head_difference(f[:len(head)], mine))
        # the walk through DATA finds the frames the oracle's TOC names
        assert M.walk_frames(p.data, c["ch"]) == [(fr.size, fr.frame_samples) for fr in p.frames]
        assert p.total_samples == sum(fr.frame_samples for fr in p.frames)


def test_every_named_path_has_a_case(reach):
    for group, names in M.REQUIRED_PATHS.items():
        for p in names:
            print(f"{group:18s} {p:38s} {len(reach.get(p, [])):3d}  {', '.join(reach.get(p, [])[:3])}")
    assert len(set(REQUIRED)) == len(REQUIRED)
    not_reached = [p for p in REQUIRED if not reach.get(p)]
    assert set(not_reached) <= set(M.NOT_REACHED_ALLOWED), not_reached
    assert sorted(not_reached) == sorted(M.NOT_REACHED_ALLOWED), "a path listed as not reached is reached: update the list"


def test_lengths_found_by_search_still_hold():
    for key, spec in M.FOUND.items():
        if key.startswith("ll_"):
            f = O.encode_lossless(M.make_pcm(spec, 1), 48000, 1, 16, 2)
        else:
            f = O.encode_lossy(M.make_pcm(spec, 2), 44100, 2, 0.55)
        assert flofile.parse(f).data_size == M.FOUND_DATA[key], key


def test_cases_take_the_paths_they_are_named_for():
    P = M.case_clip_paths
    raw = P("ll_raw_4mib_edges")
    assert ["pow:n_4MiB-2" in raw[0], "pow:n_4MiB" in raw[1], "pow:n_4MiB+2" in raw[2]] == [True] * 3
    assert "pow:three_tables" in raw[0] and "pow:bit_by_bit" in raw[1] and "pow:slice_distance_ge_4MiB" in raw[3]
    assert all(fr.frame_type == 254 for f in M.oracle_files("ll_raw_4mib_edges") for fr in flofile.parse(f).frames)
    assert [flofile.parse(f).data_size - M.X8N_FAST_BOUND for f in M.oracle_files("ll_raw_4mib_edges")] == [-2, 0, 2, 40000]
    lay = P("ll_raw_64_layout")
    assert {"layout:exactly_parts_x_s", "layout:all_slices_non_empty", "parts:32"} <= lay[0]
    assert {"layout:empty_slice_behind_non_empty", "nt256:full2plus"} <= lay[1] and "nt256:nb255" in lay[2]
    assert "layout:data_0_bytes" in lay[9]
    odd = P("ll_rice_256_odd")
    assert {"nt256:one_byte", "layout:one_byte_over_a_boundary", "parts:8"} <= odd[0] and "nt256:last63" in odd[1]
    chain = P("chain_stereo_256")
    assert {"maker:tail", "maker:fallback_256", "maker:crc_slices_form1"} <= chain[0]
    assert {"nt64:nb63", "nt64:last0", "nt64:full0"} <= chain[0] and {"nt64:full1", "nt64:nb0"} <= chain[1]
    # the tone clips, by the oracle's lengths (the device's may differ: their GPU test takes the paths from its own files)
    tones = P("chain_stereo_256_tones")
    assert {"nt64:one_byte", "nt256:one_byte", "layout:one_byte_over_a_boundary"} <= tones[0] and "nt64:last63" in tones[1]
    assert "chain_stereo_256_tones" not in [c["name"] for c in M.cases()]
    fin = P("ll_fin256_frames")
    for i, nf in enumerate((0, 1, 255, 256, 257)):
        assert f"fin256:nf{nf}" in fin[i]
    assert {"fin256:per2", "fin256:empty_run"} <= fin[5] and "fin256:per8" in fin[6]
    assert {"fin256:per9", "fin256:partial_last_run", "fin256:loop_behind_the_registers", "fin256:nf2049"} <= fin[7]
    assert "fin256:per17plus" in fin[8]
    fused = P("ll_fused_chunks")
    assert "fused:nf0_beside_clips_with_frames" in fused[0] and "fused:nf256" in fused[3] and "fused:nf257" in fused[4]
    assert {"fused:front_sum_second_stride", "parts:128"} <= fused[5] and "fused:ends_a_chunk_before_the_longest" in fused[6]
    assert all("wide:few_clips_all_empty" in p for p in P("ll_few_all_empty"))
    for sr in (44100, 22050, 11025):
        assert f"ts:carry_at_{sr}" in P(f"lossy_mono_{sr}_64")[0]
    # 8000 divides 1,024,000: a lossy clip at 8 kHz never carries a remainder (its 2049 frames are there for per = 9)
    assert "ts:remainder_carry" not in P("lossy_mono_8000_64")[0] and "fin256:per9" in P("lossy_mono_8000_64")[0]
    assert "ts:first_division_over_32bit" in P("ll_5mhz_two_frames")[0]
    # rungs x clips is what the finish counts
    plans = {n: M.describe_plan(M.case_batches(n)[0][1]["plan"]) for n in ("ladder_16x3", "ladder_16x4", "ladder_256x3", "ladder_256x4")}
    assert plans == {"ladder_16x3": "fused 1024 43", "ladder_16x4": "slices 256 32", "ladder_256x3": "slices 256 3",
                     "ladder_256x4": "slices 256 1"}, plans


def test_constants_equal_the_sources():
    src = M.source_constants()
    mine = {k: getattr(M, k) for k in src}
    assert mine == src


def test_plan_equals_the_rows_of_the_native_test():
    with open(os.path.join(M.ROOT, "tests", "native", "encode_plan_test.cpp")) as f:
        text = f.read()
    block = re.search(r"kFinishRows\[\] = \{(.*?)\n\};", text, re.S).group(1)
    rows = re.findall(r'\{(\d+), (\d+), ([01]), "([^"]+)"\}', block)
    assert len(rows) >= 15
    for n, mf, ready, want in rows:
        assert M.describe_plan(M.plan_finish(int(n), int(mf), ready == "1")) == want, (n, mf, ready)
    auto = re.findall(r'\{0, 0, ([12]), (\d+), \d+, 0, 0, 0, D44, 1, "(\w+):', text)
    assert len(auto) >= 12
    for ch, n, form in auto:
        assert {"frames": 2, "chain": 1, "chain2q": 5}[form] == M.lossy_form(0, int(ch), int(n)), (ch, n, form)


# ---------------------------------------------------------------- what the older inputs reached
def old_batches():
    """-> [(name, batch)]. The batches of tests/test_gpu_tail_crc.py at the 256 compute units of an MI355X (6 pairs each):
    the first clips of each stand for the batch (the oracle's lengths stand in for the device's, which differ from them
    by a fraction of a percent); every clip of lossy_cases.pcm_cases and of ll_model.cases as a batch of one."""
    import lossy_cases
    import ll_model
    out = []
    pairs, sample = 6 * 256, 48
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 3 * 44100, 2 * pairs + 37)
    lens[::7], lens[3::11], lens[5::13], lens[9::17] = 0, 1, 1023, 6 * 44100
    for name, n_clips, nsf, seed in (("fewer_clips_than_pairs", 100, [2 * 44100] * sample, 0x7A11),
                                     ("exactly_one_round", pairs, [2 * 44100] * sample, 0x7A12),
                                     ("one_clip_more_than_a_round", pairs + 1, [2 * 44100] * sample, 0x7A13),
                                     ("ragged_lengths", 2 * pairs + 37, [int(x) for x in lens[:sample]], 0x7A14),
                                     ("many_short_clips", 5 * pairs + 11, [8820] * 4 * sample, 0x7A15)):
        files = [O.encode_lossy(O.synth_clip(n, 2, seed, 7 + i), 44100, 2, 0.55) for i, n in enumerate(nsf)]
        for v, which, tail in (("tail", 5, True), ("fallback", 5, False), ("form1", 1, True)):
            out.append((f"tail_crc_{name}_{v}", M.batch_of("lossy", 2, files, which=which, tail=tail, n_clips=n_clips)))
    for name, pcm, sr, ch, q in lossy_cases.pcm_cases():
        out.append((f"lossy_{name}", M.batch_of("lossy", ch, [O.encode_lossy(pcm, sr, ch, q)])))
    for c in ll_model.cases():
        out.append((f"ll_{c['name']}", M.batch_of("lossless", c["ch"], [O.encode_lossless(c["pcm"], c["sr"], c["ch"], 16, c["level"])])))
    return out


# what the older inputs DO reach (measured; the test fails if the list changes): everything else was reached by nothing
OLD_INPUTS_REACH = [
    "nt256:full0", "nt256:full1", "nt256:full2plus", "nt256:nb0", "nt256:last0", "nt256:last63", "nt256:ends_on_stripe",
    "nt256:stripes_then_blocks", "nt256:stripes_then_last_bytes",
    "nt64:full0", "nt64:full1", "nt64:full2plus", "nt64:nb0", "nt64:nb63", "nt64:last0", "nt64:last63", "nt64:ends_on_stripe",
    "nt64:stripes_then_blocks", "nt64:stripes_then_last_bytes",
    "layout:empty_slice_behind_non_empty", "parts:1", "parts:512", "pow:three_tables", "fin256:per1", "fin256:per2",
    "fin256:empty_run", "fin256:nf1", "fused:one_chunk", "ts:remainder_carry", "ts:carry_at_44100", "ts:div32_in_run",
    "ts:varying_frame_samples", "maker:tail", "maker:fallback_256", "maker:crc_slices_form1", "maker:fused",
]


def test_what_the_older_inputs_reached(reach):
    old = {}
    for name, b in old_batches():
        for p in set().union(*M.batch_paths(b)):
            old.setdefault(p, []).append(name)
    for p in REQUIRED:
        print(f"{p:38s} old {len(old.get(p, [])):3d}  new {len(reach.get(p, [])):3d}   {', '.join(old.get(p, [])[:2])}")
    print("old inputs reach:", [p for p in REQUIRED if p in old])
    assert [p for p in REQUIRED if p in old] == OLD_INPUTS_REACH
