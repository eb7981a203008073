"""ll_model pinned to the oracle, and the reach table of the lossless encode path cases (no GPU needed).

1. For every case the model's decisions equal what the oracle's file shows: frame type, flags, sizes, and per channel the
   kind, coefficients, shift, Rice parameter and payload length; the payload rebuilt from the model's residuals with the
   oracle's Rice coder equals the payload bytes. res_pos comes out of the parsed file and must equal the model's layout.
2. Every path of ll_model.REQUIRED_PATHS has at least one case; the list of unreached paths holds nothing but what
   ll_model.NOT_REACHED_ALLOWED names.
3. The inputs of the older tests/test_gpu_lossless.py (one clip of each test, full-size batches left out) are run through
   the same model and the table "path, old inputs, new cases" is printed (pytest -s); DESIGN.md holds a copy. The older
   inputs reach neither bit writer's fallback (no unstaged tile at all), no tile near the staging limit, no q = 254 or 255,
   no long code at a tile's last sample, no raw winner at alignment 3, no LPC winner that needs the third sweep, neither
   the max_coeff nor the max_res discard, no plane with exactly one FULL run, no odd stereo slice under mid/side and no
   ragged multi-channel slice. They do reach the third sweep itself from both sides (the sweep and sine fixtures).
"""
import numpy as np
import pytest

import flofile
import ll_model as M
import signals
from fixtures_util import LOSSLESS_EXAMPLES, lossless_input_for
from oracle import oracle as O


def res_positions(f):
    """byte offset inside the DATA chunk of every channel's residual bytes, from the parsed file"""
    out = []
    for (_, off, _, _), fr in zip(f.toc, f.frames):
        pos, row = off + 6, []
        for c in fr.channels:
            row.append(pos + 4 + len(c.raw) - len(c.residuals))
            pos += 4 + len(c.raw)
        out.append(row)
    return out


def pin(pcm, sr, ch, level, tag):
    """Assert that the model's decisions are the oracle's for this clip -> (frames of the model, oracle bytes)."""
    o = O.encode_lossless(pcm, sr, ch, 16, level)
    f = flofile.parse(o)
    fr = M.file_model(pcm, sr, ch, level)
    assert len(fr) == len(f.frames), tag
    rp = res_positions(f)
    for i, (m, p) in enumerate(zip(fr, f.frames)):
        assert (m.frame_type, m.frame_samples, m.flags, m.size) == (p.frame_type, p.frame_samples, p.flags, p.size), (tag, i)
        if m.silent:
            assert all(len(c.raw) == 0 for c in p.channels), (tag, i)
            continue
        for c, (cm, pc) in enumerate(zip(m.channels, p.channels)):
            w = cm.winner
            if m.frame_type != 254:     # a Raw-typed frame stores the bare bytes: nothing but the length to compare
                want = (w.coeffs if w.kind == 2 else [], 128 + w.order if w.kind == 1 else (w.shift if w.kind == 2 else 0),
                        2 if w.kind == 0 else 0, w.k if w.kind else 0)
                assert (pc.coeffs, pc.shift_bits, pc.encoding, pc.rice_k) == want, (tag, i, c, w.name)
            assert len(pc.residuals) == w.size, (tag, i, c, w.name, len(pc.residuals), w.size)
            assert rp[i][c] == cm.res_pos, (tag, i, c)
            if w.kind:
                assert O.rice_encode_i32(w.residuals.astype(np.int32), w.k) == pc.residuals, (tag, i, c, w.name)
            else:
                assert (cm.ints & 0xFFFF).astype("<u2").tobytes() == pc.residuals, (tag, i, c)
    return fr, o


@pytest.fixture(scope="module")
def reach():
    """{path: [case names]} over the whole case list, each case pinned to the oracle on the way"""
    table, models = {}, {}
    for c in M.cases():
        fr, _ = pin(c["pcm"], c["sr"], c["ch"], c["level"], c["name"])
        models[c["name"]] = fr
        for p in M.paths(fr, c["level"]):
            table.setdefault(p, []).append(c["name"])
    return table, models


def test_model_equals_the_oracle_on_every_case(reach):
    table, models = reach
    assert len(models) == len(M.cases()) and len({c["name"] for c in M.cases()}) == len(M.cases())


def test_every_named_path_has_a_case(reach):
    table, _ = reach
    required = [p for group in M.REQUIRED_PATHS.values() for p in group]
    missing = [p for p in required if not table.get(p)]
    for kernel, group in M.REQUIRED_PATHS.items():
        for p in group:
            print(f"{kernel:11s} {p:28s} {len(table.get(p, [])):3d}  {', '.join(table.get(p, [])[:3])}")
    assert not missing, missing
    not_reached = [r for r in ("ac0", "err", "gamma", "max_coeff", "n<=order", "max_res") if not table.get("invalid_" + r)]
    assert set(not_reached) <= set(M.NOT_REACHED_ALLOWED), not_reached
    assert sorted(not_reached) == sorted(M.NOT_REACHED_ALLOWED), "a path listed as not reached is reached: update the list"


def test_cases_take_the_paths_they_are_named_for(reach):
    _, mo = reach

    def P(name):
        c = next(c for c in M.cases() if c["name"] == name)
        return M.paths(mo[name], c["level"])
    # the packer's two writers
    for name in ("dense96_tile0_l5", "dense96_middle_l5", "dense192_middle_l5", "dense192_last_tile_l5", "dense96_ms_l5", "dense96_3ch_l5"):
        assert {"unstaged_lpc", "unstaged_long_code"} <= P(name), name
    for name in ("dense96_middle_l2", "dense192_middle_l2", "dense96_middle_l0", "dense192_middle_l0"):
        assert "unstaged_fixed" in P(name), name
    assert [t["staged"] for t in mo["dense96_tile0_l5"][0].channels[0].tiles][:2] == [False, True]
    assert [t["staged"] for t in mo["dense192_last_tile_l5"][0].channels[0].tiles][-2:] == [True, False]
    assert [t["staged"] for t in mo["dense96_straddle_l5"][0].channels[0].tiles][:3] == [True, False, True]
    for name in ("dense192_straddle_l5", "dense192_two_tiles_l5"):
        assert "two_unstaged_in_a_row" in P(name), name
    assert mo["dense96_ms_l5"][0].use_ms and "ms" in P("dense96_ms_l5")
    assert len({cm.res_pos & 3 for cm in mo["dense96_3ch_l5"][0].channels}) == 3
    under, over = (mo[n][0].channels[0].tiles[1] for n in ("limit_under", "limit_over"))
    assert under["staged"] and not over["staged"]
    assert (under["lead"] + under["bits"], over["lead"] + over["bits"]) == (131054, 131094)
    # long codes: fixed order 0 wins the spike plane, so the residuals are the samples
    for name in [c["name"] for c in M.cases() if c["name"].startswith("long_codes") and c["group"] == "packer"]:
        cm = mo[name][0].channels[0]
        assert cm.winner.name == "fixed0" and np.array_equal(cm.winner.residuals, cm.ints), name
        assert mo[name][0].frame_type != 254, name
    assert mo["long_codes_k8_rot0"][0].channels[0].winner.k == 8 and mo["long_codes_k0_rot0"][0].channels[0].winner.k == 0
    assert mo["long_codes_neg32768"][0].channels[0].ints.min() == -32768
    # the search
    for name in ("sweep3_below_l5", "sweep3_below_l9"):
        lp = [c for c in mo[name][0].channels[0].cands if c.kind == 2]
        assert lp and all(c.valid and c.d_robust and c.d == -2 for c in lp), name
    lp = {c.order: c for c in mo["sweep3_above_some_l9"][0].channels[0].cands if c.kind == 2}
    assert lp[11].d == lp[12].d == 3 and lp[11].d_robust and lp[12].d_robust and all(0 <= lp[o].d <= 2 for o in range(5, 10))
    for name in ("sweep3_winner_l5", "sweep3_winner_l9"):
        w = mo[name][0].channels[0].winner
        assert w.kind == 2 and w.d_robust and w.d < 0, name
    assert mo["tie_first_wins"][0].channels[0].winner.name == "lpc5"
    assert mo["tie_later_has_fewer_bits"][0].channels[0].winner.name == "fixed0"
    assert mo["tie_rice_equals_raw"][0].channels[0].winner.name == "raw"
    assert mo["max_res_discard_l5"][0].channels[0].cand("lpc8").reason == "max_res"
    assert int(np.abs(mo["max_res_discard_l5"][0].channels[0].cand("lpc8").residuals).max()) > 1000000
    assert mo["max_coeff_single_impulse_l5"][0].channels[0].cand("lpc5").reason == "max_coeff"
    assert mo["ac0_zero_channel_of_three_l9"][0].channels[1].cand("lpc12").reason == "ac0"
    winners = {lv: tuple(cm.winner.name for cm in mo[f"levels_l{lv}"][0].channels) for lv in range(10)}
    assert len(set(winners.values())) >= 5, winners
    # prepare
    assert [mo[n][0].use_ms for n in ("ms_tie_stays_lr", "ms_floor_stays_lr", "ms_takes_ms")] == [False, False, True]
    for n, x in (("ms_tie_stays_lr", 20), ("ms_floor_stays_lr", 19), ("ms_takes_ms", 18)):
        l, r = mo[n][0].planes
        assert (int(l.sum()), int(r.sum()), int(((l - r) ** 2).sum())) == (x + 10, 10, x), n
    assert mo["odd_stereo_ms"][0].use_ms and not mo["odd_stereo_lr"][0].use_ms
    assert mo["silence_all_just_below"][0].silent and mo["silence_negzero_subnormal"][0].silent
    one = mo["silence_one_at_threshold"][0]
    assert not one.silent and all(not p.any() for p in one.planes)
    conv = mo["conversion_edges_mono"][0].planes[0][:23].tolist()
    assert conv == [32767, -32767, 32767, 32766, -32767, -32766, -32768, 32767, 32767, -32768, 32767, -32768, 32767, -32768,
                    0, 0, 1, -1, 0, 16383, -16383, 32767, -32768], conv


def test_undecodable_cases_are_few_and_none_is_a_packer_case(reach):
    _, mo = reach
    ex = [c["name"] for c in M.cases() if M.undecodable(mo[c["name"]])]
    print("undecodable:", ex)
    assert len(ex) == M.EXPECTED_UNDECODABLE, ex
    assert 10 * len(ex) < len(M.cases())
    assert not [n for n in ex if next(c for c in M.cases() if c["name"] == n)["group"] == "packer"]
    # level 0 can only emit Raw-typed frames: every level-0 case with a Rice winner is exempt, and is kept out of "packer"
    assert all(c["group"] == "level0" for c in M.cases() if c["level"] == 0)


def test_oracle_decodes_every_other_case_to_the_models_integers(reach):
    _, mo = reach
    for c in M.cases():
        if M.undecodable(mo[c["name"]]):
            continue
        back, sr, ch = O.decode_lossless_i32(O.encode_lossless(c["pcm"], c["sr"], c["ch"], 16, c["level"]))
        want = M.expected_ints(mo[c["name"]], c["ch"])
        assert back.size == want.size and np.array_equal(back, want), c["name"]


# ---------------------------------------------------------------- what the older inputs reached
def old_inputs():
    """One clip of every test of tests/test_gpu_lossless.py (the full-size batches are left out)."""
    out = []
    for name in LOSSLESS_EXAMPLES:
        ref, f32, ints, sr, ch = lossless_input_for(name)
        out.append((f"fixture_{name}", f32, sr, ch, O.info(ref).compression_level))
    for ch, n in [(1, 44100), (2, 44100), (2, 100000), (6, 9000), (1, 1), (2, 3), (1, 44099), (1, 44101), (2, 88201), (3, 50001)]:
        if ch <= 2:
            pcm = signals.music_like(44100, n, ch, seed=n)[: n * ch]
        else:
            pcm = np.stack([signals.sine(150.0 * (c + 1), 44100, n, 0.25) + signals.fast_noise(n, c, 0.01) for c in range(ch)], axis=1).reshape(-1)
        out.append((f"byte_identical_{ch}_{n}", pcm, 44100, ch, 5))
    for level in range(10):
        out.append((f"levels_{level}", signals.music_like(44100, 30000, 2, seed=100 + level), 44100, 2, level))
    for sr in (8000, 22050, 48000, 96000, 192000):
        out.append((f"rate_{sr}", (signals.sine(440.0, sr, sr + sr // 3, 0.6) + signals.fast_noise(sr + sr // 3, 1, 0.003)).astype(np.float32), sr, 1, 5))
    out.append(("hires", O.synth_clip(96000 * 3 + 777, 2, clip_id=5), 96000, 2, 5))
    base = signals.music_like(44100, 50000, 1, seed=4)
    out.append(("mid_side", np.stack([base, base * np.float32(0.97)], axis=1).reshape(-1), 44100, 2, 5))
    out.append(("quirk_silence", np.zeros(5000, np.float32), 44100, 2, 5))
    out.append(("quirk_tiny", np.full(44100, 3e-5, np.float32), 44100, 1, 5))
    out.append(("quirk_noise_half", signals.fast_noise(8000, 9, 0.5), 44100, 1, 5))
    out.append(("quirk_noise_full", signals.fast_noise(44100, 3, 1.0), 44100, 1, 5))
    x = signals.fast_noise(5000, 2)
    x[10], x[20], x[30] = np.nan, np.inf, -np.inf
    out.append(("quirk_nonfinite", x, 44100, 1, 5))
    out.append(("quirk_mixed", np.stack([signals.fast_noise(30000, 1, 1.0), signals.sine(300.0, 44100, 30000, 0.4)], axis=1).reshape(-1), 44100, 2, 5))
    noise = signals.fast_noise(20000, 5, 1.0)
    out.append(("mid_wraps", np.stack([noise, noise], axis=1).reshape(-1), 44100, 2, 5))
    out.append(("metadata", signals.music_like(44100, 3000, 1, seed=1), 44100, 1, 7))
    for n in (1, 44100 * 2, 12345 * 2, 100001, 88200 * 2 + 2):
        out.append((f"ragged_{n}", signals.music_like(44100, (n + 1) // 2, 2, seed=n)[:n], 44100, 2, 5))
    out.append(("synthetic_batch_clip", O.synth_clip(5 * 44100 + 123, 2, 0xF10A0D10, 7), 44100, 2, 5))
    return out


# what the older inputs must NOT reach for the gap to have been real (measured; the test fails if one of them does)
OLD_INPUTS_MUST_MISS = [
    "unstaged", "unstaged_fixed", "unstaged_lpc", "unstaged_long_code", "two_unstaged_in_a_row", "staged_next_to_unstaged",
    "tile_just_under_limit", "tile_just_over_limit", "staged_q254", "staged_q255", "long_code_last_of_tile", "res_pos3_raw",
    "sweep3_winner", "invalid_max_coeff", "invalid_max_res", "one_full_run", "odd_stereo_slice_ms", "ragged_channels",
]


def test_what_the_older_inputs_reached(reach):
    table, _ = reach
    old = {}
    for name, pcm, sr, ch, level in old_inputs():
        fr, _ = pin(pcm, sr, ch, level, name)
        for p in M.paths(fr, level):
            old.setdefault(p, []).append(name)
    required = [p for group in M.REQUIRED_PATHS.values() for p in group]
    for p in required:
        print(f"{p:28s} old {len(old.get(p, [])):3d}  new {len(table.get(p, [])):3d}   {', '.join(old.get(p, [])[:2])}")
    print("old inputs miss:", [p for p in required if p not in old])
    assert [p for p in required if p not in old] == OLD_INPUTS_MUST_MISS
