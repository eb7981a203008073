"""The f64 reference of the forward transform (fwd_ref) against the oracle, on the CPU: before test_gpu_fwd_transform.py
counts the device's error in units of the oracle's, the reference has to be the operation (it agrees with the oracle's two
f64 evaluations to their rounding, framing included), every tight case has to be finite and silent where it should be on
both sides, and the unit has to be what it is believed to be. Prints, per case, the oracle's worst max|err| / frame maximum
and its relative RMS error, and the floors of the class (measured: worst 0.5e-7 ... 4.2e-7, RMS 0.5e-7 ... 1.5e-7; the floors
are the impulse windows' worst, 4.18e-7, and tone_1022_2ch's RMS, 1.50e-7; the clips alone stay within 3.1e-7).
Full-scale noise 1.9e-7 ... 2.4e-7, music and its levels 1.3e-7 ... 1.8e-7, impulse clips 1.3e-7 ... 3.1e-7, tones, DC and Nyquist
0.5e-7 ... 2.0e-7."""
import numpy as np
import pytest

import fwd_ref as F
from oracle import oracle as O

F64_AGREE = 1e-7      # of the frame maximum: this reference's own rounding plus that of the oracle's f64 evaluations (measured: 3e-8, 6e-8)
CEILING = 1e-6        # a sanity ceiling on the yardstick, not the device's bound: beyond it the case or the reference is wrong


def test_the_reference_is_the_oracles_f64_definition():
    rng = np.random.default_rng(5)
    win = np.concatenate([rng.uniform(-1, 1, (6, 2048)).astype(np.float32), F.impulse_windows()[[0, 1, 700, 1023, 1024, 2047]],
                          F.windows(*F.case("tone_511_1ch"))[:, 0], F.windows(*F.case("music_2ch"))[:, 1]])
    mine, same = F.transform(win), F.transform_f32_products(win)
    worst = worst_same = 0.0
    for i, w in enumerate(win):
        ref = O.mdct_forward_direct_f64(w)
        if not ref.any():
            assert not mine[i].any()
            continue
        d = float(np.abs(mine[i] - ref).max() / np.abs(ref).max())
        s = float(np.abs(same[i] - ref).max() / np.abs(ref).max())
        worst, worst_same = max(worst, d), max(worst_same, s)
        assert d <= F64_AGREE, (i, d)
        assert s <= 1e-9, (i, s)      # nothing left but two float64 summations and its unreduced cosine argument (8000 rad x 1.1e-16)
    print(f"fwd_ref.transform against O.mdct_forward_direct_f64 on {len(win)} windows: at most {worst:.2e} of the frame maximum; "
          f"with its f32 windowing products {worst_same:.2e}")


@pytest.mark.parametrize("name", F.CLIPS)
def test_framing_and_values_against_the_oracles_f64_transform(name):
    """hop count, pre-roll, the dropped partial sample-frame and the channel order of every case, against O.lossy_analyze
    with the transform evaluated in double precision. That evaluation rounds twice to f32: every windowing product, and the
    coefficient. Each rounding is at most 2^-24 = 6.0e-8 of the frame maximum and each is held to 1e-7 on its own: the
    oracle against this reference with the same f32 products (the coefficient's rounding), and this reference with and
    without them (the products' rounding). Together they are printed: at most 1.0e-7, reached where a frame holds a
    single sample (frame 3 of len_2049_2ch: 1.002e-7) and both roundings fall on the frame's largest coefficient."""
    pcm, ch = F.case(name)
    truth, skip, _ = F.yardstick(name)
    o = O.lossy_analyze(pcm, F.SR, ch, 0.55, f64_mdct=True)["coeffs"]
    assert o.shape == truth.shape == (F.hops_of(pcm.size // ch), ch, 1024), (name, o.shape, truth.shape)
    assert 1 <= truth.shape[0] <= 6 and ch <= 8 and not skip.any()
    same = F.transform_f32_products(F.windows(pcm, ch))
    ms, mp, m = F.measure(o, same), F.measure(same, truth), F.measure(o, truth)
    print(f"{name:26s} oracle's f64 transform against the reference with f32 products {ms['worst']:.2e}; the products' rounding {mp['worst']:.2e}; "
          f"both {m['worst']:.2e}")
    for x in (ms, mp, m):
        assert x["finite"] and x["zero_ok"], (name, x)
    assert ms["worst"] <= F64_AGREE, (name, ms)
    assert mp["worst"] <= F64_AGREE, (name, mp)
    assert m["worst"] <= 2.0 ** -23, (name, m)       # (the two roundings' sum, by the triangle inequality)


def test_partial_sample_frame_and_lengths():
    pcm, ch = F.case("len_1025_2ch")
    assert ch == 2 and pcm.size == 2 * 1025 + 1
    assert [F.hops_of(n) for n in F.LENGTHS] == [1, 2, 2, 2, 2, 3, 3, 3, 4]
    assert F.case("len_0_1ch")[0].size == 0 and not F.yardstick("len_0_2ch")[0].any()


@pytest.mark.parametrize("name", F.TIGHT)
def test_tight_case_is_finite_and_silent_where_it_should_be_in_the_oracle(name):
    truth, skip, m = F.yardstick(name)
    assert np.isfinite(truth).all() and not skip.any(), name
    assert m["finite"], (name, "the oracle's coefficients are not finite")
    assert m["zero_ok"], (name, "a (frame, channel) that is silent in the reference is not exactly zero in the oracle", m["zero_at"])
    f, c, k = m["at"]
    print(f"{name:26s} oracle worst max|err|/frame maximum {m['worst']:.2e} at frame {f} channel {c} bin {k}, relative RMS {m['rms']:.2e}, "
          f"{m['frames']} (frame, channel) pairs compared")
    assert m["worst"] < CEILING and m["rms"] < CEILING, (name, m)


def test_floors_of_the_tight_class():
    fw, fr = F.floors()
    ws = [F.yardstick(n)[2]["worst"] for n in F.TIGHT if F.yardstick(n)[2]["frames"]]
    rs = [F.yardstick(n)[2]["rms"] for n in F.TIGHT if F.yardstick(n)[2]["frames"]]
    print(f"tight class, {len(F.TIGHT)} cases: oracle worst {min(ws):.2e} ... {max(ws):.2e}, relative RMS {min(rs):.2e} ... {max(rs):.2e}; "
          f"floors: worst {fw:.3e}, rms {fr:.3e}")
    assert fw == max(ws) and fr == max(rs)
    assert 5e-8 < fw < CEILING and 5e-8 < fr < CEILING
    for n in F.TIGHT:       # a bound is never below the floor nor below the case's own margin
        bw, br = F.bounds(n)
        m = F.yardstick(n)[2]
        assert bw == max(2.0 * m["worst"], fw) and br == max(1.5 * m["rms"], fr)


@pytest.mark.parametrize("name", F.EDGE)
def test_edge_case_is_non_finite_in_the_oracle_only_where_the_sample_lies(name):
    pcm, ch = F.case(name)
    truth, skip, m = F.yardstick(name)
    o = O.lossy_analyze(pcm, F.SR, ch, 0.55)["coeffs"]
    bad = ~np.isfinite(o).all(axis=2)
    assert skip.sum() == 2 and skip[1:3, ch - 1].all(), (name, np.argwhere(skip).tolist())
    assert np.array_equal(bad, skip), (name, "the oracle is non-finite in other (frame, channel) pairs than the sample's", np.argwhere(bad != skip).tolist())
    assert not np.isfinite(o[skip]).any(), (name, "a pair that holds the sample keeps finite coefficients in the oracle")
    assert m["finite"] and m["zero_ok"] and m["worst"] < CEILING, (name, m)
    print(f"{name:26s} oracle: (frame, channel) {np.argwhere(skip).tolist()} hold no finite value; elsewhere worst {m['worst']:.2e} rms {m['rms']:.2e}")


def test_every_transform_bearing_kernel_is_reached_by_a_case():
    table = F.reach(F.CLIPS)
    for plan, kernel in F.KERNELS.items():
        assert table.get(plan), (plan, kernel, "no tight case reaches it")
        print(f"{plan:30s} {kernel:58s} {len(table[plan])} (case, form, quality) runs, e.g. {table[plan][0]}")
    assert set(table) == set(F.KERNELS), set(table) ^ set(F.KERNELS)
