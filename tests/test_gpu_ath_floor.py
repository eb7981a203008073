"""The band-alive ballot of the lock-step stereo chain kernel against the bands' hearing floors, on the device.

A band is alive when its maximum is above its masking amplitude AND above the smallest ATH amplitude of its bins
(StatMasks::band_ath_floor); the packer wave neither quantises nor packs a block of 128 positions none of whose bands is
alive. That must change nothing: hand-made spectra go through ctx.lossy_pack_frames under forms 5, 1 and 2 (the route of
tests/test_gpu_lossy_paths.py), and form 5 must give the integers, scale words, frame sizes and DATA bytes of forms 1 and 2,
which know no ballot. Form 5's integers must also be the oracle's wherever tests/test_gpu_lossy_explained.py does not
already admit a disagreement: outside the window of 4 x the oracle's own deviation from the f64 model around a zero margin
(gpu_util.explain_lossy_stage), and, where the margin is NaN (non-finite input), everywhere.

Every case is first checked on the CPU to be what its name says: tests/psy_ref.py gives the band maxima and masking
levels, tests/ath_floor_tables.py the ATH amplitudes and floors the device is handed, and `situation` restates the
ballot and the blocks it leaves to visit. A band whose maximum lies within 0.1 % of its masking amplitude fails the case:
the restatement is f64, the device's is f32.

    floor_b{22,23,24,0}   a band that is masking-alive around its floor: maximum one ulp under it, on it (the compare is
                          strict), one ulp above it at the bin that holds the floor (kept: the device's keep test is the
                          amplitude compare against the same table), one ulp above it at a bin whose own ATH is higher (alive,
                          keeps nothing); then the same split over the two channels
    blocks                one band alive per frame: band 23 through bins of block 4 only and of block 5 only, and bands that
                          make one block of a pair alive and the other dead (the quantiser gathers a block's rows only when it
                          visits the block). At 48 kHz block 4 holds bins of band 23 only, which block 5 holds too: "block 4
                          alive, block 5 dead" does not exist there and the case says so
    channels              one channel's band 24 above its floor and the other's under it, both ways; both under it; every
                          band of both channels one ulp under its floor: all-zero frames
    alternate             blocks 5-7 alive and dead in turn, each on both frame parities, amplitudes changing frame by frame
    nonfinite             band 24 of a quiet frame: NaN next to a finite coefficient far above the floor (the reference takes a NaN
                          band energy for -100 dB and its maxima skip NaN, so the masking amplitude is finite, the band alive
                          and the finite coefficient kept: no input gives the oracle a NaN masking amplitude), and +-inf (the
                          oracle drops it - infinite band energy, masking amplitude +inf, scale factor 0 - and the channel's
                          level stays infinite: a band above its floor that no masking amplitude lets live). Every form
                          must do as the oracle does
    dense                 more than 128 non-zeros in a channel (block form) and, at q = 0.99, a frame of many runs (general form),
                          each with dead blocks behind the non-zeros
Needs an MI355X."""
import numpy as np
import pytest

import ath_floor_tables
import lossy_model as M
import psy_ref
from gpu_util import ctx  # noqa: F401
from oracle import oracle as O
from test_gpu_lossy_paths import describe_data_difference, forced

pytestmark = pytest.mark.gpu
Q = 0.55
UP, DOWN = np.float32(np.inf), np.float32(0.0)


def situation(c, sr, q):
    """CPU restatement of the ballot: dict of masking [h][ch][25] (maximum above the masking amplitude), above [h][ch][25]
    (maximum above the floor), alive [h][25] (both, in either channel), visit [h][8] (block holds bins of an alive band)"""
    t = ath_floor_tables.load(sr, q)
    m = psy_ref.model(c, sr, q)
    assert np.array_equal(m["band"], t["band"])
    smr_thr = np.float64(np.float32(O.lib().flo_o_smr_threshold(float(q))))
    with np.errstate(all="ignore"):
        tl1 = 10.0 ** ((smr_thr + m["level"] - 10.0) / 20.0)
        bmax = m["band_max"].astype(np.float64)
        near = (bmax > 0) & np.isfinite(tl1) & np.isfinite(bmax) & (np.abs(bmax / tl1 - 1.0) < 1e-3)
        assert not near.any(), ("a band maximum within 0.1 % of its masking amplitude", np.argwhere(near)[0].tolist())
        masking = bmax > tl1                                             # NaN compares false
        above = m["band_max"] > t["floor"][:25]                          # exact: both are f32
    alive = (masking & above).any(axis=1)
    blocks = np.array([[((t["band"][128 * k:128 * k + 128]) == b).any() for k in range(8)] for b in range(25)])   # [25][8]
    visit = (alive[:, :, None] & blocks[None]).any(axis=1)
    return dict(masking=masking, above=above, alive=alive, visit=visit, tables=t, model=m)


def band_bins(t, b):
    return np.flatnonzero(t["band"] == b)


def floor_bin(t, b):
    k = band_bins(t, b)
    return int(k[np.argmin(t["ath_lin"][k])])


def run_forms(ctx, name, c, sr, q):
    """forms 5, 1, 2 on the device; form 5 against forms 1 and 2 and against the oracle; returns form 5's result"""
    got = {}
    for form in (5, 1, 2):
        with forced(ctx, form):
            got[form] = ctx.lossy_pack_frames(c, sr, q)
    g = got[5]
    for form in (1, 2):
        r = got[form]
        bad = np.argwhere(g["q"] != r["q"])
        assert bad.size == 0, (name, "integers of form 5 and form", form, "first (frame, channel, position)", bad[0].tolist(),
                               int(g["q"][tuple(bad[0])]), int(r["q"][tuple(bad[0])]))
        assert np.array_equal(g["sf_words"], r["sf_words"]), (name, form, "scale words", np.argwhere(g["sf_words"] != r["sf_words"])[0].tolist())
        assert g["frame_sizes"].tolist() == r["frame_sizes"].tolist(), (name, form, "frame sizes")
        msg = describe_data_difference(f"{name} form 5 against form {form}", g["data"], r["data"], c.shape[1])
        assert msg is None, msg
    want, sizes = M.write_frames(g["q"], g["sf_words"])
    assert g["frame_sizes"].tolist() == sizes, (name, "frame sizes against the model's")
    msg = describe_data_difference(f"{name} form 5 against the frame writer", g["data"], want, c.shape[1])
    assert msg is None, msg
    # the oracle, wherever test_gpu_lossy_explained.py admits no disagreement
    o = O.lossy_quantize(c, sr, q)
    m = psy_ref.model(c, sr, q)
    eps = 4.0 * psy_ref.oracle_deviation(m, o)
    with np.errstate(invalid="ignore"):
        decided = np.isnan(m["margin"]) | (np.abs(m["margin"]) > eps)
    bad = np.argwhere(decided & (g["q"] != o["q"]))
    print(f"{name}: window {eps:.2e} dB holds {int((~decided).sum())} of {decided.size} coefficients")
    assert bad.size == 0, (name, "integers of form 5 and the oracle outside the window", eps, "first (frame, channel, position)",
                           bad[0].tolist(), int(g["q"][tuple(bad[0])]), int(o["q"][tuple(bad[0])]))
    assert np.array_equal(g["sf_words"], o["sf_words"]), (name, "scale words against the oracle")
    return g


# ------------------------------------------------------------------------------------------------ around the floor
@pytest.mark.parametrize("b", [22, 23, 24, 0])
@pytest.mark.parametrize("sr", [44100, 48000])
def test_band_around_its_floor(ctx, sr, b):
    t = ath_floor_tables.load(sr, Q)
    fl = t["floor"][b]
    kf = floor_bin(t, b)
    under, over = np.nextafter(fl, DOWN), np.nextafter(fl, UP)
    kb = band_bins(t, b)
    kh = int(kb[np.argmax(t["ath_lin"][kb])])
    assert t["ath_lin"][kf] == fl and t["ath_lin"][kh] > over and kh != kf
    # (frame, channel) -> (bin, value); everything else zero
    plan = [{0: (kf, under)}, {0: (kf, fl)}, {0: (kf, -over)}, {0: (kh, over)}, {},
            {0: (kf, under), 1: (kf, over)}, {0: (kf, -over), 1: (kf, fl)}, {0: (kf, under), 1: (kh, -over)}, {0: (kf, over), 1: (kf, over)}]
    c = np.zeros((len(plan), 2, 1024), np.float32)
    for h, chans in enumerate(plan):
        for ch, (k, v) in chans.items():
            c[h, ch, k] = v
    s = situation(c, sr, Q)
    # what the case is: every band with a coefficient is masking-alive, and alive exactly where a maximum is above the floor
    for h, chans in enumerate(plan):
        for ch in chans:
            assert s["masking"][h, ch, b], (sr, b, h, ch, "not masking-alive")
    want_alive = [False, False, True, True, False, True, True, True, True]
    assert s["alive"][:, b].tolist() == want_alive and not np.delete(s["alive"], b, axis=1).any()
    g = run_forms(ctx, f"floor_b{b}_{sr}", c, sr, Q)
    kept = {(h, ch, k) for h, ch, k in np.argwhere(g["q"] != 0).tolist()}
    want_kept = {(h, ch, k) for h, chans in enumerate(plan) for ch, (k, v) in chans.items() if k == kf and abs(v) == over}
    assert kept == want_kept, (sr, b, sorted(kept ^ want_kept))
    assert all(abs(int(g["q"][p])) == 30000 for p in kept)


# ------------------------------------------------------------------------------------------------ blocks of a pair
@pytest.mark.parametrize("sr", [44100, 48000])
def test_one_block_of_a_pair_alive(ctx, sr):
    t = ath_floor_tables.load(sr, Q)
    k23 = band_bins(t, 23)
    in4, in5 = k23[(k23 // 128) == 4], k23[(k23 // 128) == 5]
    assert in4.size and in5.size                                        # band 23 lies on both sides of the edge at both rates
    # one strong coefficient per frame, four times the bin's own ATH amplitude and far above the masking amplitude of a lone
    # coefficient: (bin, channel)
    picks = [(int(in4[-1]), 0), (int(in5[0]), 1), (int(band_bins(t, 24)[0]), 0), (int(band_bins(t, 22)[-1]), 1),
             (int(band_bins(t, 18)[0]), 0), (floor_bin(t, 0), 1), (int(band_bins(t, 21)[0]), 0), (int(band_bins(t, 24)[-1]), 1),
             (int(band_bins(t, 20)[0]), 0), (int(band_bins(t, 16)[0]), 1)]
    c = np.zeros((len(picks), 2, 1024), np.float32)
    for h, (k, ch) in enumerate(picks):
        c[h, ch, k] = np.float32(4.0) * max(t["ath_lin"][k], np.float32(1.0)) * (-1 if h % 3 == 0 else 1)
    s = situation(c, sr, Q)
    for h, (k, ch) in enumerate(picks):
        assert s["alive"][h].sum() == 1 and s["alive"][h, t["band"][k]], (sr, h, "one band alive")
    pairs = {g: {(bool(v[2 * g]), bool(v[2 * g + 1])) for v in s["visit"]} for g in range(4)}
    assert s["visit"][0, 4] and s["visit"][0, 5] and s["visit"][1, 4] and s["visit"][1, 5]      # band 23 alive: both of its blocks
    assert (False, True) in pairs[2] and (True, True) in pairs[2] and (True, False) in pairs[0] and (False, True) in pairs[0]
    if sr == 44100:
        assert (True, False) in pairs[2]                                 # band 22 alone: block 4 without block 5
    else:
        blocks4 = set(t["band"][512:640].tolist())
        assert blocks4 == {23}                                           # no band makes block 4 alive and leaves block 5 dead here
    g = run_forms(ctx, f"blocks_{sr}", c, sr, Q)
    assert {(h, ch, k) for h, ch, k in np.argwhere(g["q"] != 0).tolist()} == {(h, ch, k) for h, (k, ch) in enumerate(picks)}


# ------------------------------------------------------------------------------------------------ channels
def test_channels_apart_and_every_band_dead(ctx):
    sr = 44100
    t = ath_floor_tables.load(sr, Q)
    fl, kf = t["floor"][24], floor_bin(t, 24)
    under, over = np.nextafter(fl, DOWN), np.nextafter(fl, UP)
    c = np.zeros((8, 2, 1024), np.float32)
    c[0, 0, kf], c[0, 1, kf] = over, under
    c[1, 0, kf], c[1, 1, kf] = under, -over
    c[2, 0, kf], c[2, 1, kf] = under, fl
    present = [b for b in range(25) if band_bins(t, b).size]
    for h in (3, 4, 5, 6):                                               # every band of both channels one ulp under its floor
        for b in present:
            c[h, :, floor_bin(t, b)] = np.nextafter(t["floor"][b], DOWN) * (-1 if (h + b) % 2 else 1)
    c[7, 1, kf] = over
    s = situation(c, sr, Q)
    assert s["alive"][:, 24].tolist() == [True, True, False, False, False, False, False, True] and not s["alive"][:, :24].any()
    assert s["above"][0, :, 24].tolist() == [True, False] and s["above"][1, :, 24].tolist() == [False, True]
    for h in (3, 4, 5, 6):
        assert not s["above"][h].any() and s["masking"][h][:, [0, 22, 23, 24]].all(), (h, "masking-alive bands under their floors")
        assert not s["visit"][h].any()
    g = run_forms(ctx, "channels", c, sr, Q)
    assert {(h, ch, k) for h, ch, k in np.argwhere(g["q"] != 0).tolist()} == {(0, 0, kf), (1, 1, kf), (7, 1, kf)}
    frames = M.split_frames(g["data"], 2)
    for h in (2, 3, 4, 5, 6):
        assert frames[h][1] == [M.EMPTY_BLOB, M.EMPTY_BLOB], (h, "an all-zero frame")


# ------------------------------------------------------------------------------------------------ alternating frames
def test_blocks_5_to_7_alive_and_dead_in_turn(ctx):
    sr = 44100
    t = ath_floor_tables.load(sr, Q)
    k24 = band_bins(t, 24)
    top = [int(k24[(k24 // 128) == blk][7]) for blk in (5, 6, 7)]          # a band-24 bin in each of blocks 5, 6, 7
    assert all(t["ath_lin"][k] < 3000 for k in top)
    live = [1, 0, 1, 0, 1, 1, 0, 0, 1, 0, 0, 1]                           # alive and dead on even and on odd frames
    assert {(h % 2, v) for h, v in enumerate(live)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    c = np.zeros((len(live), 2, 1024), np.float32)
    under = np.nextafter(t["floor"][24], DOWN)
    for h, v in enumerate(live):
        ch = h % 2
        c[h, :, 10 + h] = np.float32(50.0 + 7 * h)                        # block 0 is alive in every frame
        for i, k in enumerate(top):
            # alive: 4 x the bin's ATH amplitude and more, another size every frame; dead: the same bins under the band's floor
            c[h, ch, k] = np.float32(4.0 + 0.5 * h + i) * t["ath_lin"][k] * (-1 if i == 1 else 1) if v else under
    s = situation(c, sr, Q)
    assert s["visit"][:, 0].all() and not s["visit"][:, 1:5].any()
    for h, v in enumerate(live):
        assert s["visit"][h, 5:].tolist() == [bool(v)] * 3, (h, s["visit"][h].tolist())
    g = run_forms(ctx, "alternate", c, sr, Q)
    nz = g["q"] != 0
    for h, v in enumerate(live):
        assert nz[h, h % 2, top].tolist() == [bool(v)] * 3 and nz[h, :, 10 + h].all(), h
    assert int(nz.sum()) == 2 * len(live) + 3 * sum(live)


# ------------------------------------------------------------------------------------------------ non-finite
def test_inf_and_nan_in_band_24(ctx):
    sr = 44100
    t = ath_floor_tables.load(sr, Q)
    k24 = band_bins(t, 24)
    k0, k1 = int(k24[0]), int(k24[5])
    big = np.float32(8.0) * t["ath_lin"][k1]
    c = np.zeros((10, 2, 1024), np.float32)
    c[0, 0, k0], c[0, 0, k1] = np.nan, big                               # NaN energy, finite maximum far above the floor
    c[1, 0, k0], c[1, 0, k1], c[1, 1, k1] = np.nan, big, -big            # ... next to a finite band in the other channel
    c[2, 1, k1] = big
    c[3, 0, k1] = big
    c[4, 1, k0], c[4, 1, k1] = np.nan, big
    c[5, 0, k0] = np.inf                                                 # alone in a quiet frame
    c[6, 0, k0], c[6, 1, k1] = -np.inf, big                              # the other channel keeps band 24 alive
    c[7, 0, k1] = big                                                    # channel 0's level is infinite from frame 5 on
    c[8, 1, k1] = big
    c[9, 0, k1], c[9, 1, k0] = big, np.inf
    s = situation(c, sr, Q)
    # a NaN band energy is a band level of -100 dB to the reference (its `> 1e-10` is false) and its maxima skip NaN: the
    # masking amplitude stays finite, the band alive. An infinite one leaves a masking amplitude of +inf, for good
    assert s["masking"][0, 0, 24] and s["above"][0, 0, 24] and s["alive"][:5, 24].all()
    assert s["above"][5, 0, 24] and not s["masking"][5, 0, 24] and not s["alive"][5].any()
    assert s["alive"][:, 24].tolist() == [True] * 5 + [False, True, False, True, False]
    assert s["above"][[7, 9], 0, 24].all() and not s["masking"][[7, 9]][:, :, 24].any()        # above the floor, no masking amplitude below
    g = run_forms(ctx, "nonfinite", c, sr, Q)
    kept = {(h, ch, k) for h, ch, k in np.argwhere(g["q"] != 0).tolist()}
    assert kept == {(0, 0, k1), (1, 0, k1), (1, 1, k1), (2, 1, k1), (3, 0, k1), (4, 1, k1), (6, 1, k1), (8, 1, k1)}, sorted(kept)
    assert kept == {(h, ch, k) for h, ch, k in np.argwhere(O.lossy_quantize(c, sr, Q)["q"] != 0).tolist()}


# ------------------------------------------------------------------------------------------------ block and general form
def test_block_and_general_form_with_dead_blocks_behind(ctx):
    sr = 44100
    amp = M.AMP
    c = np.zeros((8, 2, 1024), np.float32)
    sign = np.where(np.arange(1024) % 3 == 0, -1.0, 1.0).astype(np.float32)
    c[0, 0, 0:200] = amp * sign[0:200]                                   # 200 non-zeros in blocks 0 and 1: block form, blocks 2-7 dead
    c[0, 1, 5] = amp
    c[1, 0, 3] = amp
    c[1, 1, 130:330] = amp * sign[130:330]                               # blocks 1 and 2; block 0 and blocks 3-7 dead
    c[2, :, 0:256] = (amp * sign[0:256])[None]                           # both channels, a run of 256: general form
    c[3, 0, 0:384:2] = amp                                               # 192 runs of one: general form, blocks 3-7 dead
    c[3, 1, 730] = amp                                                   # ... and blocks 5-7 alive through the other channel's band 24
    c[4, 0, 256:512] = amp * sign[256:512]                               # dead blocks in front of and behind a general form
    c[5, 1, 0:129] = amp * sign[0:129]                                   # 129 non-zeros: the item form's first decline
    s = situation(c, sr, Q)
    assert s["visit"][0].tolist() == [True, True] + [False] * 6 and s["visit"][1].tolist() == [True, True, True] + [False] * 5
    # (band 21 reaches from block 2 into block 3: visited, all zeros) band 24: blocks 5 to 7
    assert s["visit"][3].tolist() == [True, True, True, True, False, True, True, True]
    # (bands 20 and 22 reach into blocks 1 and 4) dead blocks in front of and behind the visited ones
    assert s["visit"][4].tolist() == [False, True, True, True, True, False, False, False]
    assert s["visit"][5].tolist() == [True, True] + [False] * 6 and not s["visit"][6].any() and not s["visit"][7].any()
    g = run_forms(ctx, "dense_q055", c, sr, Q)
    forms = [[M.channel_form(g["q"][h, ch])[0] for ch in range(2)] for h in range(6)]
    assert forms == [["block", "item"], ["item", "block"], ["general", "general"], ["general", "item"], ["general", "item"],
                     ["item", "block"]], forms
    assert np.array_equal(g["q"] != 0, c != 0)
    # q = 0.99: every coefficient above 1e-10 and its bin's ATH amplitude is kept; a dense frame of many runs, nothing behind it
    q = 0.99
    t = ath_floor_tables.load(sr, q)
    d = np.zeros((8, 2, 1024), np.float32)
    d[0, 0, 0:600] = (np.float32(100.0) + np.arange(600, dtype=np.float32)) * sign[0:600]
    d[0, 0, 0:600:4] = 0                                                 # 150 runs of three
    d[0, 1, 0:300] = np.float32(300.0) * sign[0:300]
    d[1, 1, 0:512] = d[0, 0, 0:512]
    d[2, 0, 100] = np.float32(5.0)
    d[3, :, 0:640:2] = np.float32(77.0)
    assert (np.abs(d[d != 0]) > 4 * np.broadcast_to(t["ath_lin"], d.shape)[d != 0]).all()
    s = situation(d, sr, q)
    # (band 23 reaches from block 4 into block 5, band 22 from block 3 into block 4)
    assert s["visit"][0].tolist() == [True] * 6 + [False] * 2 and s["visit"][1].tolist() == [True] * 5 + [False] * 3
    assert s["visit"][2].tolist() == [True] + [False] * 7
    assert s["visit"][3].tolist() == [True] * 6 + [False] * 2 and not s["visit"][4:].any()
    g = run_forms(ctx, "dense_q099", d, sr, q)
    assert M.channel_form(g["q"][0, 0])[0] == "general" and M.channel_form(g["q"][0, 1])[0] == "general"
    assert M.channel_form(g["q"][3, 0])[0] == "general"
    assert np.array_equal(g["q"] != 0, d != 0)
