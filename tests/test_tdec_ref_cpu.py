"""The f64 reference of the transform decoder (tdec_ref) against the oracle's f32 decoder, on the CPU: before
test_gpu_tdecode.py counts the device's error in units of the oracle's, the reference and the oracle have to agree on every
case the device is held to, and the unit has to be what it is believed to be. Each test prints, per case, the oracle's
worst max|err| / scale over the blocks and its relative RMS error (measured: 2.0e-7 ... 3.9e-7 and 1.0e-7 ... 1.5e-7)."""
import numpy as np

import tdec_ref as T
from oracle import oracle as O

CEILING = 1e-6     # a sanity ceiling on the yardstick, not the device's bound: beyond it the case or the reference is wrong


def _report(name, m):
    print(f"{name:34s} oracle worst max|err|/scale {m['worst']:.2e} at block {m['at'][0]} channel {m['at'][1]} position {m['at'][2]}, "
          f"relative RMS {m['rms']:.2e}, {m['blocks']} blocks compared")


def _check(name, flo):
    sr, ch, frames = T.describe(flo)
    got, gsr, gch = O.decode(flo)
    ref, scale, m = T.yardstick(name, flo)
    assert (gsr, gch) == (sr, ch) and got.shape == ref.shape == ((len(frames) - 1) * 1024 * ch,), name
    assert scale.shape == (len(frames) - 1, ch), name            # every (block, channel) is compared: none is left out
    assert np.isfinite(ref).all() and m["finite"], name
    assert m["zero_ok"], (name, "a block of scale 0 is not exactly zero in the oracle")
    _report(name, m)
    assert m["worst"] < CEILING and m["rms"] < CEILING, (name, m)
    return m


def test_band_map_is_freq_to_bark_band_in_f32():
    for sr in T.RATES + [32000, 12000, 88200]:
        assert np.array_equal(T.band_map(sr), O.psy_tables(sr)[1]), sr
    assert int(T.band_map(8000).max()) == 17          # 8 kHz has 18 bands
    assert len(set(T.band_map(384000))) < 25          # and the highest rates skip some of the lowest


def test_oracle_agrees_with_the_f64_reference_on_hand_made_files():
    worst = rms = 0.0
    for name in T.HAND_MADE:
        m = _check(name, T.hand_made(name))
        worst, rms = max(worst, m["worst"]), max(rms, m["rms"])
    print(f"hand-made files: oracle worst {worst:.2e}, relative RMS at most {rms:.2e}")


def test_oracle_agrees_with_the_f64_reference_on_encoder_made_files():
    # (the device tests encode with the device; the oracle's encoder makes the same kind of file for the CPU)
    for name, flo in T.encoder_cases(O.encode_lossy):
        _check(name, flo)


def test_absent_channels_keep_their_overlap():
    # the rule the reference restates, on the smallest file that shows it: channel 1 is carried by frames 0, 2 and 4 only;
    # block 1 (frame 2) starts with frame 0's second half, block 3 (frame 4) with frame 2's, blocks 0 and 2 are silent
    rng = np.random.default_rng(1)
    frames = [[(T._words(rng, 33000, 35000), T._ints(rng, 0.2, 3000)) for _ in range(n)] for n in (2, 1, 2, 1, 2)]
    flo = T._file(44100, 2, frames)
    ref, scale = T.decode(flo)
    r = ref.reshape(4, 1024, 2)
    assert not r[0, :, 1].any() and not r[2, :, 1].any() and scale[0, 1] == 0 and scale[2, 1] == 0
    alone = T.decode((44100, 1, [[frames[0][1]], [frames[2][1]], [frames[4][1]]]))[0].reshape(2, 1024)
    assert np.array_equal(r[1, :, 1], alone[0]) and np.array_equal(r[3, :, 1], alone[1])
    _check("alternating 2/1/2/1/2", flo)


def test_edge_class_is_outside_the_f64_bound():
    # why words 1 - 600 and 62000 - 65535 are held to the oracle and not to float64: the first overflow inside the
    # oracle's own f32 transform, the second give subnormal values, where an f32 result is no longer within 1e-6
    for name, flo in T.edge_cases():
        o = O.decode(flo)[0]
        ref, scale = T.decode(flo)
        m = T.measure(o, ref, scale)
        print(f"{name:34s} oracle: {int(np.isnan(o).sum())} NaN, {int(np.isinf(o).sum())} inf of {o.size}, worst {m['worst']:.2e}")
        assert o.shape == ref.shape
        assert not m["finite"] or float(np.abs(o).max()) < 1e-25, name          # NaN throughout, or factors of 2^-114 and less
