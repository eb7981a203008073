"""The windowed overlap carry of the stereo chain encode (lossy_chain2q_kernel, form 5): a half-frame is folded once as the
new half, its contribution to the next frame (the a-parts, fold_carry_2) is carried in registers instead of the samples, and
the rotation twiddles stay in registers for the launch. Forms 1 (one wave per channel, fold<CH>) and 2 (frame-parallel,
fold_2 over both halves) are the independent yardsticks: every file of form 5 equals the same clip's file under both, byte
for byte.

Clips are stereo, q = 0.55. A clip of n sample-frames has ceil((n + 1024) / 1024) frames.

    frame counts    0, 700, 1500, 3500 sample-frames (1, 2, 3, 5 frames) at 44.1, 48 and 96 kHz: a clip that is only the
                    pre-roll's carry, odd and even counts, every instantiation
    half edges      a unit impulse on the first and the last sample-frame of the first two halves (0, 1023, 1024, 2047), the
                    other channel an impulse of the other sign on another of them; a DC clip (+1.0 / -0.5), where the
                    a-part's window and the b-part's differ
    zeros           a clip of -0.0 in both channels
    inf, nan        one sample replaced, where it is only ever a new half's (1300) and where it is a new half's and then
                    carried (2100 of 3500)
    carry reset     seven unequal clips at six slots per workgroup; the same lengths over (compute units + 7) clips at one
                    slot per workgroup, full-scale noise and all-zero clips in turn: a zero clip behind a noise clip on the
                    same slot must give the file of a zero clip encoded alone
"""
import os

import numpy as np
import pytest

import flo_amd  # noqa: F401
import signals
from gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu
CH, Q = 2, 0.55
HOP_LENS = [0, 700, 1500, 3500]          # 1, 2, 3, 5 frames
EDGE_POS = [0, 1023, 1024, 2047]


def frames(n):
    return (n + 1024 + 1023) // 1024


def encode(ctx, which, clips, sr, override=None):
    old = os.environ.get("FLO_CHAIN2X_CLIPS")
    if override:
        os.environ["FLO_CHAIN2X_CLIPS"] = str(override)
    else:
        os.environ.pop("FLO_CHAIN2X_CLIPS", None)
    ctx.force_path(which)
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        out = ctx.encode_batch(1, clips, sr, CH, Q)
        launches = ctx.profile_query("lossy_chain2q")[1] if which == 5 else 0
    finally:
        ctx.profile_enable(False)
        ctx.force_path(0)
        if old is None:
            os.environ.pop("FLO_CHAIN2X_CLIPS", None)
        else:
            os.environ["FLO_CHAIN2X_CLIPS"] = old
    assert which != 5 or launches == 1, ("lossy_chain2q launches", launches)
    return out


def first_difference(a, b):
    n = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))
    return int(d[0]) if d.size else (n if len(a) != len(b) else None)


def check(ctx, clips, sr, tag, override=None, refs=(1, 2)):
    got = encode(ctx, 5, clips, sr, override)
    assert len(got) == len(clips)
    for which in refs:
        want = encode(ctx, which, clips, sr)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (f"{tag}, {sr} Hz: clip {i} ({clips[i].size // 2} sample-frames) of form 5 differs from form {which} at byte "
                            f"{first_difference(g, w)} (lengths {len(g)} / {len(w)})")
    return got


@pytest.mark.parametrize("sr", [44100, 48000, 96000])
def test_clips_of_1_2_3_and_5_frames(ctx, sr):
    assert [frames(n) for n in HOP_LENS] == [1, 2, 3, 5]
    check(ctx, [signals.music_like(sr, n, CH, seed=170 + i) for i, n in enumerate(HOP_LENS)], sr, "music")


def impulse_clip(p0, p1, n=3500):
    x = np.zeros((n, 2), np.float32)
    x[p0, 0] = 1.0
    x[p1, 1] = -1.0
    return x.reshape(-1)


@pytest.mark.parametrize("sr", [44100, 48000])
def test_impulses_on_the_edges_of_the_first_two_halves(ctx, sr):
    clips = [impulse_clip(p, EDGE_POS[(i + 1) % 4]) for i, p in enumerate(EDGE_POS)]
    check(ctx, clips, sr, "impulses at 0, 1023, 1024, 2047")


@pytest.mark.parametrize("sr", [44100, 48000])
def test_dc_and_minus_zero(ctx, sr):
    dc = np.tile(np.array([1.0, -0.5], np.float32), 3500)
    minus_zero = np.full(2 * 3500, -0.0, np.float32)
    assert np.signbit(minus_zero).all()
    check(ctx, [dc, minus_zero], sr, "dc +1.0 / -0.5, then -0.0")


@pytest.mark.parametrize("value", [np.inf, -np.inf, np.nan])
@pytest.mark.parametrize("sr", [44100, 48000])
def test_non_finite_sample_new_and_carried(ctx, sr, value):
    base = signals.music_like(sr, 3500, CH, seed=181)
    new_only, carried = base.copy(), base.copy()
    new_only[2 * 1300] = np.float32(value)         # channel 0: frame 1's new half, frame 2's carry
    carried[2 * 2100 + 1] = np.float32(value)      # channel 1: frame 2's new half, then carried into frame 3
    check(ctx, [new_only, carried, base], sr, f"sample {value}")


def test_carry_is_reset_between_the_clips_of_a_slot(ctx):
    sr = 44100
    lens = [0, 3500, 700, 1500, 0, 1000, 4096]
    assert [frames(n) for n in lens] == [1, 5, 2, 3, 1, 2, 5]
    seven = [signals.music_like(sr, n, CH, seed=190 + i) for i, n in enumerate(lens)]
    check(ctx, seven, sr, "seven clips, six slots per workgroup", override=6)
    # one slot per workgroup, more clips than workgroups: every slot takes a second clip, and noise and zeros alternate
    noise = [signals.fast_noise(2 * n, seed=200 + i, amp=1.0) for i, n in enumerate(lens)]
    zeros = [np.zeros(2 * n, np.float32) for n in lens]
    n = int(ctx.device_info()[1]) + 7
    many = [(zeros if i & 1 else noise)[i % 7] for i in range(n)]
    got = encode(ctx, 5, many, sr, override=1)
    zero_alone = {m: encode(ctx, 5, [np.zeros(2 * m, np.float32)], sr)[0] for m in sorted(set(lens))}
    noise_ref = encode(ctx, 1, noise, sr)
    for i, g in enumerate(got):
        want = zero_alone[lens[i % 7]] if i & 1 else noise_ref[i % 7]
        what = "a zero clip encoded alone" if i & 1 else "form 1's file of the noise clip"
        assert g == want, f"clip {i} of {n} ({lens[i % 7]} sample-frames) differs from {what} at byte {first_difference(g, want)}"
