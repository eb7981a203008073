"""Band statistics of the stereo chain encode (lossy_chain2q_kernel, form 5) by lane masks: segment stores under
exec = close[e] to one running slot address per lane, no kRowKeep / kRowDst rows, the gathers as before. Forms 1 (one wave
per channel, band_stats<CH>) and 2 (frame-parallel, the unmasked band_stats_2) are the independent yardsticks: every file of
form 5 equals the same clip's file under both, byte for byte.

Clips are stereo, q = 0.55. A clip of n sample-frames has ceil((n + 1024) / 1024) frames: 0, 700, 1500 and 3500 sample-frames
give 1, 2, 3 and 5 frames, so both unrolled frame bodies, an odd tail and the last frame's masking pass run, and from the
second frame on the slots are written again, through a slot address that must have been set anew.

    44.1 kHz        the DIRTY = 0xBDBE instantiation (twelve masked positions)
    48 kHz          the generic instantiation (sixteen positions, some masks empty)
    96 kHz          the generic instantiation with cold gather groups behind the three hot ones
    silence         every segment sum and maximum is zero
    edges           a full-scale tone on the last bin of every band and of every lane: every closing lane closes a segment
                    that is not zero, at every position
    inf, nan        one sample of channel 0 replaced: the restart must give inf x 0 = NaN as the row's 0.0 did
    seven clips     unequal frame counts (1, 5, 2, 3, 1, 2, 5 frames) at six clip slots per workgroup; and the same seven
                    lengths cycled over more clips than the device has compute units at one slot per workgroup, where
                    every slot is certain to take a second clip
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
EDGES = np.array([0, 100, 200, 300, 400, 510, 630, 770, 920, 1080, 1270, 1480, 1720, 2000, 2320, 2700, 3150, 3700,
                  4400, 5300, 6400, 7700, 9500, 12000, 15500, 20500], dtype=np.float32)


def frames(n):
    return (n + 1024 + 1023) // 1024


def band_map(sr):
    f = (np.arange(1024, dtype=np.float32) + np.float32(0.5)) * (np.float32(sr) / np.float32(2048))
    return np.minimum(np.searchsorted(EDGES[1:], f, side="right"), 24)


def edge_clip(sr, n):
    """a tone of amplitude 1 on the centre of the last bin of every band and of every lane's sixteen (channel 1: other phases)"""
    band = band_map(sr)
    bins = sorted({k for k in range(1024) if k % 16 == 15 or k == 1023 or band[k + 1] != band[k]})
    t = np.arange(n, dtype=np.float64) / sr
    x = np.zeros((n, 2))
    for k in bins:
        w = 2 * np.pi * (k + 0.5) * sr / 2048
        x[:, 0] += np.sin(w * t + 0.1 * k)
        x[:, 1] += np.sin(w * t + 0.37 * k + 1.0)
    return x.astype(np.float32).reshape(-1)


def with_sample(x, value):
    y = x.copy()
    y[2 * 1300] = np.float32(value)      # channel 0, in the second frame's new half
    return y


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
    check(ctx, [signals.music_like(sr, n, CH, seed=70 + i) for i, n in enumerate(HOP_LENS)], sr, "music")


@pytest.mark.parametrize("sr", [44100, 48000, 96000])
def test_digital_silence(ctx, sr):
    check(ctx, [np.zeros(2 * 3500, np.float32)], sr, "silence")


@pytest.mark.parametrize("sr", [44100, 48000, 96000])
def test_full_scale_bin_on_every_band_edge(ctx, sr):
    check(ctx, [edge_clip(sr, 3500)], sr, "edges")


@pytest.mark.parametrize("value", [np.inf, -np.inf, np.nan])
@pytest.mark.parametrize("sr", [44100, 48000, 96000])
def test_non_finite_sample(ctx, sr, value):
    base = signals.music_like(sr, 3500, CH, seed=81)
    check(ctx, [with_sample(base, value), base], sr, f"sample {value}")


def test_seven_clips_of_unequal_frame_counts(ctx):
    lens = [0, 3500, 700, 1500, 0, 1000, 4096]
    assert [frames(n) for n in lens] == [1, 5, 2, 3, 1, 2, 5]
    seven = [signals.music_like(44100, n, CH, seed=90 + i) for i, n in enumerate(lens)]
    want = check(ctx, seven, 44100, "seven clips, six slots per workgroup", override=6)
    # more clips than workgroups at one slot each: every slot serves clips of different lengths one after the other
    n = int(ctx.device_info()[1]) + 7
    many = [seven[i % 7] for i in range(n)]
    got = encode(ctx, 5, many, 44100, override=1)
    for i, g in enumerate(got):
        assert g == want[i % 7], f"clip {i} of {n} at one slot per workgroup differs from the seven-clip batch at byte {first_difference(g, want[i % 7])}"
