"""Clip slots of the stereo chain encode (lossy_chain2q_kernel, form 5): which wave serves which slot, and which transform
wave of a SIMD has issue priority, must not show in the bytes. Every case: stereo, q = 0.55, clip lengths cycling through
1, 1023, 1024, 1025, 2500 and 5000 sample-frames; every file of form 5 equals the same batch under form 1 (the independently
written chain, one wave per channel), and a second encode of the batch gives the first one's bytes (a race between waves
of different priority would not repeat).

    FLO_CHAIN2X_CLIPS = 1 .. 6, 13 clips   one round; the pairs whose first claim fails take the tail path
    300 clips at override 1                persistent workgroups, slots take second clips
    1030 clips, no override                g = 5 by batch size: the shape of a 1250-clip shard
"""
import os

import numpy as np
import pytest

import flo_amd  # noqa: F401
import lossy_model as M
from gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu
SR, CH, Q = 44100, 2, 0.55
LENS = [1, 1023, 1024, 1025, 2500, 5000]
_clips, _form1 = {}, {}


def clip(i):
    """content by i mod 97 (two music-like clips among tone bursts), length by i mod 6"""
    key = (LENS[i % len(LENS)], i % 97)
    if key not in _clips:
        _clips[key] = M.ragged_clip(key[0], CH, key[1])
    return _clips[key]


def form1(ctx, n):
    """the batch of n clips under form 1, encoded once"""
    if n not in _form1:
        ctx.force_path(1)
        try:
            _form1[n] = ctx.encode_batch(1, [clip(i) for i in range(n)], SR, CH, Q)
        finally:
            ctx.force_path(0)
    return _form1[n]


def form5_twice(ctx, n, override):
    old = os.environ.get("FLO_CHAIN2X_CLIPS")
    if override:
        os.environ["FLO_CHAIN2X_CLIPS"] = str(override)
    else:
        os.environ.pop("FLO_CHAIN2X_CLIPS", None)
    ctx.force_path(5)
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        clips = [clip(i) for i in range(n)]
        out = [ctx.encode_batch(1, clips, SR, CH, Q) for _ in range(2)]
        launches = ctx.profile_query("lossy_chain2q")[1]
    finally:
        ctx.profile_enable(False)
        ctx.force_path(0)
        if old is None:
            os.environ.pop("FLO_CHAIN2X_CLIPS", None)
        else:
            os.environ["FLO_CHAIN2X_CLIPS"] = old
    assert launches == 2, ("lossy_chain2q launches", launches)
    return out


def first_difference(a, b):
    n = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))
    return int(d[0]) if d.size else (n if len(a) != len(b) else None)


def check(ctx, n, override):
    want = form1(ctx, n)
    first, second = form5_twice(ctx, n, override)
    assert len(first) == len(second) == len(want) == n
    for tag, got, ref in (("form 5 against form 1", first, want), ("second encode against the first", second, first)):
        for i, (f, r) in enumerate(zip(got, ref)):
            assert f == r, (f"{n} clips, override {override}: {tag}: clip {i} ({LENS[i % len(LENS)]} sample-frames) differs at byte "
                            f"{first_difference(f, r)} (lengths {len(f)} / {len(r)})")


@pytest.mark.parametrize("g", [1, 2, 3, 4, 5, 6])
def test_one_round_of_13_clips_at_every_workgroup_size(ctx, g):
    check(ctx, 13, g)


def test_persistent_slots_take_second_clips(ctx):
    cus = int(ctx.device_info()[1])
    assert 300 > cus, "the batch must hold more clips than the device has compute units"
    check(ctx, 300, 1)


def test_g5_by_batch_size(ctx):
    assert M.source_constants()["kChain2qFill"] == 256 and (1030 + 255) // 256 == 5
    check(ctx, 1030, 0)
