"""CRC32 of the stereo many-clips batch computed in the chain encode's idle tail (lossy_kernels.hip, tail_crc) with
finish_files_kernel<256> computing whatever the tail did not reach: the files must not depend on how far the tail got.
FLO_TAIL_CRC=0 switches the tail off (every CRC then comes from finish_files); the one-wave-per-channel form (1) takes
the separate crc_slices_kernel path and is a third, independent maker of the same files."""
import os
import zlib

import numpy as np
import pytest

import flofile
from gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu


def _files(b):
    return [b.fetch(i) for i in range(b.n_clips)]


def _check_crcs(files):
    for i, f in enumerate(files):
        p = flofile.parse(f)
        assert (zlib.crc32(p.data) & 0xFFFFFFFF) == p.data_crc32, f"clip {i}: header CRC differs from zlib over DATA"


def _encode(b, tail=True):
    old = os.environ.get("FLO_TAIL_CRC")
    if tail:
        os.environ.pop("FLO_TAIL_CRC", None)
    else:
        os.environ["FLO_TAIL_CRC"] = "0"
    try:
        b.encode(5)
        b.sync()
    finally:
        if old is None:
            os.environ.pop("FLO_TAIL_CRC", None)
        else:
            os.environ["FLO_TAIL_CRC"] = old
    return _files(b)


def _pairs(ctx):
    # persistent workgroups of the lock-step form: one per CU, six (transform, packer) pairs each once the batch is large
    return 6 * ctx.device_info()[1]


def _run(ctx, n_interleaved, seed):
    import flo_amd
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, n_interleaved, 44100, 2, 0.55)
    try:
        b.fill_synthetic(seed=seed, clip_id0=7)
        with_tail = _encode(b)
        _check_crcs(with_tail)
        assert sum(len(flofile.parse(f).data) for f in with_tail) == b.data_bytes()
        again = _encode(b)                  # the next epoch: counters and ready words of the launch before are stale
        assert again == with_tail
        fallback = _encode(b, tail=False)   # every CRC from finish_files_kernel<256>
        assert fallback == with_tail
        after = _encode(b)                  # the tail back on, two epochs later
        assert after == with_tail
        b.encode(1)                         # one wave per channel: crc_slices_kernel + finish_files_kernel<256>
        b.sync()
        assert _files(b) == with_tail
    finally:
        b.close()
    return with_tail


def test_fewer_clips_than_pairs(ctx):
    # 100 clips: one pair each, so every clip is its pair's last and is CRC-ed by its own packer (or by finish_files)
    _run(ctx, [2 * 44100] * 100, 0x7A11)


def test_exactly_one_round(ctx):
    _run(ctx, [2 * 44100] * _pairs(ctx), 0x7A12)


def test_one_clip_more_than_a_round(ctx):
    files = _run(ctx, [2 * 44100] * (_pairs(ctx) + 1), 0x7A13)
    assert len(files) == _pairs(ctx) + 1


def test_ragged_lengths_with_one_frame_clips(ctx):
    rng = np.random.default_rng(5)
    n = 2 * _pairs(ctx) + 37
    lens = rng.integers(0, 3 * 44100, n)
    lens[::7] = 0          # no samples: one frame
    lens[3::11] = 1        # one sample-frame: two frames
    lens[5::13] = 1023     # the first frame boundary
    lens[9::17] = 6 * 44100
    files = _run(ctx, [2 * int(x) for x in lens], 0x7A14)
    for i in np.nonzero(lens == 0)[0][:5]:
        assert len(flofile.parse(files[i]).frames) == 1


def test_many_short_clips(ctx):
    # five rounds of 0.2-second clips: most clips go through the done queue
    _run(ctx, [2 * 8820] * (5 * _pairs(ctx) + 11), 0x7A15)


def test_two_batches_interleaved(ctx):
    # two batches, each with its own epochs and queues, encoded alternately
    import flo_amd
    m = _pairs(ctx) + 3
    a = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [44100 * 2] * m, 44100, 2, 0.55)
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [30000 * 2] * (m // 2), 44100, 2, 0.55)
    try:
        a.fill_synthetic(seed=1, clip_id0=0)
        b.fill_synthetic(seed=2, clip_id0=0)
        fa, fb = _encode(a), _encode(b)
        _check_crcs(fa)
        _check_crcs(fb)
        for _ in range(2):
            assert _encode(a) == fa
            assert _encode(b) == fb
    finally:
        a.close()
        b.close()
