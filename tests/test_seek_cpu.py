"""flo_amd.get_toc / seek_to_time (libflo/src/seeking.rs) against a restatement of their semantics written here from the
container layout: the TOC read from the bytes, the rightmost-timestamp binary search, the clamp to the frames read, the
sample offset and the last frame's duration. Runs without a GPU."""
import glob
import os
import struct

import pytest

import flo_amd
from conftest import EXAMPLES

FILES = sorted(glob.glob(os.path.join(EXAMPLES, "*.flo")))
BOUNDARIES = [0, 1, 1000, 1001, 2999, 3000, 4999, 5000, 6000, 10000]


def _read(b):
    """header fields, TOC entries and the frame_samples of the frames the reader accepts (frames starting inside DATA)"""
    sr = struct.unpack_from("<I", b, 8)[0]
    toc_size, data_size = struct.unpack_from("<QQ", b, 38)
    pos = 70
    toc = []
    if toc_size >= 4:
        n = struct.unpack_from("<I", b, pos)[0]
        pos += 4
        for _ in range(n):
            toc.append(struct.unpack_from("<IQII", b, pos))   # frame_index, byte_offset, frame_size, timestamp_ms
            pos += 20
    data_start = pos
    samples = []
    for e in toc:
        fs = data_start + e[1]
        if fs >= data_start + data_size:
            break
        samples.append(struct.unpack_from("<I", b, fs + 1)[0])
    return sr, toc, samples


def _seek(b, t):
    sr, toc, samples = _read(b)
    if not toc:
        raise flo_amd.FloError("No TOC available for seeking")
    lo, hi = 0, len(toc) - 1
    while lo < hi:
        mid = lo + (hi - lo + 1) // 2
        if toc[mid][3] <= t:
            lo = mid
        else:
            hi = mid - 1
    fi = min(lo, len(samples) - 1)
    ts = toc[fi][3]
    if fi + 1 < len(toc):
        nxt = toc[fi + 1][3]
    else:
        nxt = (ts + samples[fi] * 1000 // sr) & 0xFFFFFFFF
    off = min(max(t - ts, 0) * sr // 1000 & 0xFFFFFFFF, samples[fi])
    return (fi, toc[fi][1], ts, off, nxt)


def test_fixture_count():
    assert len(FILES) >= 18


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_toc_and_seek_match_restatement(path):
    b = open(path, "rb").read()
    _, toc, _ = _read(b)
    got = flo_amd.get_toc(b)
    assert [tuple(e) for e in got] == [(i, o, s, t) for i, o, s, t in [(e[0], e[1], e[2], e[3]) for e in toc]]
    times = set(BOUNDARIES)
    for e in toc:
        times.update({max(e[3] - 1, 0), e[3], e[3] + 1})
    for t in sorted(times):
        assert tuple(flo_amd.seek_to_time(b, t)) == _seek(b, t), (path, t)


def _some_file():
    return open(next(p for p in FILES if "lossless" in os.path.basename(p)), "rb").read()


def test_empty_toc_message():
    b = bytearray(_some_file())
    struct.pack_into("<Q", b, 38, 0)   # toc_size = 0: the reader reads no TOC, the bytes behind the header become DATA
    assert flo_amd.get_toc(bytes(b)) == []
    with pytest.raises(flo_amd.FloError, match="No TOC available for seeking"):
        flo_amd.seek_to_time(bytes(b), 0)


def test_truncated_files_give_reader_messages():
    b = _some_file()
    for cut in (0, 3, 10, 69, 71, 80):
        for fn in (flo_amd.get_toc, lambda d: flo_amd.seek_to_time(d, 5)):
            with pytest.raises(flo_amd.FloError) as e:
                fn(b[:cut])
            try:
                flo_amd.probe_container(b[:cut])
                msg = None
            except flo_amd.FloError as pe:
                msg = str(pe)
            assert str(e.value) == msg


def test_no_crash_where_the_reference_panics():
    b = bytearray(_some_file())
    # TOC entries whose frames all start past DATA: the reference's `frames.len() - 1` underflows
    n = struct.unpack_from("<I", b, 70)[0]
    for i in range(n):
        struct.pack_into("<Q", b, 74 + 20 * i + 4, 1 << 40)
    assert len(flo_amd.get_toc(bytes(b))) == n
    with pytest.raises(flo_amd.FloError):
        flo_amd.seek_to_time(bytes(b), 0)
    # a zero sample rate on the last frame's duration: the reference divides by zero
    b = bytearray(_some_file())
    struct.pack_into("<I", b, 8, 0)
    with pytest.raises(flo_amd.FloError):
        flo_amd.seek_to_time(bytes(b), 10 ** 9)
