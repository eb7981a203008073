"""flo_amd.StreamingDecoder without a context (parsing and counters only, no device) against tests/sdec_model.py, and the
model itself against the oracle's whole-file decode. Runs without a GPU."""
import glob
import os
import struct

import numpy as np
import pytest

import flo_amd
import flofile
from conftest import EXAMPLES
from oracle import oracle as O
from sdec_model import ModelError, StreamingDecoderModel

FILES = sorted(glob.glob(os.path.join(EXAMPLES, "*.flo")))
CHUNKS = [1, 7, 69, 70, 71, 100, 4096, None]


def _snap(d):
    i = d.info()
    return (int(d.state()), d.frames_available(), d.available_frames(), d.buffered_bytes(),
            None if i is None else (i.sample_rate, i.channels, i.bit_depth, i.total_samples, i.is_lossy))


def _feed_both(d, m, chunk):
    try:
        want = m.feed(chunk)
    except ModelError as e:
        want = ("error", str(e))
    try:
        got = d.feed(chunk)
    except flo_amd.FloError as e:
        got = ("error", str(e))
    return got, want


def _run(b, step):
    d, m = flo_amd.StreamingDecoder(), StreamingDecoderModel()
    step = step or len(b)
    for at in range(0, len(b), step):
        got, want = _feed_both(d, m, b[at:at + step])
        assert got == want, at
        assert _snap(d) == m.snapshot(), at
    got, want = _feed_both(d, m, b"\0" * 3)   # feed after the end (or after Error)
    assert got == want and _snap(d) == m.snapshot()
    return d, m


@pytest.mark.parametrize("step", CHUNKS)
@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_feed_counters_equal_the_model(path, step):
    _run(open(path, "rb").read(), step)


def test_no_context_cannot_decode():
    b = open(FILES[0], "rb").read()
    d = flo_amd.StreamingDecoder()
    assert d.feed(b)
    assert d.state() == flo_amd.DecoderState.Ready
    assert d.current_frame_index() == 0
    d.reset()
    assert d.state() == flo_amd.DecoderState.WaitingForHeader and d.buffered_bytes() == 0 and d.info() is None


def _lossless_file(frames, ch=2):
    return flofile.build_lossless(44100, ch, frames)


def _malformed():
    ok = {"coeffs": [1], "shift": 0, "k": 2, "residuals": b"\x55" * 40}
    good = _lossless_file([(1, 64, 0, [ok, ok]), (1, 64, 0, [ok, ok])])
    out = {"bad_magic": b"FLX!" + good[4:]}
    # short toc_size: the header says fewer bytes than the entries need
    b = bytearray(good)
    struct.pack_into("<Q", b, 38, 4 + 20)   # two entries declared, room for one
    out["short_toc"] = bytes(b)
    out["truncated_frame"] = _lossless_file([(1, 64, 0, [ok, ok])])[:-30]
    # LPC order 13, an ALPC wrapper too small, a missing rice parameter, an empty ALPC wrapper (silence)
    lpc13 = bytes([13]) + b"\0" * 60
    out["lpc13"] = flofile.build_lossless(44100, 1, [(1, 64, 0, [lpc13])])
    out["alpc_small"] = flofile.build_lossless(44100, 1, [(1, 64, 0, [bytes([2, 1, 0])])])
    out["missing_rice"] = flofile.build_lossless(44100, 1, [(1, 64, 0, [bytes([0, 0, 0])])])
    out["empty_alpc"] = flofile.build_lossless(44100, 1, [(3, 64, 0, [b""])])
    return out


@pytest.mark.parametrize("name", list(_malformed()))
@pytest.mark.parametrize("step", [1, 13, 70, None])
def test_malformed_equal_the_model(name, step):
    _run(_malformed()[name], step)


def test_short_toc_pushes_entries_again():
    b = _malformed()["short_toc"]
    d, m = _run(b, 100)   # the first feed holds the first entry only
    assert len(m.toc) == 3   # the quirk: entries pushed on every feed that re-read them


def test_model_parse_errors():
    for name, msg in [("lpc13", "Invalid LPC order"), ("alpc_small", "ALPC channel too small"), ("missing_rice", "Missing rice parameter")]:
        m = StreamingDecoderModel()
        m.feed(_malformed()[name])
        for _ in range(2):   # the same frame fails again
            with pytest.raises(ModelError, match=msg):
                m.next_frame()
            assert m.current == 0


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_model_equals_oracle_decode(path):
    b = open(path, "rb").read()
    m = StreamingDecoderModel()
    m.feed(b)
    parts = []
    while True:
        x = m.next_frame()
        if x is None:
            break
        parts.append(x)
    assert m.state == 3
    got = np.concatenate(parts) if parts else np.zeros(0, np.float32)
    want = O.decode(b)[0]
    assert got.size == want.size
    if m.is_lossy:
        assert float(np.abs(got - want).max(initial=0)) <= 2e-6
    else:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
