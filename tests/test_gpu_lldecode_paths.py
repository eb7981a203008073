"""The parallel lossless decoder on every path of its tile tables, chain, residual stage, predictor rows and finish
(tests/lldec_model.py names them and holds the cases; tests/test_lldec_model_cpu.py shows that the cases reach them and
that the model's integers and floats are the oracle's).

Per case, against the oracle: the integers of flo_decode_lossless_i32 (the scalar finish) and the floats of flo_decode
(the vector finish where the frame allows it) bit for bit; and, read from the FLO_TRACE line of ll_decode_device, the
number of wrappers handed to the serial kernel by the host and by the device, which must be the model's exactly - a
parallel form that gives up silently, or keeps a wrapper it must give up, decodes the same values and fails here.

One case per group of PATHS (and every kind of handover) also goes through the other builders of wrapper lists - a
Corpus window over the whole file, a StreamingDecoder fed the whole file, decode_frame_at frame by frame - against the
oracle's floats. Those paths print no counts (the trace line belongs to ll_decode_device), so only values are compared
there. Every case is decoded once more with FLO_LL_DECODE_SERIAL set, which holds the serial kernel to the oracle on the
same inputs. Needs an MI355X."""
import re

import numpy as np
import pytest

import flo_amd
import lldec_model as M
from gpu_util import ctx  # noqa: F401
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in M.cases()]
LINE = re.compile(r"\[flo\] ll decode: serial by the host (\d+), by the device (\d+)")

_ORACLE = {}


def oracle(name):
    """the oracle's (integers, floats) of a case, computed once"""
    if name not in _ORACLE:
        flo = M.case(name)["flo"]
        _ORACLE[name] = (O.decode_lossless_i32(flo)[0], O.decode(flo)[0])
        for a in _ORACLE[name]:
            a.setflags(write=False)
    return _ORACLE[name]


def same_bits(got, want, who):
    assert got.shape == want.shape, (who, got.shape, want.shape)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (who, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("name", NAMES)
def test_values_and_handovers(ctx, name, monkeypatch, capfd):
    c = M.case(name)
    oi, of = oracle(name)
    monkeypatch.setenv("FLO_TRACE", "1")
    capfd.readouterr()
    di = ctx.decode_lossless_i32(c["flo"])
    df = ctx.decode(c["flo"])
    err = capfd.readouterr().err
    monkeypatch.delenv("FLO_TRACE")
    same_bits(di, oi, "integers")
    same_bits(df, of, "floats")
    counts = [(int(a), int(b)) for a, b in LINE.findall(err)]
    print(f"{name}: serial by the host {counts[0][0] if counts else '?'}, by the device {counts[0][1] if counts else '?'}; "
          f"the model: {c['host']} and {c['device']} of {len(c['model']['list'].ws)} wrappers")
    assert len(counts) == 2, err[-2000:]   # one line per decode call
    assert counts[0] == counts[1] == (c["host"], c["device"]), (counts, c["host"], c["device"])


@pytest.mark.parametrize("name", NAMES)
def test_the_serial_kernel_on_the_same_files(ctx, name, monkeypatch, capfd):
    c = M.case(name)
    oi, of = oracle(name)
    monkeypatch.setenv("FLO_LL_DECODE_SERIAL", "1")
    monkeypatch.setenv("FLO_TRACE", "1")
    capfd.readouterr()
    di = ctx.decode_lossless_i32(c["flo"])
    df = ctx.decode(c["flo"])
    err = capfd.readouterr().err
    monkeypatch.delenv("FLO_TRACE")
    monkeypatch.delenv("FLO_LL_DECODE_SERIAL")
    same_bits(di, oi, "integers")
    same_bits(df, of, "floats")
    n = len(c["model"]["list"].ws)
    assert [(int(a), int(b)) for a, b in LINE.findall(err)] == [(n, 0), (n, 0)], err[-2000:]


OTHER_LISTS = [
    "route: k 14 / 15, sum of taps 2^21 - 1 / 2^21, shift 20 / 21 / 84 / 85",
    "scan k = 5: 72 tiles in a workgroup, one fewer, one more",
    "chain 257 tiles, k = 14, a run over the boundary",
    "ones: 130, 256, 300 bytes of 0xff at tile-aligned and unaligned offsets",
    "escape: runs of 255, 256 and 257 ones",
    "i32: a sample one above INT_MAX",
    "i32: a sample equal to INT_MAX",
    "run-on: a doubling wrapper of 20 samples beside two of 900",
    "rows: an idle row in front, an idle row behind, a group of none",
    "finish: stereo frames of 4 m + 0..3 samples in a row",
    "finish: mid/side pairs that wrap, odd and negative; samples above 2^24",
]


def test_the_other_lists_cover_every_group_and_every_handover():
    assert set(OTHER_LISTS) <= set(NAMES)
    assert {M.case(n)["group"] for n in OTHER_LISTS} == set(M.PATHS)
    paths = set().union(*(M.case(n)["paths"] for n in OTHER_LISTS))
    assert {"residual:esc_by_256_ones", "predict:rows_flag_by_sample", "predict:rows_flag_by_run-on_only", "route:serial_by_host"} <= paths


@pytest.mark.parametrize("name", OTHER_LISTS)
def test_corpus_stream_and_frame_lists(ctx, name):
    """The counts cannot be read on these paths: they do not go through ll_decode_device. Values only, against the oracle."""
    c = M.case(name)
    flo = c["flo"]
    _, of = oracle(name)
    ch = c["model"]["channels"]
    corpus = flo_amd.Corpus([flo], ctx)
    try:
        n = int(corpus.lengths[0])
        assert n * ch == of.size
        win = corpus.decode_windows(np.zeros(1, np.uint32), np.zeros(1, np.uint64), n).cpu().numpy().reshape(-1)
        corpus.sync()
    finally:
        corpus.close()
    same_bits(win, of, "corpus window")
    d = flo_amd.StreamingDecoder(ctx)
    try:
        d.feed(flo)
        r = flo_amd.decode_streams([d])
        assert int(r.status[0]) == 0, r.errors
        got = r.out.cpu().numpy().reshape(-1)
    finally:
        d.close()
    same_bits(got, of, "streaming decoder")
    for i, fr in enumerate(c["model"]["list"].frames):
        a, b = fr["out_off"] * ch, (fr["out_off"] + fr["samples"]) * ch
        same_bits(ctx.decode_frame_at(flo, i), of[a:b], "decode_frame_at %d" % i)
