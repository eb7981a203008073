"""Every compare, tail and totals path of the fidelity reports on the device, by the named cases of fidelity_cases.py:
flo_compare against a lossless file (fid_compare_kernel), a lossy file and a ready transform file (the fused
lossy_decode_kernel<kDecCompare>), and flo_batch_fidelity fused, unfused and lossless, all through fid_totals_kernel. The
expected report is the NumPy model's (fidelity_ref.py) of the source and the device's own decode (anchored to f64 by
test_gpu_tdecode.py): every sum, peak, count and block record bit for bit, the two logarithms within 1e-9 dB
(M.assert_matches). Each case's predicates are asserted on the expected report first, so that the case reaches what it
is there for; each report is asked for twice and must come back with the same bytes."""
import numpy as np
import pytest

import fidelity_cases as C
import fidelity_ref as M
from gpu_util import ctx  # noqa: F401
from test_gpu_fidelity import _batch, _decoded, _raw

import flo_amd

pytestmark = pytest.mark.gpu

QUALITY, LEVEL = 0.55, 5
_FILES = {}


def _file_and_decode(ctx, p, form):
    """the case's file in this form and the device's decode of it, made once per (file_key, form)"""
    key = (p.file_key, form, p.bits)
    if key not in _FILES:
        f = p.file()
        if form == "lossy":
            f = ctx.encode_lossy(f, C.SR, p.ch, QUALITY)
        elif form == "lossless":
            f = ctx.encode_lossless(f, C.SR, p.ch, p.bits, LEVEL)
        dec = ctx.decode(f)
        dec.setflags(write=False)
        _FILES[key] = (bytes(f), dec)
    return _FILES[key]


@pytest.mark.parametrize("name, form", C.PAIR_IDS, ids=[f"{n}-{f}" for n, f in C.PAIR_IDS])
def test_compare_follows_the_model(ctx, name, form):
    p = C.PAIRS[name]
    f, dec = _file_and_decode(ctx, p, form)
    src = p.source(dec)
    want, wb = M.fidelity(src, dec, p.ch)
    for tag in p.there_for:
        assert C.PREDICATES[tag](want, wb), (name, form, tag, "the case does not reach what it is there for")
    got = ctx.compare(src, f, blocks=True)
    print(name, form, {k: got[k] for k in ("snr_db", "seg_snr_db", "seg_blocks", "peak_error", "peak_out", "clipped")})
    M.assert_matches(got, want, wb, tag=(name, form))
    assert got["blocks"].shape == (want["n_blocks"], p.ch)
    assert _raw([ctx.compare(src, f, blocks=True)]) == _raw([got])            # two calls: identical bits
    without = ctx.compare(src, f)
    assert "blocks" not in without and _raw([dict(without, blocks=np.zeros(0))]) == _raw([dict(got, blocks=np.zeros(0))])


def test_compare_with_an_empty_source_returns_no_blocks(ctx):
    p = C.PAIRS["short_source_0"]
    for form in p.forms:
        f, dec = _file_and_decode(ctx, p, form)
        for src in (np.zeros(0, np.float32), np.zeros(p.ch - 1, np.float32)):      # nothing, and less than one frame
            r = ctx.compare(src, f, blocks=True)
            assert r["n_blocks"] == 0 and r["blocks"].shape == (0, p.ch) and r["blocks"].dtype == flo_amd.FIDELITY_BLOCK_DTYPE
            assert r["source_frames"] == 0 and r["compared_frames"] == 0 and r["decoded_frames"] == dec.size // p.ch
            assert np.all(r["snr_db"] == np.inf) and np.all(np.isnan(r["seg_snr_db"])) and np.all(r["seg_blocks"] == 0)
            want, _ = M.fidelity(src, dec, p.ch)
            assert np.all(r["tail_energy"] == want["tail_energy"]) and np.all(r["tail_energy"] > 0.0)
        import ctypes
        out, nb = np.zeros(p.ch, flo_amd.FIDELITY_DTYPE), ctypes.c_size_t(7)          # the C entry takes a null source of no samples
        assert ctx._L.flo_compare(ctx._h, None, 0, f, len(f), out.ctypes.data, None, 0, ctypes.byref(nb)) == 0 and nb.value == 0
        assert _raw([dict(flo_amd.fidelity_dict(out), blocks=np.zeros(0))]) == _raw([dict(ctx.compare(np.zeros(0, np.float32), f), blocks=np.zeros(0))])


def _check(b, tag):
    """a batch's reports against the model of each clip's source and decode; block_off against the model's n_blocks"""
    rep = b.fidelity(blocks=True)
    dec = _decoded(b, rep)
    wants = []
    for i in range(b.n_clips):
        want, wb = M.fidelity(b.download_pcm(i), dec[i], b.channels)
        M.assert_matches(rep[i], want, wb, tag=(tag, i))
        wants.append(want)
    off = np.zeros(b.n_clips + 1, np.uint64)
    assert b._L.flo_batch_fidelity(b._h, None, None, 0, off.ctypes.data) == 0                 # the sizing call
    assert list(off) == list(np.concatenate([[0], np.cumsum([w["n_blocks"] for w in wants])])), tag
    assert _raw(b.fidelity(blocks=True)) == _raw(rep), tag                                     # two calls: identical bits
    return rep, wants


@pytest.mark.parametrize("name", list(C.BATCHES))
def test_batch_follows_the_model_fused_unfused_and_lossless(ctx, name, monkeypatch):
    bc = C.BATCHES[name]
    clips = bc.clips()
    b = _batch(ctx, flo_amd.MODE_LOSSY, clips, bc.ch, QUALITY)
    try:
        fused, wants = _check(b, (name, "fused"))
        for tag in bc.there_for:
            assert C.BATCH_PREDICATES[tag](wants, bc.ch), (name, tag, "the case does not reach what it is there for")
        monkeypatch.setenv("FLO_FIDELITY_UNFUSED", "1")
        unfused, _ = _check(b, (name, "unfused"))
        monkeypatch.delenv("FLO_FIDELITY_UNFUSED")
        assert _raw(unfused) == _raw(fused)
    finally:
        b.close()
    b = _batch(ctx, flo_amd.MODE_LOSSLESS, clips, bc.ch, LEVEL)
    try:
        _, wants = _check(b, (name, "lossless"))
        for tag in bc.there_for:
            assert C.BATCH_PREDICATES[tag](wants, bc.ch), (name, tag, "lossless")
        assert all(w["decoded_frames"] == w["source_frames"] == c.size // bc.ch for w, c in zip(wants, clips))
    finally:
        b.close()


@pytest.mark.parametrize("mode", [flo_amd.MODE_LOSSY, flo_amd.MODE_LOSSLESS], ids=["lossy", "lossless"])
def test_a_nonfinite_clip_leaves_its_neighbours_reports_alone(ctx, mode, monkeypatch):
    """the neighbours of the clip with NaN and inf: the bytes they give in a batch without that clip"""
    clips = C.nonfinite_batch_clips()
    q = QUALITY if mode == flo_amd.MODE_LOSSY else LEVEL
    forms = ("0", "1") if mode == flo_amd.MODE_LOSSY else ("0",)
    for unfused in forms:
        monkeypatch.setenv("FLO_FIDELITY_UNFUSED", unfused)
        with_bad, without = _batch(ctx, mode, clips, 2, q), _batch(ctx, mode, [clips[0], clips[2]], 2, q)
        try:
            a, b = with_bad.fidelity(blocks=True), without.fidelity(blocks=True)
            assert not np.all(np.isfinite(a[1]["signal"]))
            assert np.all(np.isfinite(b[0]["snr_db"])) and np.all(np.isfinite(b[1]["seg_snr_db"]))
            assert _raw([a[0], a[2]]) == _raw(b), unfused
        finally:
            with_bad.close()
            without.close()
