"""The analysis metadata on every path of its scans, segments, tiles and chains (tests/analysis_model.py names them and
holds the cases; tests/test_analysis_model_cpu.py shows that the cases reach them): flo_analyze and
flo_analysis_metadata clip by clip, flo_batch_analyze_all and flo_batch_analysis_metadata_all with one batch per
(rate, channels) - the batched K-weighting passes, peak FIR and block energies are code of their own - once in one
group and once under a small FLO_BATCH_ANALYSIS_GROUP_BYTES.

Against the oracle: waveform peaks, hash, fingerprint bytes, the f32 sum of squares, true peak and sample peak bit for
bit at any length; the META chunk byte for byte; integrated loudness and range bit for bit within one exact segment and
within the bound of analysis_model.expected beyond (measured against the oracle's long-double twin; a non-finite oracle
value must be met in kind)."""
import re

import numpy as np
import pytest

import analysis_model as M
import flo_amd
from gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

FIELDS = ("hash", "duration_ms", "sample_rate", "channels", "frequency_peaks", "energy_profile", "avg_loudness",
          "integrated_lufs", "length_ms", "loudness_range_lu", "true_peak_dbtp", "sample_peak_dbfs", "sum_squares")


def _bits(v):
    if isinstance(v, (float, np.floating)):
        return np.array(v, np.float64 if isinstance(v, float) else type(v)).tobytes()
    return v


def _same(a, b, who):
    assert a["peaks"].size == b["peaks"].size and np.array_equal(a["peaks"].view(np.uint32), b["peaks"].view(np.uint32)), who
    for k in FIELDS:
        assert _bits(a[k]) == _bits(b[k]) or (isinstance(a[k], float) and np.isnan(a[k]) and np.isnan(b[k])), (who, k, a[k], b[k])


@pytest.mark.parametrize("name", [c["name"] for c in M.cases()])
def test_one_clip(ctx, name):
    c = M.case(name)
    x = c["make"]()
    a = ctx.analyze(x, c["sr"], c["ch"], c["pps"])
    M.check_analysis(a, ctx.analysis_metadata(x, c["sr"], c["ch"], c["pps"]), c)


def _groups():
    g = {}
    for c in M.cases():
        g.setdefault((c["sr"], c["ch"], c["pps"]), []).append(c)
    return g


@pytest.mark.parametrize("key", sorted(_groups()), ids=lambda k: "%d Hz %d ch %d peaks" % k)
def test_batch(ctx, key, monkeypatch):
    sr, ch, pps = key
    cs = _groups()[key]
    clips = [c["make"]() for c in cs]
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSLESS, [x.size for x in clips], sr, ch, 5)
    try:
        for i, x in enumerate(clips):
            b.upload(i, x)
        got, metas = b.analyze_all(pps), b.analysis_metadata_all(pps)
        assert len(got) == len(metas) == len(cs)
        for i, c in enumerate(cs):
            M.check_analysis(got[i], metas[i], c, " (batch)")
        # the same in groups: every large clip alone, the small ones a few at a time
        monkeypatch.setenv("FLO_BATCH_ANALYSIS_GROUP_BYTES", str(1 << 18))
        again, metas2 = b.analyze_all(pps), b.analysis_metadata_all(pps)
        for i, c in enumerate(cs):
            _same(again[i], got[i], (c["name"], "groups"))
            assert metas2[i] == metas[i], (c["name"], "groups")
    finally:
        b.close()


@pytest.mark.parametrize("name", [c["name"] for c in M.cases() if c["family"] == "sumsq"])
def test_the_sum_of_squares_walks_only_what_it_must(ctx, name, monkeypatch, capfd):
    """The walk-every-chunk fallback gives the right sum too: the chain's one-addition and 64-at-once paths are shown to
    have produced it by the number of chunks it reports as walked (FLO_TRACE), which must be the model's must-walk count."""
    c = M.case(name)
    x = c["make"]()
    want = M.sumsq_chain(x)
    monkeypatch.setenv("FLO_TRACE", "1")
    capfd.readouterr()
    a = ctx.analyze(x, c["sr"], c["ch"], c["pps"])
    err = capfd.readouterr().err
    monkeypatch.delenv("FLO_TRACE")
    m = re.search(r"\[analysis\] sum of squares: (\d+) chunks, (\d+) walked sample by sample", err)
    assert m, err[-2000:]
    print(f"{name}: {m.group(1)} chunks, {m.group(2)} walked; the model: {want['chunks']} chunks, {len(want['must_walk'])} must be walked")
    assert np.float32(a["sum_squares"]).view(np.uint32) == want["result"].view(np.uint32)
    assert int(m.group(1)) == want["chunks"]
    assert int(m.group(2)) == len(want["must_walk"]), (m.group(2), sorted(want["must_walk"].items()))
