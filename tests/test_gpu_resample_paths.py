"""Sample-rate conversion on the device, path by path (tests/resample_model.py names the paths and builds the cases;
tests/test_resample_model_cpu.py asserts that every path has one).

The kernel's header states its arithmetic exactly: every output is fma(h[p][k], x[i + k - T/2 + 1], acc) for k = 0 .. T - 1
in that order from acc = 0, whatever the batch, the tile or the kernel variant. resample_model.chain runs that chain in
f32 over the table flo_resample_filter returns (the FMA emulated with one rounding, checked against rational arithmetic
on the CPU), and every output of every clip - in its mixed batch through Batch.resample, and alone through flo_resample -
must equal it bit for bit: -0.0 is not +0.0, an infinity is that infinity, and where the chain gives NaN the device gives
NaN. No partial sum of any chain is subnormal (asserted on the CPU), so this holds whether or not the hardware flushes;
the one clip of denormals is held to the f64 bound alone. Every output is also held to the older bound against the f64 dot
product, |y - y_ref| <= (T + 1) 2^-24 sum |h x| + T 2^-126, wherever that reference is finite.

A failure names the rate pair, the channel count, the clip, the output frame and channel, the slot and phase of the lane
that made it, and the clip's paths."""
import numpy as np
import pytest

import flo_amd
import resample_model as M
from gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = M.cases()
_refs, _batches = {}, {}


def _reference(c):
    """per clip (chain, f64 dot product, bound), computed once per case and left unchanged"""
    if c["name"] not in _refs:
        _, table = flo_amd.resample_filter(c["in_rate"], c["out_rate"])
        out = []
        for _, x in c["clips"]:
            y, _ = M.chain(c["plan"], table, x, c["ch"])
            d, bound = M.dot_reference(c["plan"], table, x, c["ch"])
            for a in (y, d, bound):
                a.setflags(write=False)
            out.append((y, d, bound))
        _refs[c["name"]] = out
    return _refs[c["name"]]


def _batch(ctx, c):
    """the case's clips converted as one batch, once"""
    if c["name"] not in _batches:
        clips = [x for _, x in c["clips"]]
        b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSLESS, [x.size for x in clips], c["in_rate"], c["ch"], 5)
        try:
            for i, x in enumerate(clips):
                b.upload(i, x)
            r = b.resample(c["out_rate"])
            try:
                assert r.sample_rate == c["out_rate"] and r.channels == c["ch"] and r.n_clips == len(clips)
                _batches[c["name"]] = [r.download_pcm(i) for i in range(r.n_clips)]
            finally:
                r.close()
        finally:
            b.close()
    return _batches[c["name"]]


def _where(c, i, k):
    """the text of a failure at element k of clip i's output"""
    P, ch = c["plan"], c["ch"]
    name, x = c["clips"][i]
    j = k // ch
    lane = M.lane_of(P, j)
    own = sorted(M.clip_paths(P, x.size // ch) | M.value_paths(P, ch, x))
    return (f"{c['in_rate']} -> {c['out_rate']} x{ch} ({c['why']}), clip {i} '{name}' of {x.size // ch} frames, output frame {j} channel {k % ch}: "
            f"tile {lane['tile']} unit {lane['unit']} lane {lane['lane']} slot {lane['slot']} phase {lane['phase']} (block member "
            f"{lane['member']}, row {lane['row']}); the clip's paths: {', '.join(own)}; the launch's: "
            f"{', '.join(sorted(M.paths(c['in_rate'], c['out_rate'], ch, [v.size for _, v in c['clips']])))}")


def _hold(c, i, y, how):
    """clip i's device output y against both references; returns (outputs compared bit for bit, worst |y - ref| / bound)"""
    want, ref, bound = _reference(c)[i]
    name, x = c["clips"][i]
    assert y.dtype == np.float32 and y.size == want.size, (how, _where(c, i, 0), y.size, want.size)
    if not y.size:
        return 0, 0.0
    exact = 0
    if not M.is_denormal_clip(x):
        nan = np.isnan(want)
        bad = np.flatnonzero((np.isnan(y) != nan) | (~nan & (y.view(np.uint32) != want.view(np.uint32))))
        assert bad.size == 0, (f"{how}: {bad.size} of {y.size} outputs leave the chain, the first at {_where(c, i, int(bad[0]))}: device "
                               f"{y[bad[0]]!r} ({y.view(np.uint32)[bad[0]]:#010x}), chain {want[bad[0]]!r} ({want.view(np.uint32)[bad[0]]:#010x})")
        exact = y.size
    fin = np.isfinite(ref)
    assert np.isfinite(y[fin]).all(), (how, _where(c, i, int(np.flatnonzero(fin & ~np.isfinite(y))[0])))
    err = np.abs(y[fin].astype(np.float64) - ref[fin])
    over = np.flatnonzero(err > bound[fin])
    assert over.size == 0, (f"{how}: beyond the f64 bound at {_where(c, i, int(np.flatnonzero(fin)[over[0]]))}: "
                            f"{err[over[0]]:.3e} > {bound[fin][over[0]]:.3e}")
    return exact, float((err / bound[fin]).max()) if err.size else 0.0


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_a_mixed_batch_is_the_chain_bit_for_bit(ctx, c):
    outs = _batch(ctx, c)
    exact, worst = 0, 0.0
    for i in range(len(c["clips"])):
        e, w = _hold(c, i, outs[i], "Batch.resample")
        exact, worst = exact + e, max(worst, w)
    P = c["plan"]
    print(f"{c['name']}: Q {P['slots']}, {P['phases_per_wave']} phases per wave, taps {P['taps']}, tile {P['tile_outputs']}: "
          f"{exact} outputs bit for bit, worst |y - f64| / bound = {worst:.3f}")


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_every_clip_alone_is_the_chain_bit_for_bit(ctx, c):
    for i, (_, x) in enumerate(c["clips"]):
        _hold(c, i, ctx.resample(x, c["in_rate"], c["out_rate"], c["ch"]), "flo_resample")

