"""The normalisation's entries in the registry of tests/recycled_scenarios.py (every export is covered by a scenario of
tests/test_gpu_recycled_memory.py or exempt with a reason: tests/test_recycled_memory_cpu.py), added to its lists
on import. The normalisation's test modules import this one, so a collection of tests/ holds the entries
before either of those tests reads the registry; the scenario goes in front of the last one, whose place the registry's
test fixes.

The scenario: what flo_batch_true_peak, flo_batch_normalize and flo_normalize return must not depend on what their pool
blocks held - the work list with the start values of the report words and of the peak words, and the new batch's PCM."""
import numpy as np

import flo_amd
import recycled_scenarios as S

S.EXEMPT.setdefault("flo_normalize_gain", "host arithmetic")
S.EXEMPT.setdefault("flo_normalize_lookahead", "host arithmetic")

NAME = "normalise and true peaks"


def normalise(ctx):
    clips = [S.noise(5000, 2, 81), S.noise(0, 2, 82), S.noise(2048, 2, 83, 0.3), S.noise(1, 2, 84), S.noise(6300, 2, 85, 0.05), np.zeros(600, np.float32)]
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [c.size for c in clips], S.SR, 2, 0.55)
    rec = []
    try:
        for i, x in enumerate(clips):
            b.upload(i, x)
        rec.append(("true peaks", np.ascontiguousarray(b.true_peaks(linear=True)).tobytes()))
        for limit in (False, True):
            out, reports = b.normalize(target_lufs=-3.0, limit=limit)
            try:
                rec += [("limit %d clip %d" % (limit, i), out.download_pcm(i).tobytes()) for i in range(out.n_clips)]
                rec.append(("limit %d reports" % limit, repr(reports).encode()))
            finally:
                out.close()
    finally:
        b.close()
    one, rep = ctx.normalize(clips[0], S.SR, 2, target_lufs=-3.0, limit=True, lookahead_ms=20.0)
    rec += [("flo_normalize", one.tobytes()), ("flo_normalize report", repr(rep).encode())]
    return rec


if NAME not in [s["name"] for s in S.SCENARIOS]:
    S.SCENARIOS.insert(len(S.SCENARIOS) - 1, dict(name=NAME, covers=["flo_batch_true_peak", "flo_batch_normalize", "flo_normalize"], run=normalise))
