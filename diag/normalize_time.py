"""Normalisation of a resident batch (flo_batch_normalize, flo_batch_true_peak): milliseconds per launch of each kernel -
1250 synthetic 10 s stereo clips at 44100 Hz by default - median of five after a warm-up, against the HBM floor (bytes read +
bytes written at the peak bench.py's roofline uses):
  norm_gain    GAIN mode: one read and one write of every sample
  norm_limit   LIMIT mode with every tile on the short path (a ceiling nothing reaches), and with no tile on it
               (FLO_NORM_NO_SKIP=1: the envelope of every frame, 256 FMAs per frame and channel, and the sliding stages)
  norm_peak    Batch.true_peaks: one read of every sample, the same envelope
The whole call (the batched analysis for the loudness, the true peaks, the kernel) is timed on the host beside them.
usage: python diag/normalize_time.py [n_clips] [seconds] [--channels N] [--rate HZ]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, ".")
import flo_amd  # noqa: E402

HBM_PEAK = 8.0e12   # bytes per second: bench.py's HBM_PEAK_GBS

ap = argparse.ArgumentParser()
ap.add_argument("n_clips", nargs="?", type=int, default=1250)
ap.add_argument("seconds", nargs="?", type=float, default=10.0)
ap.add_argument("--channels", type=int, default=2)
ap.add_argument("--rate", type=int, default=44100)
a = ap.parse_args()
n, secs, ch, rate = a.n_clips, a.seconds, a.channels, a.rate
frames = int(secs * rate)
samples = n * frames * ch

ctx = flo_amd.Context(0)
b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [frames * ch] * n, rate, ch, 0.55)
b.fill_synthetic(seed=0xF10A0D10, clip_id0=1)
b.sync()
A = flo_amd.normalize_lookahead(rate)
print(f"{n} clips of {secs:g} s, {ch} channels at {rate} Hz: {samples * 4 / 1e9:.2f} GB of PCM; look-ahead {A} frames")


def timed(kernel, call, moved):
    ms, wall = [], []
    ctx.profile_enable(True)
    for it in range(6):   # the first is the warm-up (pool allocations, the kernel's attribute)
        ctx.profile_reset()
        t0 = time.perf_counter()
        info = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        k, cnt = ctx.profile_query(kernel)
        assert cnt == 1, (kernel, cnt)
        if it:
            ms.append(k)
    ctx.profile_enable(False)
    med = statistics.median(ms)
    floor_ms = moved / HBM_PEAK * 1e3
    return med, ms, floor_ms, statistics.median(wall[1:]), info


def normalize(**kw):
    def call():
        out, reports = b.normalize(**kw)
        out.close()
        return sum(r["limited_frames"] for r in reports), min(r["gain_db"] for r in reports), max(r["gain_db"] for r in reports)
    return call


rows = [("GAIN mode", "norm_gain", normalize(target_lufs=-14.0), 2 * samples * 4, {}),
        ("LIMIT mode, every tile skipping", "norm_limit", normalize(target_lufs=-14.0, ceiling_dbtp=40.0, limit=True), 2 * samples * 4, {}),
        ("LIMIT mode, no tile skipping", "norm_limit", normalize(target_lufs=-14.0, limit=True), 2 * samples * 4, {"FLO_NORM_NO_SKIP": "1"}),
        ("LIMIT mode as it comes", "norm_limit", normalize(target_lufs=-14.0, limit=True), 2 * samples * 4, {}),
        ("true_peaks", "norm_peak", lambda: b.true_peaks().max(), samples * 4, {})]
for name, kernel, call, moved, env in rows:
    os.environ.update(env)
    try:
        med, ms, floor_ms, wall, info = timed(kernel, call, moved)
    finally:
        for k in env:
            os.environ.pop(k, None)
    print(f"{name}: {kernel} {med:.3f} ms (median of 5: {', '.join(f'{x:.3f}' for x in ms)}) | HBM floor {floor_ms:.3f} ms "
          f"({moved / 1e9:.2f} GB at {HBM_PEAK / 1e12:.0f} TB/s): fraction {floor_ms / med:.3f} | {samples / (med / 1e3) / 1e9:.1f} G samples/s | "
          f"the whole call {wall:.1f} ms on the host | {info}")
b.close()
ctx.close()
