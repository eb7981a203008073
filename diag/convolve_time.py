"""FIR filtering of a resident batch (flo_batch_convolve): milliseconds per launch of the convolve kernel, one mono response
for all clips, mode "head" - 1250 synthetic 10 s stereo clips at 48000 Hz by default - for K = 64, 512, 4096 and 32768 taps:
median of five after a warm-up with its range, from the profile bracket, the tap-outputs per second that makes, and for
K = 64 the fraction of the HBM floor (source frames read + output frames written at the peak bench.py's roofline uses).
A direct form costs K FMAs per output sample, so the long responses take the first n_clips * 512 / K clips of the batch
(at least 8: 1880 tiles, more than one per workgroup slot of the device) to keep a launch under a second; the rate per
tap-output is what the table is read for. diag/resample_time.py's 44100 -> 48000 row is the yardstick of DESIGN 4.18.
usage: python diag/convolve_time.py [n_clips] [seconds] [--rate HZ] [--taps K,K,...]"""
import argparse
import statistics
import sys

import numpy as np

sys.path.insert(0, ".")
import flo_amd  # noqa: E402

HBM_PEAK = 8.0e12   # bytes per second: bench.py's HBM_PEAK_GBS

ap = argparse.ArgumentParser()
ap.add_argument("n_clips", nargs="?", type=int, default=1250)
ap.add_argument("seconds", nargs="?", type=float, default=10.0)
ap.add_argument("--rate", type=int, default=48000)
ap.add_argument("--taps", default="64,512,4096,32768")
a = ap.parse_args()
n, secs, rate, ch = a.n_clips, a.seconds, a.rate, 2
frames = int(secs * rate)

ctx = flo_amd.Context(0)
b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [frames * ch] * n, rate, ch, 0.55)
b.fill_synthetic(seed=0xF10A0D10, clip_id0=1)
b.sync()
g = flo_amd.conv_geometry(ch, 1)
print(f"{n} clips of {secs:g} s, {ch} channels at {rate} Hz: {n * frames * ch * 4 / 1e9:.2f} GB of PCM; tiles of {g['tile_frames']} frames, "
      f"chunks of {g['tap_chunk']} taps, {g['lane_outputs']} outputs per lane")
rng = np.random.default_rng(1)
for K in [int(x) for x in a.taps.split(",")]:
    h = (rng.standard_normal(K) / np.sqrt(K)).astype(np.float32)
    irs = flo_amd.Batch(ctx, flo_amd.MODE_LOSSLESS, [K], rate, 1, 0)
    irs.upload(0, h)
    m = n if K <= 512 else max(min(n, 8), n * 512 // K)
    jobs = [dict(clip=i, ir=0) for i in range(m)]
    ms = []
    ctx.profile_enable(True)
    for it in range(6):   # the first is the warm-up (pool allocations)
        ctx.profile_reset()
        r = b.convolve(irs, jobs)
        r.sync()
        t, cnt = ctx.profile_query("convolve")
        assert cnt == 1, cnt
        r.close()
        if it:
            ms.append(t)
    ctx.profile_enable(False)
    irs.close()
    med = statistics.median(ms)
    tap_outputs = m * frames * ch * K
    line = (f"K {K}: {m} clips | {med:.3f} ms per launch (median of 5, range {min(ms):.3f} .. {max(ms):.3f}) | "
            f"{tap_outputs / (med / 1e3) / 1e12:.2f} T tap-outputs/s (range {tap_outputs / (max(ms) / 1e3) / 1e12:.2f} .. "
            f"{tap_outputs / (min(ms) / 1e3) / 1e12:.2f}), {m * frames * ch / (med / 1e3) / 1e9:.1f} G output samples/s")
    if K == 64:
        moved = 2 * m * frames * ch * 4
        line += f" | HBM floor {moved / HBM_PEAK * 1e3:.3f} ms ({moved / 1e9:.2f} GB at {HBM_PEAK / 1e12:.0f} TB/s): fraction {moved / HBM_PEAK * 1e3 / med:.3f}"
    print(line, flush=True)
b.close()
ctx.close()
