"""Partitioned FFT convolution of a resident batch (flo_batch_convolve_fft) against the direct form (flo_batch_convolve):
milliseconds per call, one mono response for all clips, mode "head" - 1250 synthetic 10 s stereo clips at 48000 Hz by default -
for K = 64 .. 65536 by powers of four, and 262144. Per K: the FFT path on the whole batch, median of five calls after a warm-up
with its range, per profile name (fftconv_ir, fftconv_fwd, fftconv_mac: the sums over a call's groups) and in all; the direct
path in the same session at the K it supports, on the clip subset diag/convolve_time.py uses (n_clips * 512 / K, at least 8),
scaled to the whole batch by clips; and the ratio. The smallest K from which the FFT path is no slower is crossover_taps
(DESIGN 4.19).
--no-direct times the FFT path alone (comparing builds of another block_frames or lane_blocks through FLO_HIP_LIB).
usage: python diag/fftconv_time.py [n_clips] [seconds] [--rate HZ] [--taps K,K,...] [--no-direct]"""
import argparse
import statistics
import sys

import numpy as np

sys.path.insert(0, ".")
import flo_amd  # noqa: E402

NAMES = ("fftconv_ir", "fftconv_fwd", "fftconv_mac")

ap = argparse.ArgumentParser()
ap.add_argument("n_clips", nargs="?", type=int, default=1250)
ap.add_argument("seconds", nargs="?", type=float, default=10.0)
ap.add_argument("--rate", type=int, default=48000)
ap.add_argument("--taps", default="64,256,1024,4096,16384,65536,262144")
ap.add_argument("--no-direct", action="store_true")
a = ap.parse_args()
n, secs, rate, ch = a.n_clips, a.seconds, a.rate, 2
frames = int(secs * rate)

ctx = flo_amd.Context(0)
b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [frames * ch] * n, rate, ch, 0.55)
b.fill_synthetic(seed=0xF10A0D10, clip_id0=1)
b.sync()
g = flo_amd.conv_fft_geometry(ch, 1)
print(f"{n} clips of {secs:g} s, {ch} channels at {rate} Hz: {n * frames * ch * 4 / 1e9:.2f} GB of PCM; blocks of {g['block_frames']} frames, "
      f"{g['lane_blocks']} blocks per lane, crossover_taps {g['crossover_taps']}")


def med(v):
    return f"{statistics.median(v):.3f} ms ({min(v):.3f} .. {max(v):.3f})"


rng = np.random.default_rng(1)
for K in [int(x) for x in a.taps.split(",")]:
    h = (rng.standard_normal(K) / np.sqrt(K)).astype(np.float32)
    irs = flo_amd.Batch(ctx, flo_amd.MODE_LOSSLESS, [K], rate, 1, 0)
    irs.upload(0, h)
    jobs = [dict(clip=i, ir=0) for i in range(n)]
    per = {name: [] for name in NAMES}
    total = []
    ctx.profile_enable(True)
    for it in range(6):   # the first is the warm-up (pool allocations)
        ctx.profile_reset()
        r = b.convolve(irs, jobs, method="fft")
        r.sync()
        t = {name: ctx.profile_query(name)[0] for name in NAMES}
        r.close()
        if it:
            for name in NAMES:
                per[name].append(t[name])
            total.append(sum(t.values()))
    line = f"K {K}: fft {med(total)} | " + ", ".join(f"{name[8:]} {med(per[name])}" for name in NAMES)
    if K <= 65536 and not a.no_direct:
        m = n if K <= 512 else max(min(n, 8), n * 512 // K)
        ms = []
        for it in range(6):
            ctx.profile_reset()
            r = b.convolve(irs, jobs[:m])
            r.sync()
            ms.append(ctx.profile_query("convolve")[0])
            r.close()
        ms = [x * n / m for x in ms[1:]]
        line += f" | direct ({m} clips, scaled) {med(ms)} | direct / fft {statistics.median(ms) / statistics.median(total):.2f}"
    ctx.profile_enable(False)
    irs.close()
    print(line, flush=True)
b.close()
ctx.close()
