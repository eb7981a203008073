"""Sample-rate conversion of a resident batch (flo_batch_resample): milliseconds per launch - 1250 synthetic 10 s stereo
clips by default - at 48000 -> 44100, 44100 -> 48000 and 96000 -> 44100, median of five after a warm-up, against the HBM
floor (bytes read + bytes written at the peak bench.py's roofline uses), with the tap-outputs per second that makes.
For scale, the true-peak filter of the batch analysis (anb_peak_kernel: 4 x 49 taps per sample, analysis_batch_kernels.hip)
runs over the same source batch; it has no profile bracket of its own, so its time is read from a kernel trace:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o rs -- python diag/resample_time.py
    python diag/resample_time.py --peak-stats <dir>/.../rs_kernel_stats.csv
usage: python diag/resample_time.py [n_clips] [seconds] [--channels N] [--peak-stats CSV]"""
import argparse
import csv
import statistics
import sys

sys.path.insert(0, ".")
import flo_amd  # noqa: E402

HBM_PEAK = 8.0e12   # bytes per second: bench.py's HBM_PEAK_GBS

ap = argparse.ArgumentParser()
ap.add_argument("n_clips", nargs="?", type=int, default=1250)
ap.add_argument("seconds", nargs="?", type=float, default=10.0)
ap.add_argument("--channels", type=int, default=2)
ap.add_argument("--peak-stats", default=None, help="kernel stats CSV of a traced run: print anb_peak's rate and stop")
a = ap.parse_args()
n, secs, ch = a.n_clips, a.seconds, a.channels

if a.peak_stats:
    for row in csv.DictReader(open(a.peak_stats)):
        if "anb_peak_kernel(" in row.get("Name", ""):
            calls, avg_ns = int(row["Calls"]), float(row["AverageNs"])
            taps = n * int(secs * 44100) * ch * 4 * 49   # per launch over the 44100 Hz batch: 4 phases of 49 taps per sample
            print(f"anb_peak_kernel: {calls} launches, {avg_ns / 1e6:.3f} ms each: {taps / (avg_ns / 1e9) / 1e12:.2f} T tap-outputs/s "
                  f"({n} x {secs:g} s x {ch} ch at 44100 Hz)")
    sys.exit(0)

ctx = flo_amd.Context(0)
for in_rate, out_rate in ((48000, 44100), (44100, 48000), (96000, 44100)):
    info, _ = flo_amd.resample_filter(in_rate, out_rate)
    frames = int(secs * in_rate)
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [frames * ch] * n, in_rate, ch, 0.55)
    b.fill_synthetic(seed=0xF10A0D10, clip_id0=1)
    out_frames = flo_amd.resample_out_frames(in_rate, out_rate, frames)
    ms = []
    ctx.profile_enable(True)
    for it in range(6):   # the first is the warm-up (pool allocations, the kernel's attribute)
        ctx.profile_reset()
        r = b.resample(out_rate)
        r.sync()
        k, cnt = ctx.profile_query("resample")
        assert cnt == 1
        r.close()
        if it:
            ms.append(k)
    ctx.profile_enable(False)
    med = statistics.median(ms)
    moved = n * (frames + out_frames) * ch * 4
    floor_ms = moved / HBM_PEAK * 1e3
    tap_outputs = n * out_frames * ch * info["taps"]
    print(f"{in_rate} -> {out_rate}: L {info['L']} M {info['M']} taps {info['taps']} tile {info['tile_outputs']} | "
          f"{med:.3f} ms per launch (median of 5: {', '.join(f'{x:.3f}' for x in ms)}) | HBM floor {floor_ms:.3f} ms "
          f"({moved / 1e9:.2f} GB at {HBM_PEAK / 1e12:.0f} TB/s): fraction {floor_ms / med:.3f} | "
          f"{tap_outputs / (med / 1e3) / 1e12:.2f} T tap-outputs/s, {n * out_frames * ch / (med / 1e3) / 1e9:.1f} G output samples/s")
    if in_rate == 44100:   # the true-peak FIR over the same batch, for a kernel trace to time
        b.analyze_all()
    b.close()
ctx.close()
