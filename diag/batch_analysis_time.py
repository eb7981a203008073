"""The analysis metadata of a whole batch: the per-clip loop (flo_batch_analysis_metadata, one clip per call) against the
batched call (flo_batch_analysis_metadata_all / flo_batch_analyze_all) over the same batch - 1250 synthetic 10 s stereo
clips by default - with the kernel time from the profile hooks and the bytes read against the HBM roofline.
usage: python diag/batch_analysis_time.py [n_clips] [seconds]"""
import sys
import time

sys.path.insert(0, ".")
import flo_amd  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1250
secs = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
sr, ch = 44100, 2
ctx = flo_amd.Context(0)
b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [int(secs * sr) * ch] * n, sr, ch, 0.55)
b.fill_synthetic(seed=0xF10A0D10, clip_id0=1)
pcm_bytes = n * int(secs * sr) * ch * 4

# the per-clip loop (each call ends in a blocking read-back)
b.analysis_metadata(0)
ctx.profile_enable(True)
ctx.profile_reset()
t = time.perf_counter()
loop = [b.analysis_metadata(i) for i in range(n)]
d_loop = time.perf_counter() - t
k_loop, cnt_loop = ctx.profile_query("analysis")

# the batched call, warmed up once (pool allocations), then timed
b.analysis_metadata_all()
ctx.profile_reset()
t = time.perf_counter()
metas = b.analysis_metadata_all()
d_all = time.perf_counter() - t
k_all, cnt_all = ctx.profile_query("analysis_batch")
ctx.profile_enable(False)
t = time.perf_counter()
b.analyze_all()
d_an = time.perf_counter() - t
assert metas == loop, "batched META differs from the per-clip META"

# PCM passes of the batched kernels on clips beyond one segment: waveform peaks, K-weighting passes 1 and 2, the
# true-peak tiles, the chunk sums and the terms of the sum of squares, the BLAKE3 chunks (the FFT reads 3 x 256 frames)
passes = 7
hbm = 8.0e12   # bytes per second, MI355X HBM3E peak
print(f"{n} x {secs:g} s stereo clips, {pcm_bytes / 1e9:.2f} GB of PCM")
print(f"per-clip loop       : {d_loop * 1e3:9.1f} ms wall, {k_loop:8.2f} ms in {cnt_loop} event-timed launches, "
      f"{d_loop / n * 1e3:.3f} ms per clip")
print(f"analysis_metadata_all: {d_all * 1e3:9.2f} ms wall, {k_all:8.2f} ms in {cnt_all} event-timed launch groups")
print(f"analyze_all          : {d_an * 1e3:9.2f} ms wall")
print(f"speed-up (wall)      : {d_loop / d_all:9.1f} x")
print(f"bytes read           : ~{passes} passes x {pcm_bytes / 1e9:.2f} GB = {passes * pcm_bytes / 1e9:.1f} GB; "
      f"at {hbm / 1e12:.0f} TB/s that is {passes * pcm_bytes / hbm * 1e3:.2f} ms; kernels took {k_all:.2f} ms "
      f"({passes * pcm_bytes / (k_all / 1e3) / 1e12:.2f} TB/s effective)")
b.close()
ctx.close()
