"""Mixing and concatenation of a resident batch (flo_batch_mix): milliseconds per launch of the mix kernel - 1250 synthetic
10 s stereo clips at 48000 Hz by default - median of five after a warm-up with its range, from the profile bracket, against the
HBM floor (source frames read + output frames written at the peak bench.py's roofline uses):
  yardstick    Batch.edit of every clip whole, copy form (edit_copy): one read and one write of every sample
  (a) concat   n / 2 outputs, each two clips end to end: the yardstick's bytes
  (b) overlay  n outputs, each 0.5 * clip i + 0.5 * clip (i + 1) % n: two reads and one write of every sample
  (c) xfade    (a) with a 10 ms crossfade
  (d) host     what Batch.mix costs on the host before it returns (the parts built in Python, the checks, the work list, the
               enqueue), beside the whole call with its wait
usage: python diag/mix_time.py [n_clips] [seconds] [--rate HZ]"""
import argparse
import statistics
import sys
import time

sys.path.insert(0, ".")
import flo_amd  # noqa: E402

HBM_PEAK = 8.0e12   # bytes per second: bench.py's HBM_PEAK_GBS

ap = argparse.ArgumentParser()
ap.add_argument("n_clips", nargs="?", type=int, default=1250)
ap.add_argument("seconds", nargs="?", type=float, default=10.0)
ap.add_argument("--rate", type=int, default=48000)
a = ap.parse_args()
n, secs, rate, ch = a.n_clips // 2 * 2, a.seconds, a.rate, 2
frames = int(secs * rate)

ctx = flo_amd.Context(0)
b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [frames * ch] * n, rate, ch, 0.55)
b.fill_synthetic(seed=0xF10A0D10, clip_id0=1)
b.sync()
print(f"{n} clips of {secs:g} s, {ch} channels at {rate} Hz: {n * frames * ch * 4 / 1e9:.2f} GB of PCM; tiles of {flo_amd.edit_tile_frames(ch, ch)} frames")


def timed(kernel, call):
    """[ms of five launches], the host's median milliseconds until the call returned, and for the whole call with its wait"""
    ms, host, wall = [], [], []
    ctx.profile_enable(True)
    for it in range(6):   # the first is the warm-up (pool allocations)
        ctx.profile_reset()
        t0 = time.perf_counter()
        r = call()
        t1 = time.perf_counter()
        r.sync()
        wall.append((time.perf_counter() - t0) * 1e3)
        host.append((t1 - t0) * 1e3)
        r.close()
        t, cnt = ctx.profile_query(kernel)
        assert cnt == 1, (kernel, cnt)
        if it:
            ms.append(t)
    ctx.profile_enable(False)
    return ms, statistics.median(host[1:]), statistics.median(wall[1:])


def report(name, kernel, call, moved):
    ms, host, wall = timed(kernel, call)
    med, floor_ms = statistics.median(ms), moved / HBM_PEAK * 1e3
    print(f"{name}: {kernel} {med:.3f} ms (median of 5, range {min(ms):.3f} .. {max(ms):.3f}) | HBM floor {floor_ms:.3f} ms "
          f"({moved / 1e9:.2f} GB at {HBM_PEAK / 1e12:.0f} TB/s): fraction {floor_ms / med:.3f} | host {host:.1f} ms until the call returned, "
          f"{wall:.1f} ms with the wait")
    return med, max(ms) - min(ms)


fb = frames * ch * 4 * n   # bytes of every sample once
whole = [dict(clip=i) for i in range(n)]
y = report("yardstick, whole-clip copy", "edit_copy", lambda: b.edit(whole), 2 * fb)

groups = [[2 * k, 2 * k + 1] for k in range(n // 2)]
c = report("(a) two clips end to end", "mix", lambda: b.concat(groups), 2 * fb)
print(f"  against the yardstick: {c[0]:.3f} ms, the bound {y[0]:.3f} + {y[1]:.3f} + {c[1]:.3f} = {y[0] + y[1] + c[1]:.3f} ms: "
      f"{'within' if c[0] <= y[0] + y[1] + c[1] else 'ABOVE'}")
overlay = [dict(out=i, clip=j, gain=0.5) for i in range(n) for j in (i, (i + 1) % n)]
report("(b) 0.5 * clip i + 0.5 * clip i + 1", "mix", lambda: b.mix(overlay, [frames] * n), 3 * fb)
report("(c) two clips end to end, 10 ms crossfade", "mix", lambda: b.concat(groups, crossfade_ms=10.0), 2 * fb)
print("(d) the host column of (a) .. (c) is Batch.mix's cost before it returns; (b) builds 2 parts per output in Python")
b.close()
ctx.close()
