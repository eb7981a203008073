"""Editing of a resident batch (flo_batch_edit, flo_batch_active_range): milliseconds per launch of each kernel - 1250
synthetic 10 s stereo clips at 48000 Hz by default - median of five after a warm-up with its range, against the HBM floor
(source frames read + output frames written at the peak bench.py's roofline uses):
  yardstick    GAIN-mode Batch.normalize (norm_gain): the parent's kernel of the same kind, one read and one write of every sample
  whole copy   Batch.edit of every clip whole, copy form: the same bytes as the yardstick, less arithmetic
  (a) crop     copy form, the middle 8 s from an odd start (the source two floats past a 16-byte boundary), and from the
               even start in front of it (the source on a 16-byte boundary) to compare
  (b) to_mono  2 -> 1
  swap         the generic form on a 2 x 2 matrix that swaps the channels: frame by frame, 4 bytes per lane and access
  (c) trim     Batch.trim_silence with 10 ms fades on clips with 0.5 s of silence at either end: edit_active, then edit_copy
  (d) ranges   Batch.active_ranges alone
With --classes a mono batch of the same bytes is cropped from starts 0 .. 3, so every alignment class of the source is timed:
class 0 is what aligned 16-byte loads cost, classes 1 .. 3 what the same loads cost at a 4-byte aligned address.
usage: python diag/edit_time.py [n_clips] [seconds] [--rate HZ] [--classes]"""
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
ap.add_argument("--classes", action="store_true")
a = ap.parse_args()
n, secs, rate, ch = a.n_clips, a.seconds, a.rate, 2
frames = int(secs * rate)

ctx = flo_amd.Context(0)
b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [frames * ch] * n, rate, ch, 0.55)
b.fill_synthetic(seed=0xF10A0D10, clip_id0=1)
b.sync()
print(f"{n} clips of {secs:g} s, {ch} channels at {rate} Hz: {n * frames * ch * 4 / 1e9:.2f} GB of PCM; "
      f"tiles of {flo_amd.edit_tile_frames(2, 2)} (2 -> 2) and {flo_amd.edit_tile_frames(2, 1)} (2 -> 1) frames")


def timed(kernels, call):
    """{kernel: [ms of five launches]}, the host's median milliseconds for the whole call"""
    ms, wall = {k: [] for k in kernels}, []
    ctx.profile_enable(True)
    for it in range(6):   # the first is the warm-up (pool allocations)
        ctx.profile_reset()
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        for k in kernels:
            t, cnt = ctx.profile_query(k)
            assert cnt == 1, (k, cnt)
            if it:
                ms[k].append(t)
    ctx.profile_enable(False)
    return ms, statistics.median(wall[1:])


def report(name, kernels, call, moved):
    ms, wall = timed(kernels, call)
    out = {}
    for k in kernels:
        med, floor_ms = statistics.median(ms[k]), moved[k] / HBM_PEAK * 1e3
        out[k] = (med, max(ms[k]) - min(ms[k]))
        print(f"{name}: {k} {med:.3f} ms (median of 5, range {min(ms[k]):.3f} .. {max(ms[k]):.3f}) | HBM floor {floor_ms:.3f} ms "
              f"({moved[k] / 1e9:.2f} GB at {HBM_PEAK / 1e12:.0f} TB/s): fraction {floor_ms / med:.3f} | the whole call {wall:.1f} ms on the host")
    return out


def closing(make):
    def call():
        r = make()
        r = r[0] if isinstance(r, tuple) else r
        r.sync()
        r.close()
    return call


whole = [dict(clip=i) for i in range(n)]
start = (frames // 10) | 1
crop = [dict(clip=i, start=start, frames=frames * 8 // 10) for i in range(n)]
fb = frames * ch * 4 * n   # bytes of every sample once

y = report("yardstick, GAIN-mode normalize", ["norm_gain"], closing(lambda: b.normalize(target_lufs=-14.0)), {"norm_gain": 2 * fb})["norm_gain"]
w = report("whole-clip copy", ["edit_copy"], closing(lambda: b.edit(whole)), {"edit_copy": 2 * fb})["edit_copy"]
print(f"  against the yardstick: {w[0]:.3f} ms, the bound {y[0]:.3f} + {y[1]:.3f} + {w[1]:.3f} = {y[0] + y[1] + w[1]:.3f} ms: "
      f"{'within' if w[0] <= y[0] + y[1] + w[1] else 'ABOVE'}")
report(f"(a) crop of 8 s from frame {start} (class 2)", ["edit_copy"], closing(lambda: b.edit(crop)), {"edit_copy": 2 * fb * 8 // 10})
even = [dict(g, start=start - 1) for g in crop]
report(f"(a) the same crop from frame {start - 1} (class 0)", ["edit_copy"], closing(lambda: b.edit(even)), {"edit_copy": 2 * fb * 8 // 10})
report("(b) to_mono", ["edit_2to1"], closing(lambda: b.to_mono()), {"edit_2to1": fb + fb // 2})
report("swap, the generic form", ["edit_mix"], closing(lambda: b.remix([[0, 1], [1, 0]])), {"edit_mix": 2 * fb})

half = rate // 2
quiet = b.edit([dict(clip=i, start=half, frames=frames - 2 * half, pad_head=half, pad_tail=half) for i in range(n)])
quiet.sync()
ranges = quiet.active_ranges()
kept = int((ranges[:, 1] - ranges[:, 0]).sum())
print(f"clips with {half} silent frames at either end: active ranges {ranges[:, 0].min()} .. {ranges[:, 1].max()}, {kept / n:.0f} frames kept per clip")
report("(c) trim_silence, 10 ms fades", ["edit_active", "edit_copy"], closing(lambda: quiet.trim_silence(fade_ms=10.0)),
       {"edit_active": fb, "edit_copy": 2 * kept * ch * 4})
report("(d) active_ranges", ["edit_active"], lambda: quiet.active_ranges(), {"edit_active": fb})
quiet.close()
b.close()

if a.classes:
    m = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [frames * ch] * n, rate, 1, 0.55)   # the same bytes as one channel
    m.fill_synthetic(seed=0xF10A0D10, clip_id0=1)
    m.sync()
    for s in range(4):
        segs = [dict(clip=i, start=s, frames=frames * ch - 8) for i in range(n)]
        report(f"mono crop from frame {s} (class {s})", ["edit_copy"], closing(lambda: m.edit(segs)), {"edit_copy": 2 * (fb - 32 * n)})
    m.close()
ctx.close()
