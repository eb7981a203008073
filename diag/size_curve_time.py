"""The size curve (flo_batch_size_curve, K = 16 candidates i/16) against the route that gives the same answer without it:
sixteen encodes + syncs of the same batch, one per candidate quality (set_quality re-points the batch; without
set_quality that route is a batch created per quality, its fill left out of the timing). The two alternate in one
process after a warm-up; every timed region ends in a device synchronisation; five repeats, median and spread.
Shapes: 1250 x 10 s stereo (fill_synthetic) and one 3-minute stereo clip. Then what measuring costs a caller:
encode_to_bitrate_many against encode_with_bitrate_many on 256 x 10 s clips (wall time, host buffers in, files out).
usage: python diag/size_curve_time.py [--curve-only]     (--curve-only: warm-up and one curve per shape, for a kernel trace:
       rocprofv3 --kernel-trace --stats -- python diag/size_curve_time.py --curve-only)"""
import statistics
import sys
import time

sys.path.insert(0, ".")
import flo_amd  # noqa: E402

GRID = [i / 16 for i in range(16)]
REPEATS = 5
HBM = 8.0e12   # bytes per second, MI355X HBM3E peak
curve_only = "--curve-only" in sys.argv
sr, ch = 44100, 2
ctx = flo_amd.Context(0)


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def sixteen_encodes(b):
    for q in GRID:
        b.set_quality(q)
        b.encode(0)
        b.sync()


def shape(n, secs):
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [int(secs * sr) * ch] * n, sr, ch, 0.55)
    b.fill_synthetic(seed=0xF10A0D10, clip_id0=1)
    pcm_bytes = n * int(secs * sr) * ch * 4
    print(f"--- {n} x {secs:g} s stereo, {pcm_bytes / 1e9:.3f} GB of PCM")
    curve = b.size_curve(GRID)        # warm-up: tables of every candidate, pool blocks
    if curve_only:
        b.size_curve(GRID)
        b.close()
        return
    sixteen_encodes(b)
    # the curve is the encoder's own size at every candidate, on this shape too
    for j in (0, 7, 15):
        b.set_quality(GRID[j])
        b.encode(0)
        b.sync()
        assert b.data_bytes() + n * (74 + 20 * ((int(secs * sr) + 2047) // 1024)) == int(curve[:, j].sum()), j
    t_curve, t_enc = [], []
    for _ in range(REPEATS):
        t_curve.append(timed(lambda: b.size_curve(GRID)))
        t_enc.append(timed(lambda: sixteen_encodes(b)))
    mc, me = statistics.median(t_curve), statistics.median(t_enc)
    print(f"size curve, K = 16     : median {mc:9.3f} ms (min {min(t_curve):.3f}, max {max(t_curve):.3f})")
    print(f"sixteen encodes + syncs: median {me:9.3f} ms (min {min(t_enc):.3f}, max {max(t_enc):.3f}); one encode {me / 16:.3f} ms")
    print(f"curve / sixteen encodes: {mc / me:.3f}  (the curve costs {mc / (me / 16):.2f} encodes)")
    # kernel times from the profile hooks, in a pass of their own (the event brackets cost time)
    ctx.profile_enable(True)
    ctx.profile_reset()
    b.size_curve(GRID)
    parts = [(k, *ctx.profile_query(k)) for k in ("curve_bands", "curve_scan", "size_curve")]
    ctx.profile_enable(False)
    total = sum(p[1] for p in parts)
    print("kernels of one curve   : " + ", ".join(f"{k} {ms:.3f} ms in {cnt} launches" for k, ms, cnt in parts) + f"; sum {total:.3f} ms")
    floor = 2 * pcm_bytes / HBM * 1e3
    print(f"HBM floor (two reads of the PCM at {HBM / 1e12:.0f} TB/s): {floor:.3f} ms = {100 * floor / total:.1f} % of the kernel time")
    b.close()


shape(1250, 10.0)
shape(1, 180.0)

if not curve_only:
    n, secs = 256, 10.0
    src = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [int(secs * sr) * ch] * n, sr, ch, 0.55)
    src.fill_synthetic(seed=0xF10A0D10, clip_id0=1)
    clips = [src.download_pcm(i) for i in range(n)]
    src.close()
    print(f"--- what measuring costs a caller: {n} x {secs:g} s stereo clips from host buffers, 128 kbps")
    flo_amd.encode_with_bitrate_many(clips[:8], sr, ch, 16, 128)      # warm-up of both routes (default context)
    flo_amd.encode_to_bitrate_many(clips[:8], sr, ch, 128)
    t_map, t_meas = [], []
    for _ in range(3):
        t_map.append(timed(lambda: flo_amd.encode_with_bitrate_many(clips, sr, ch, 16, 128)))
        t_meas.append(timed(lambda: flo_amd.encode_to_bitrate_many(clips, sr, ch, 128)))
    files, infos = flo_amd.encode_to_bitrate_many(clips, sr, ch, 128, with_info=True)
    mapped = flo_amd.encode_with_bitrate_many(clips, sr, ch, 16, 128)
    target = infos[0]["target_bytes"]
    print(f"encode_with_bitrate_many: median {statistics.median(t_map):9.1f} ms; files {min(map(len, mapped))} .. {max(map(len, mapped))} bytes "
          f"for a target of {target}")
    print(f"encode_to_bitrate_many  : median {statistics.median(t_meas):9.1f} ms; files {min(map(len, files))} .. {max(map(len, files))} bytes, "
          f"{sum(i['fits'] for i in infos)} of {n} fit, {len(set(i['index'] for i in infos))} distinct qualities chosen")
ctx.close()
