"""The quality ladder (flo_batch_encode_ladder) at K = 2, 4, 8 and 16 rungs against the route that gives the same files
without it: K x (set_quality + encode + sync) of the same resident batch. The two alternate in one process after a warm-up;
every timed region ends in a device synchronisation (the ladder is synchronous, its destruction is outside the timing);
five repeats, median (min .. max). Shapes: 1250 x 10 s stereo (fill_synthetic) and one 3-minute stereo clip. The per-kernel
split comes from the profile hooks, in a pass of its own (the event brackets cost time).
usage: python diag/ladder_time.py [--ladder-only] [--groups]
       --ladder-only: warm-up and one ladder of 8 rungs per shape, for a kernel trace
                      (rocprofv3 --kernel-trace --stats -- python diag/ladder_time.py --ladder-only)
       --groups:      the 16-rung ladder of the large shape at several FLO_LADDER_GROUP_BYTES"""
import os
import statistics
import sys
import time

sys.path.insert(0, ".")
import flo_amd  # noqa: E402

KS = [2, 4, 8, 16]
REPEATS = 5
KERNELS = ("ladder_bands", "ladder_scan", "lossy_ladder", "ladder_compact", "ladder_finish", "ladder_pack")
ladder_only = "--ladder-only" in sys.argv
groups = "--groups" in sys.argv
sr, ch = 44100, 2
ctx = flo_amd.Context(0)


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e3, r


def rungs(k):
    return [(i + 0.5) / k for i in range(k)]


def k_encodes(b, qs):
    for q in qs:
        b.set_quality(q)
        b.encode(0)
        b.sync()


def fmt(ts):
    return f"median {statistics.median(ts):9.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def shape(n, secs):
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [int(secs * sr) * ch] * n, sr, ch, 0.55)
    b.fill_synthetic(seed=0xF10A0D10, clip_id0=1)
    hops = (int(secs * sr) + 2047) // 1024
    print(f"--- {n} x {secs:g} s stereo, {n * hops} frames, {n * int(secs * sr) * ch * 4 / 1e9:.3f} GB of PCM")
    b.encode_ladder(rungs(16)).close()        # warm-up: tables of the rungs, pool blocks
    if ladder_only:
        b.encode_ladder(rungs(8)).close()
        b.close()
        return
    k_encodes(b, rungs(16))
    if groups:
        for mib in (256, 1024, 4096, 16384):
            os.environ["FLO_LADDER_GROUP_BYTES"] = str(mib << 20)
            ts = []
            for _ in range(REPEATS):
                t, lad = timed(lambda: b.encode_ladder(rungs(16)))
                lad.close()
                ts.append(t)
            print(f"K = 16, groups of {mib:5d} MiB: {fmt(ts)}")
        del os.environ["FLO_LADDER_GROUP_BYTES"]
        b.close()
        return
    for k in KS:
        qs = rungs(k)
        # the ladder is the encoder's own size at every rung, on this shape too
        with b.encode_ladder(qs) as lad:
            total = lad.file_bytes.sum(axis=0)
        for j in (0, k - 1):
            b.set_quality(qs[j])
            b.encode(0)
            b.sync()
            assert b.data_bytes() + n * (74 + 20 * hops) == int(total[j]), (k, j)
        t_lad, t_enc = [], []
        for _ in range(REPEATS):
            t, lad = timed(lambda: b.encode_ladder(qs))
            lad.close()
            t_lad.append(t)
            t_enc.append(timed(lambda: k_encodes(b, qs))[0])
        ml, me = statistics.median(t_lad), statistics.median(t_enc)
        print(f"K = {k:2d}: ladder {fmt(t_lad)} | {k} encodes + syncs {fmt(t_enc)} | ladder / encodes {ml / me:.3f}; "
              f"files {int(total.sum()) / 1e6:.1f} MB")
        ctx.profile_enable(True)
        ctx.profile_reset()
        b.encode_ladder(qs).close()
        parts = [(name, *ctx.profile_query(name)) for name in KERNELS]
        ctx.profile_enable(False)
        print("        kernels: " + ", ".join(f"{name} {ms:.3f} ms / {cnt}" for name, ms, cnt in parts) + f"; sum {sum(p[1] for p in parts):.3f} ms")
    b.close()


shape(1250, 10.0)
shape(1, 180.0)
ctx.close()
