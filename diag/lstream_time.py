"""Lossy streaming encode rate (flo_stream_encode_ready): N stereo 48 kHz streams (quality 0.55) each receive one tick of
new samples, then ONE encode_streams call encodes every complete frame of all of them; against the same ticks through N
push_samples calls (one stream step per stream). Reports per tick the wall time of both, the kernel time and the
upload bytes of the batched call, and frames per second (1024 sample-frames per frame). The samples come from host
memory, so large ticks are bound by the upload: the share is in the rocprofv3 trace (--memory-copy-trace).
usage: python diag/lstream_time.py [out.json] [N ...]   (default N: 1 64 1024; ticks 20 ms, 100 ms, 1 s)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flo_amd  # noqa: E402

SR, CH, Q = 48000, 2, 0.55
KERNELS = ["lstream_bands", "lstream_scan", "lstream_frames", "lstream_compact"]
TICKS_MS = (20, 100, 1000)


def pool(n_sf, k=8):
    """k distinct signals of n_sf sample-frames: tones and noise at speech / music levels"""
    rng = np.random.default_rng(7)
    t = np.arange(n_sf, dtype=np.float64) / SR
    out = []
    for i in range(k):
        f = 110.0 * (i + 1)
        s = 0.3 * np.sin(2 * np.pi * f * t) + 0.05 * rng.standard_normal(n_sf)
        out.append(np.repeat(s[:, None], CH, axis=1).astype(np.float32).reshape(-1))
    return out


def run(ctx, n, tick_ms, ticks, warm):
    tick_sf = SR * tick_ms // 1000
    src = pool(tick_sf * (ticks + warm))
    res = {"streams": n, "tick_ms": tick_ms}
    for mode in ("encode_streams", "push_samples"):
        encs = [flo_amd.LossyStreamingEncoder(SR, CH, Q, ctx=ctx) for _ in range(n)]
        frames = 0
        wall = 0.0
        call = 0.0
        for t in range(ticks + warm):
            if t == warm:
                ctx.profile_enable(mode == "encode_streams")
                ctx.profile_reset()
                for e in encs:   # count only what the measured ticks make
                    while e.next_frame() is not None:
                        pass
            a = t * tick_sf * CH
            t0 = time.perf_counter()
            if mode == "encode_streams":
                for i, e in enumerate(encs):
                    e.append_samples(src[i % len(src)][a:a + tick_sf * CH])
                t1 = time.perf_counter()
                r = flo_amd.encode_streams(encs)
                assert not r.status.any(), r.errors
            else:
                t1 = time.perf_counter()
                for i, e in enumerate(encs):
                    e.push_samples(src[i % len(src)][a:a + tick_sf * CH])
            t2 = time.perf_counter()
            if t >= warm:
                wall += t2 - t0
                call += t2 - t1
        frames = sum(e.pending_frames() for e in encs)
        key = "batched" if mode == "encode_streams" else "per_stream"
        res[key + "_ms_per_tick"] = 1e3 * wall / ticks
        res[key + "_call_ms_per_tick"] = 1e3 * call / ticks
        res[key + "_frames_per_s"] = frames / wall if wall else 0.0
        if mode == "encode_streams":
            res["kernel_ms_per_tick"] = sum(ctx.profile_query(k)[0] for k in KERNELS) / ticks
            res["upload_mb_per_tick"] = n * (tick_sf + 1024) * CH * 4 / 1e6   # windows: new samples + carried block
            ctx.profile_enable(False)
        res["frames_per_tick"] = frames / ticks
        for e in encs:
            e.close()
    return res


def main():
    out = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1].endswith(".json") else None
    ns = [int(a) for a in sys.argv[1:] if a.isdigit()] or [1, 64, 1024]
    ctx = flo_amd.Context(0)
    rows = []
    for n in ns:
        for tick_ms in TICKS_MS:
            ticks = 50 if tick_ms < 1000 else 10
            if n >= 1024:
                ticks = 10 if tick_ms < 1000 else 4
            r = run(ctx, n, tick_ms, ticks, warm=3)
            rows.append(r)
            print(f"N={n:5d} tick={tick_ms:4d} ms: encode_streams {r['batched_ms_per_tick']:8.3f} ms/tick "
                  f"(call {r['batched_call_ms_per_tick']:8.3f}, kernels {r['kernel_ms_per_tick']:7.3f}, "
                  f"upload {r['upload_mb_per_tick']:7.2f} MB) {r['batched_frames_per_s']:10.0f} frames/s | "
                  f"push_samples {r['per_stream_ms_per_tick']:8.3f} ms/tick {r['per_stream_frames_per_s']:10.0f} frames/s",
                  flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
