"""Streaming decode rate: n streaming decoders over synthetic 180-s stereo files (encoded on the device; distinct files
are reused across streams), each fed about one second of new bytes per call, then one decode_streams over all of them.
Reports the kernel time per call (profile hooks) and output Gsamples/s (samples = sample-frames x channels), lossy
(q = 0.55) and lossless (level 5).
usage: python diag/sdec_time.py [n_lossy_streams] [n_lossless_streams] [calls]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flo_amd  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from window_decode_time import corpus_files  # noqa: E402

KERNELS = ["sdec_lossy", "sdec_ll_decode_parallel", "sdec_ll_decode", "sdec_ll_finish"]


def measure(ctx, tag, files, n_streams, calls, warm=3, secs=180):
    decs = [flo_amd.StreamingDecoder(ctx) for _ in range(n_streams)]
    blobs = [files[i % len(files)] for i in range(n_streams)]
    head = [70 + int.from_bytes(b[38:46], "little") for b in blobs]   # header + TOC up front
    per_call = [max(1, (len(b) - h) // secs) for b, h in zip(blobs, head)]
    pos = [0] * n_streams
    out = torch.empty(n_streams * 48 * 1024 * 2 * 2, dtype=torch.float32, device="cuda")

    def one_call():
        for i, d in enumerate(decs):
            step = head[i] + per_call[i] if pos[i] == 0 else per_call[i]
            d.feed(blobs[i][pos[i]:pos[i] + step])
            pos[i] += step
        r = flo_amd.decode_streams(decs, out=out)
        return int(r.offsets[-1])

    for _ in range(warm):
        one_call()
    torch.cuda.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    samples = 0
    for _ in range(calls):
        samples += one_call()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / calls
    ms = sum(ctx.profile_query(k)[0] for k in KERNELS) / calls
    ctx.profile_enable(False)
    per = samples / calls
    print(f"{tag}: {n_streams} streams ({len(files)} distinct files), ~1 s of bytes per stream per call: "
          f"{per / 1e6:.1f} Msamples per call, kernels {ms:.3f} ms per call ({per / ms / 1e6:.1f} Gsamples/s), "
          f"wall {wall * 1e3:.1f} ms per call (host feed + plan included)")
    for d in decs:
        d.close()


def main():
    n_lossy = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    n_ll = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    calls = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    ctx = flo_amd.Context(0)
    if n_lossy:
        measure(ctx, "lossy q=0.55", corpus_files(ctx, flo_amd.MODE_LOSSY, 64), n_lossy, calls)
    if n_ll:
        measure(ctx, "lossless level 5", corpus_files(ctx, flo_amd.MODE_LOSSLESS, 64), n_ll, calls)
    ctx.close()


if __name__ == "__main__":
    main()
