"""Fidelity reports against the batch decode they build on, in one process, alternating, medians of several runs:
flo_batch_decode into device memory, the fused flo_batch_fidelity (lossy: one decode-and-compare pass that writes no PCM)
and the same with FLO_FIDELITY_UNFUSED=1 (decode into scratch, compare behind it). Three batches: 1250 synthetic 10 s
stereo clips at quality 0.55, one 180 s stereo clip, 128 lossless 96 kHz stereo clips. Device times from the profile
hooks (event brackets around the launches); kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python diag/fidelity_time.py` run.
usage: python diag/fidelity_time.py [runs]"""
import os
import statistics
import sys
import time

sys.path.insert(0, ".")
import torch  # noqa: E402

import flo_amd  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
ctx = flo_amd.Context(0)


def make(mode, n, secs, sr, q):
    n_il = int(secs * sr) * 2
    b = flo_amd.Batch(ctx, mode, [n_il] * n, sr, 2, q)
    b.fill_synthetic(seed=0xF10A0D10, clip_id0=1)
    b.encode(0)
    b.sync()
    return b


def timed(fn, names):
    ctx.profile_reset()
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    wall = time.perf_counter() - t
    return wall * 1e3, sum(ctx.profile_query(k)[0] for k in names)


def measure(tag, b, decode_kernels):
    rep = b.fidelity()
    total = sum(r["decoded_frames"] for r in rep) * 2
    out = torch.empty(total, dtype=torch.float32, device="cuda:0")
    pcm_gb = total * 4 / 1e9

    def decode():
        b.decode_to(out.data_ptr(), out.numel())

    def fused():
        os.environ.pop("FLO_FIDELITY_UNFUSED", None)
        b.fidelity()

    def unfused():
        os.environ["FLO_FIDELITY_UNFUSED"] = "1"
        b.fidelity()
        os.environ.pop("FLO_FIDELITY_UNFUSED", None)

    ctx.profile_enable(True)
    for f in (decode, fused, unfused):   # warm-up: pool allocations, tables
        f()
    res = {"decode": [], "fused": [], "unfused": []}
    for _ in range(runs):
        res["decode"].append(timed(decode, decode_kernels))
        res["fused"].append(timed(fused, ["fidelity"]))
        res["unfused"].append(timed(unfused, decode_kernels + ["fidelity"]))
    ctx.profile_enable(False)
    assert b.fidelity()[0]["signal"].tobytes() == rep[0]["signal"].tobytes()
    print(f"{tag}: {len(rep)} clips, {pcm_gb:.2f} GB of decoded PCM, median of {runs}")
    for k, v in res.items():
        w = statistics.median(x[0] for x in v)
        d = statistics.median(x[1] for x in v)
        print(f"  {k:8s}: {w:9.2f} ms wall, {d:9.3f} ms device (profile hooks)")
    snr = [float(r["snr_db_all"]) for r in rep]
    print(f"  SNR over the clips: min {min(snr):.2f} dB, median {statistics.median(snr):.2f} dB, max {max(snr):.2f} dB")


lossy_names = ["lossy_decode"]
ll_names = ["ll_decode_parallel", "ll_decode", "ll_finish"]
b = make(flo_amd.MODE_LOSSY, 1250, 10, 44100, 0.55)
measure("lossy 1250 x 10 s stereo, q 0.55", b, lossy_names)
b.close()
b = make(flo_amd.MODE_LOSSY, 1, 180, 44100, 0.55)
measure("lossy 1 x 180 s stereo, q 0.55", b, lossy_names)
b.close()
b = make(flo_amd.MODE_LOSSLESS, 128, 10, 96000, 5)
measure("lossless 128 x 10 s stereo 96 kHz", b, ll_names)
b.close()
ctx.close()
