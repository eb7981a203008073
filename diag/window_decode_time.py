"""Corpus window decode rate: random 1-s stereo windows from a corpus of synthetic 180-s files encoded on the device in
chunks. Reports the kernel time of one decode_windows call (profile hooks) and output Gsamples/s (samples = window
sample-frames x channels), lossy (q = 0.55) and lossless (level 5).
usage: python diag/window_decode_time.py [n_files_lossy] [n_files_lossless] [windows]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flo_amd  # noqa: E402

KERNELS = ["lossy_window", "window_tail", "window_ll_decode_parallel", "window_ll_decode", "window_ll_finish"]


def corpus_files(ctx, mode, n_files, secs=180, sr=44100, ch=2, chunk=64):
    files = []
    for c0 in range(0, n_files, chunk):
        k = min(chunk, n_files - c0)
        b = flo_amd.Batch(ctx, mode, [secs * sr * ch] * k, sr, ch, 0.55 if mode == flo_amd.MODE_LOSSY else 5)
        b.fill_synthetic(seed=3, clip_id0=c0)
        b.encode()
        b.sync()
        files += [b.fetch(i) for i in range(k)]
        b.close()
    return files


def measure(ctx, tag, files, n_windows, reps=10):
    corpus = flo_amd.Corpus(files, ctx)
    sr, ch = corpus.sample_rate, corpus.channels
    rng = np.random.default_rng(1)
    fi = rng.integers(0, len(files), n_windows).astype(np.uint32)
    st = np.array([int(rng.integers(0, corpus.lengths[f] - sr)) for f in fi], np.uint64)
    out = torch.empty((n_windows, sr, ch), dtype=torch.float32, device="cuda")
    for _ in range(3):
        corpus.decode_windows(fi, st, sr, out=out)
    corpus.sync()
    torch.cuda.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        corpus.decode_windows(fi, st, sr, out=out)
    corpus.sync()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / reps
    ms = sum(ctx.profile_query(k)[0] for k in KERNELS) / reps
    ctx.profile_enable(False)
    samples = n_windows * sr * ch
    print(f"{tag}: {len(files)} files, {n_windows} windows of {sr} sample-frames x {ch}: kernels {ms:.3f} ms per call "
          f"({samples / ms / 1e6:.1f} Gsamples/s), wall {wall * 1e3:.3f} ms per call")
    corpus.close()


def main():
    n_lossy = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    n_ll = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    n_win = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
    ctx = flo_amd.Context(0)
    if n_lossy:
        measure(ctx, "lossy q=0.55", corpus_files(ctx, flo_amd.MODE_LOSSY, n_lossy), n_win)
    if n_ll:
        measure(ctx, "lossless level 5", corpus_files(ctx, flo_amd.MODE_LOSSLESS, n_ll), n_win)
    ctx.close()


if __name__ == "__main__":
    main()
