"""The partitioned FFT convolution's entry in the registry of tests/recycled_scenarios.py (every export is covered by a
scenario of tests/test_gpu_recycled_memory.py or exempt with a reason: tests/test_recycled_memory_cpu.py).

Like the FIR stage (tests/convolve_recycled.py) it registers an A, B, A sequence in S.LEFTOVERS, which nothing indexes.
tests/test_gpu_fftconv.py imports this module; pytest imports test modules in name order, so the entry is there before
tests/test_gpu_late_streams.py, tests/test_gpu_recycled_memory.py and tests/test_recycled_memory_cpu.py build their lists;
the same module runs A under every fill of S.FILLS itself.

The sequence: what flo_batch_convolve_fft and flo_convolve_fft return must not depend on what their pool blocks held - the
work lists, the twiddles, the spectra of segments and responses (B leaves NaN and infinities in both), the segments that are
not stored, the blocks no segment reaches and the zero padding behind the clips of a lossy batch (the files of the filtered
batch show that). The host-only export is called through flo_amd/api.py on the way: the geometry places the lengths."""
import numpy as np

import flo_amd
import recycled_scenarios as S

NAME = "fftconv"
FLT_MAX = np.finfo(np.float32).max


def _geometry():
    return flo_amd.conv_fft_geometry(2, 1)


def _clips_a():
    g = _geometry()
    tile, B = g["block_frames"] * g["lane_blocks"], g["block_frames"]
    return ([S.noise(tile + 900, 2, 391, 0.4), S.noise(0, 2, 392), S.noise(tile + 1, 2, 393, 0.3), S.noise(1, 2, 394)],
            [S.noise(2 * B + 70, 1, 395, 0.1).reshape(-1), S.noise(40, 1, 396, 0.2).reshape(-1), np.zeros(0, np.float32)])


def _clips_b():
    first, second = [np.array(x) for x in _clips_a()[0]], [np.array(x) for x in _clips_a()[1]]
    g = _geometry()
    second[1] = np.array(S.noise((g["lane_blocks"] + 2) * g["block_frames"] + 9, 1, 397, 0.1)).reshape(-1)
    for x in first + second:
        for k, v in enumerate((np.nan, np.inf, -np.inf, FLT_MAX, -FLT_MAX)):
            if x.size:
                x[(k * 977) % x.size] = np.float32(v)
    return first, second


def _jobs_a():
    g = _geometry()
    B = g["block_frames"]
    tile = B * g["lane_blocks"]
    return [dict(clip=0, ir=0, skip=31), dict(clip=0, ir=1, frames=tile + 900 + 39), dict(clip=2, ir=0, skip=5, ir_start=3, taps=B + 1),
            dict(clip=1, ir=0, frames=70), dict(clip=3, ir=1, frames=45), dict(clip=2, ir=2, frames=9), dict(clip=0, ir=0, frames=0),
            dict(clip=2, ir=0, frames=300, skip=tile - 100), dict(clip=2, ir=1, frames=tile + 4 * B, skip=0)]


def _jobs_b():
    g = _geometry()
    tile = g["block_frames"] * g["lane_blocks"]
    return _jobs_a() + [dict(clip=j % 4, ir=j % 3, frames=200 + 37 * j, skip=11 * j, ir_start=j % 5) for j in range(40)] + \
        [dict(clip=0, ir=1, frames=2 * tile + 3, skip=g["block_frames"])]


def _upload(b, clips):
    for i, x in enumerate(clips):
        b.upload(i, x)


def _a(ctx, lossy, irs):
    first, second = _clips_a()
    _upload(lossy, first)
    _upload(irs, second)
    rec = []
    out = lossy.convolve(irs, _jobs_a(), method="fft")
    try:
        rec += [("clip %d" % i, out.download_pcm(i).tobytes()) for i in range(out.n_clips)]
        out.encode()
        out.sync()
        rec += [("file %d" % i, out.fetch(i)) for i in range(out.n_clips)]
    finally:
        out.close()
    one = ctx.convolve(first[2], second[0], S.SR, 2, 1, mode="full", method="fft")
    rec.append(("flo_convolve_fft", one.tobytes()))
    return rec


def _b(ctx, lossy, irs_b):
    first, second = _clips_b()
    _upload(lossy, first)
    _upload(irs_b, second)
    out = lossy.convolve(irs_b, _jobs_b(), method="fft")
    try:
        for i in range(out.n_clips):
            out.download_pcm(i)
    finally:
        out.close()
    ctx.convolve(first[0], first[2][:600], S.SR, 2, 2, dict(frames=5000, skip=100), method="fft")


def _sources(ctx, clips):
    first, second = clips
    return (flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [c.size for c in first], S.SR, 2, 0.55),
            flo_amd.Batch(ctx, flo_amd.MODE_LOSSLESS, [c.size for c in second], S.SR, 1, 5))


def fftconv_a(ctx):
    """A on batches of its own"""
    lossy, irs = _sources(ctx, _clips_a())
    try:
        return _a(ctx, lossy, irs)
    finally:
        lossy.close()
        irs.close()


def fftconv_aba(ctx):
    fresh = S._fresh_context(fftconv_a)
    lossy, irs = _sources(ctx, _clips_a())
    irs_b = _sources(ctx, _clips_b())
    irs_b[0].close()
    try:
        first = _a(ctx, lossy, irs)
        _b(ctx, lossy, irs_b[1])
        return fresh, first, _a(ctx, lossy, irs)
    finally:
        lossy.close()
        irs.close()
        irs_b[1].close()


if NAME not in [s["name"] for s in S.LEFTOVERS]:
    S.LEFTOVERS.append(dict(name=NAME, covers=["flo_batch_convolve_fft", "flo_convolve_fft", "flo_conv_fft_geometry"], run=fftconv_aba))
