"""The mixing stage's entry in the registry of tests/recycled_scenarios.py (every export is covered by a scenario of
tests/test_gpu_recycled_memory.py or exempt with a reason: tests/test_recycled_memory_cpu.py).

S.SCENARIOS cannot take another late entry: tests/test_gpu_edit.py holds the edit scenario at [-2] when its tests begin and
tests/test_gpu_concurrent_contexts.py has frozen the indices below it. So the mix registers an A, B, A sequence in
S.LEFTOVERS, which nothing indexes. tests/test_gpu_batch_mix.py imports this module; pytest imports test modules in name
order, so the entry is there before tests/test_gpu_late_streams.py, tests/test_gpu_recycled_memory.py and
tests/test_recycled_memory_cpu.py build their lists (test_leftovers[mix], test_late[A, B, A: mix]); the same module runs A
under every fill of S.FILLS itself.

The sequence: what flo_batch_mix and flo_mix return must not depend on what their pool blocks held - the parts, the clips
and the two prefixes of the work list, the frames no part covers, the frames past a source's end and the zero padding behind
the clips of a lossy batch (the files of the mixed batch show that)."""
import numpy as np

import flo_amd
import recycled_scenarios as S

NAME = "mix"
FLT_MAX = np.finfo(np.float32).max


def _clips_a():
    return ([S.noise(5000, 2, 191, 0.4), S.noise(0, 2, 192), S.noise(2049, 2, 193, 0.3), S.noise(1, 2, 194)],
            [S.noise(4300, 2, 195, 0.05), S.noise(600, 2, 196, 0.2)])


def _clips_b():
    first, second = [np.array(x) for x in _clips_a()[0]], [np.array(x) for x in _clips_a()[1]]
    for x in first + second:
        for k, v in enumerate((np.nan, np.inf, -np.inf, FLT_MAX, -FLT_MAX)):
            if x.size:
                x[(k * 977) % x.size] = np.float32(v)
    return first, second


PARTS_A = [
    dict(out=0, clip=0, start=3, frames=4100, at=5, fade_in=100, fade_out=4100), dict(out=0, batch=1, clip=0, at=2000, gain=0.5),   # overlap, fades
    dict(out=1, clip=2, start=2040, frames=300, at=1),                                # past the source's end
    dict(out=1, batch=1, clip=1, start=10, frames=50, at=4000, gain=-1.0, fade_in=50),   # a gap in front of it
    dict(out=3, clip=3, at=7), dict(out=3, clip=1, at=2),                             # (output 2 has no part)
    dict(out=4, clip=0, start=1, frames=2048), dict(out=4, clip=0, start=1, frames=2048, at=480, gain=0.25),   # an echo
]
FRAMES_A = [6300, 4200, 700, 9, 2048, 0]
PARTS_B = PARTS_A[:2] + [dict(out=0, batch=b, clip=c, start=7 * j, frames=900 + j, at=31 * j, gain=0.1 * (j % 5 - 2), fade_in=j, fade_out=2 * j)
                         for j in range(150) for b, c in ((0, 0), (1, 0))] + [dict(out=1, clip=2, at=3000), dict(out=2, clip=0, at=5000, fade_out=5000)]
FRAMES_B = [9000, 9000, 12000, 4096]


def _upload(b, clips):
    for i, x in enumerate(clips):
        b.upload(i, x)


def _a(ctx, lossy, other):
    first, second = _clips_a()
    _upload(lossy, first)
    _upload(other, second)
    rec = []
    out = lossy.mix(PARTS_A, FRAMES_A, others=(other,))
    try:
        rec += [("clip %d" % i, out.download_pcm(i).tobytes()) for i in range(out.n_clips)]
        out.encode()
        out.sync()
        rec += [("file %d" % i, out.fetch(i)) for i in range(out.n_clips)]
    finally:
        out.close()
    cat = lossy.concat([[0, 2, 3], [], [2, 1, 0]], crossfade_ms=5.0)
    try:
        rec += [("concat %d" % i, cat.download_pcm(i).tobytes()) for i in range(cat.n_clips)]
    finally:
        cat.close()
    one = ctx.mix([first[0], second[0]], S.SR, 2, [dict(out=0, clip=0, start=9, frames=4000, at=3, fade_in=50, fade_out=60),
                                                  dict(out=0, clip=1, at=1000, gain=0.5)], 5000)
    rec.append(("flo_mix", one.tobytes()))
    return rec


def _b(ctx, lossy, other):
    first, second = _clips_b()
    _upload(lossy, first)
    _upload(other, second)
    out = lossy.mix(PARTS_B, FRAMES_B, others=(other,))
    try:
        for i in range(out.n_clips):
            out.download_pcm(i)
    finally:
        out.close()
    ctx.mix(first + second, S.SR, 2, [dict(out=0, clip=j % 6, start=j, at=11 * j, gain=0.5) for j in range(200) if j % 6 not in (1,)], 9000)


def _sources(ctx):
    first, second = _clips_a()
    return (flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [c.size for c in first], S.SR, 2, 0.55),
            flo_amd.Batch(ctx, flo_amd.MODE_LOSSLESS, [c.size for c in second], S.SR, 2, 5))


def mix_a(ctx):
    """A on source batches of its own"""
    lossy, other = _sources(ctx)
    try:
        return _a(ctx, lossy, other)
    finally:
        lossy.close()
        other.close()


def mix_aba(ctx):
    fresh = S._fresh_context(mix_a)
    lossy, other = _sources(ctx)
    try:
        first = _a(ctx, lossy, other)
        _b(ctx, lossy, other)
        return fresh, first, _a(ctx, lossy, other)
    finally:
        lossy.close()
        other.close()


if NAME not in [s["name"] for s in S.LEFTOVERS]:
    S.LEFTOVERS.append(dict(name=NAME, covers=["flo_batch_mix", "flo_mix"], run=mix_aba))
