"""The batch editing stage's entries in the registry of tests/recycled_scenarios.py (every export is covered by a scenario of
tests/test_gpu_recycled_memory.py or exempt with a reason: tests/test_recycled_memory_cpu.py).

Only tests/test_gpu_edit.py imports this module. tests/test_gpu_concurrent_contexts.py, which pytest imports
before it, freezes the number and the names of the scenarios at import but indexes the live list while its tests run, so a
scenario registered at any index below that number would run there under another scenario's name and push that one out.
Registration therefore has two steps:
* on import the scenario is appended BEHIND the last one: no index that a module has frozen moves, and the modules imported
  later (tests/test_gpu_late_streams.py, tests/test_gpu_recycled_memory.py) find its name when they build their lists;
* take_place(), which a module-wide fixture of tests/test_gpu_edit.py calls when that module's tests begin - behind the
  concurrent-contexts tests, in front of the late-stream, recycled-memory and registry tests - moves it in front of the last
  one, whose place the registry's test fixes.
The concurrent-contexts tests thus run exactly the scenarios they name, and do not run this one.

The scenario: what flo_batch_edit, flo_batch_active_range and flo_edit return must not depend on what their pool blocks
held - the segments and the tile prefix, the start values of the range words, the pads, the frames past the source's end
and the zero padding behind the clips of a lossy batch (the files of the edited batch show that)."""
import numpy as np

import flo_amd
import recycled_scenarios as S

S.EXEMPT.setdefault("flo_edit_tile_frames", "host arithmetic")

NAME = "edit: cuts, pads, fades, remixes and active ranges"


def _quiet_ends(x, ch, head, tail):
    y = np.array(x, np.float32).reshape(-1, ch)
    y[:head] = 0
    if tail:
        y[-tail:] = 0
    return y.reshape(-1)


def edit(ctx):
    clips = [_quiet_ends(S.noise(5000, 2, 91), 2, 300, 450), S.noise(0, 2, 92), _quiet_ends(S.noise(2049, 2, 93, 0.3), 2, 0, 7), S.noise(1, 2, 94),
             np.zeros(2 * 600, np.float32), S.noise(4300, 2, 95, 0.05)]
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [c.size for c in clips], S.SR, 2, 0.55)
    rec = []
    try:
        for i, x in enumerate(clips):
            b.upload(i, x)
        rec.append(("active ranges", np.ascontiguousarray(b.active_ranges(-40.0)).tobytes()))
        segs = [dict(clip=0, start=3, frames=4100, pad_head=5, pad_tail=2051, fade_in=100, fade_out=4100), dict(clip=2, start=2040, frames=300, pad_head=1),
                dict(clip=5), dict(clip=1, pad_tail=9), dict(clip=0, start=1, frames=2048), dict(clip=3, start=7, frames=3)]
        for what, out in (("copy", b.edit(segs)), ("mono", b.edit(segs, 1, [[0.5, -0.5]])), ("wide", b.edit(segs, 3, [[1, 0], [0, 1], [0.25, 0.75]]))):
            try:
                rec += [("%s clip %d" % (what, i), out.download_pcm(i).tobytes()) for i in range(out.n_clips)]
                if what != "wide":
                    out.encode()
                    out.sync()
                    rec += [("%s file %d" % (what, i), out.fetch(i)) for i in range(out.n_clips)]
            finally:
                out.close()
        out, ranges = b.trim_silence(-40.0, pre_ms=1.0, post_ms=2.0, fade_ms=3.0)
        try:
            rec.append(("trim ranges", np.ascontiguousarray(ranges).tobytes()))
            rec += [("trim clip %d" % i, out.download_pcm(i).tobytes()) for i in range(out.n_clips)]
        finally:
            out.close()
    finally:
        b.close()
    one = ctx.edit(clips[0], S.SR, 2, dict(start=9, frames=4000, pad_head=3, pad_tail=3, fade_in=50, fade_out=60), 2, [[0, 1], [1, 0]])
    rec.append(("flo_edit", one.tobytes()))
    mono = flo_amd.Batch(ctx, flo_amd.MODE_LOSSLESS, [3000], S.SR, 1, 5)
    try:
        mono.upload(0, S.noise(3000, 1, 96))
        up = mono.remix([[1.0], [-1.0]])
        try:
            rec.append(("1 to 2", up.download_pcm(0).tobytes()))
        finally:
            up.close()
    finally:
        mono.close()
    return rec


def take_place():
    """move the scenario from behind the last of the others to in front of it; does nothing once it is there"""
    names = [s["name"] for s in S.SCENARIOS]
    if len(names) >= 2 and names[-1] == NAME:
        mine = S.SCENARIOS.pop()
        S.SCENARIOS.insert(len(S.SCENARIOS) - 1, mine)


if NAME not in [s["name"] for s in S.SCENARIOS]:
    S.SCENARIOS.append(dict(name=NAME, covers=["flo_batch_edit", "flo_batch_active_range", "flo_edit"], run=edit))
