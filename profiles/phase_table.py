#!/usr/bin/env python3
"""Static per-phase instruction counts of the transform wave of lossy_chain2q_kernel from a -DFLO_MARKS assembly listing.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -ffp-contract=off -Iinclude -DFLO_MARKS \
        -S --cuda-device-only -o /tmp/lk_marks.s flo_amd/csrc/lossy_kernels.hip
  python3 profiles/phase_table.py /tmp/lk_marks.s [mangled-name-substring]

The markers pin the schedule (they are memory clobbers), so the counts are those of the marked build, a few per cent
above the shipped one. A frame loop the compiler laid out rotated (latch in front of the header) is recognised and
counted in program order. Counted per stereo frame: the counts of a phase are divided by the number of frame bodies in
the listing (one; two while the loop was unrolled by two). What follows the last frame_end marker runs once per clip,
not per frame (the loop's back edge, the last frame's masking pass, the clip loop): it is listed apart and not summed.
"""
import collections
import re
import sys


def classify(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    return None


def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "lossy_chain2q_kernelILb0ELj48574ELb0EE"
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and want in l and ":" in l.split(";")[0])
    end = next(i for i in range(start, len(lines)) if ".size" in lines[i] and want in lines[i])
    phases = collections.OrderedDict()
    cur = "pre (clip set-up, packer wave)"
    order = []
    bodies = max(1, sum(1 for l in lines[start:end] if l.strip().startswith("; MARK frame_begin")))
    last_end = max((i for i in range(start, end) if lines[i].strip().startswith("; MARK frame_end")), default=end)
    # A rotated frame loop (the compiler lays the latch - the tail of the band statistics and the next frame's fold - out in
    # front of the loop header, so frame_end precedes frame_begin in the listing): the loop's code runs from the latch's
    # label to the label the latch leaves the loop for; between the latch's label and the first marker lies the end of the
    # phase behind the LAST marker of the listing, and what follows the exit label runs once per clip.
    marks = [(i, re.match(r"; MARK (\w+)", lines[i].strip()).group(1)) for i in range(start, end) if lines[i].strip().startswith("; MARK ")]
    first = {n: min(i for i, m in marks if m == n) for n in {m for _, m in marks}}
    rotated = "frame_end" in first and "frame_begin" in first and first["frame_end"] < first["frame_begin"]
    loop_start = post_start = None
    if rotated:
        label_at = lambda i: max(j for j in range(start, i + 1) if re.match(r"\.LBB\d+_\d+:", lines[j]))
        loop_start, header = label_at(marks[0][0]), label_at(first["frame_begin"])
        leave = next(lines[j] for j in range(header - 1, loop_start, -1) if lines[j].strip().startswith("s_cbranch"))
        exit_label = leave.split()[1]
        post_start = next(j for j in range(start, end) if lines[j].startswith(exit_label + ":"))
        assert post_start > marks[-1][0], "the loop's exit lies behind its last marker"
    for i, l in enumerate(lines[start:end], start):
        if rotated:
            if i == loop_start:
                cur = marks[-1][1]
            elif i == post_start:
                cur = "post (behind the frame loop)"
        elif i == last_end + 1:
            cur = "post (behind the last frame_end)"
        s = l.strip()
        m = re.match(r"; MARK (\w+)", s)
        if m:
            cur = m.group(1)
            continue
        if not s or s.startswith((";", ".", "//")) or s.endswith(":"):
            continue
        op = s.split()[0]
        k = classify(op)
        if k is None:
            continue
        # the phase a marker NAMES ends at the marker: instructions belong to the NEXT marker seen; collect by previous
        phases.setdefault(cur, collections.Counter())[k] += 1
        if cur not in order:
            order.append(cur)
    if rotated:   # program order: the header's phase first, the latch's phases last
        seq = [m for _, m in marks]
        k = seq.index("frame_begin")
        prog = seq[k:] + seq[:k]
        order = [o for o in order if o.startswith("pre (")] + [m for m in prog if m in order] + [o for o in order if o.startswith("post (")]
    # instructions after marker X and before marker Y belong to phase Y
    # (round 4: the frame loop is software-pipelined - the next frame's fold runs at the end of a frame, the masking pass of the
    # previous frame inside the FFT, behind the first exchange)
    # what FOLLOWS each marker (round 4: the frame loop is software-pipelined - the next frame's fold runs at the end of a
    # frame, the masking pass of the previous frame inside the FFT, behind the first exchange)
    # (the prefetch is issued behind the FFT: frame_begin, fft_done, prefetch_done, postrot_done, ...)
    names = {"frame_begin": "masking rows, fft512 x2 + masking pass (prev. frame)", "fft_done": "prefetch (16 loads)",
             "prefetch_done": "post-rotation + transpose", "postrot_done": "band_stats_2",
             "bandstats_done": "fold of the next frame (a)", "frame_end": "fold of the next frame (b), loop"}
    print(f"{'phase':32s} {'VALU':>6s} {'SALU':>6s} {'LDS':>5s} {'VMEM':>5s} {'wait':>5s}   (per stereo frame, {bodies} frame bod{'y' if bodies == 1 else 'ies'})")
    tot = collections.Counter()
    for ph in order:
        c = phases[ph]
        nm = names.get(ph, ph)
        once = ph.startswith(("pre (", "post ("))
        div = 1 if once else bodies
        row = {k: c[k] / div for k in ("valu", "salu", "lds", "vmem", "wait")}
        if not once:
            for k, v in row.items():
                tot[k] += v
        print(f"{nm:32s} {row['valu']:6.0f} {row['salu']:6.0f} {row['lds']:5.0f} {row['vmem']:5.0f} {row['wait']:5.0f}")
    print(f"{'transform wave, per frame':32s} {tot['valu']:6.0f} {tot['salu']:6.0f} {tot['lds']:5.0f} {tot['vmem']:5.0f} {tot['wait']:5.0f}")


if __name__ == "__main__":
    main()
