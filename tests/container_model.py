"""The container finish by model: an independent writer of header + TOC, the path predicates of the device's finish
(container_kernels.hip, crc_device.hpp, tail_crc in lossy_kernels.hip), and the shared list of cases.

`head_and_toc` writes bytes 0 .. 74 + 20 nf of a .flo file from the frames' (bytes, samples) in plain Python integers,
as writer.rs:132-224 does; the CRC field is zlib's. It knows nothing of slices, stripes or chunks.

The predicates say which data-dependent branch of the device code a clip takes. They follow the kernels' constants,
restated below; tests/test_container_model_cpu.py reads the same constants out of the sources as text and compares.

  slice arithmetic (crc_slice_reg<NT>)   a slice of `len` bytes is cut into stripes of NT * 64 bytes: full = len / stripe
      complete stripes, then nb = rem / 64 whole blocks and last = rem % 64 bytes. NT = 256: crc_slices_kernel, the fused
      crc_and_toc_kernel and crc_fallback_256; NT = 64: the chain encode's tail (one wave per slice).
  slice layout (crc_slice_range)         s = ceil(n / parts) rounded up to 16 KiB; slice p = [min(p s, n), ...)
  powers of x (x8n_fast)                 three tables below 4 MiB, bit by bit from 4 MiB; called with n and with every
      non-empty slice's distance to the end of the chunk
  fin256 (finish_files_kernel<256>)      many clips: one workgroup writes a clip's whole TOC, thread t owns a run of
      per = ceil(nf / 256) frames; the first eight of a run sit in registers, a loop takes the rest
  fused (crc_and_toc_kernel)             few clips: TOC chunks of 256 frames, one workgroup each, which first sums the
      frames in front of its chunk 1024 at a time
  wide (finish_files_kernel<1024>)       few clips and no frames at all
  timestamps                             floor(cum * 1000 / rate) carried as quotient and remainder inside a run

Which clips of a many-clips stereo batch the encode's tail reaches depends on timing: the NT = 64 names say what the tail
computes IF it takes the clip, and the GPU test asserts only that the files do not depend on it.

Not reached by any case (the reach test allows only these names in that list):

  ts:div64_in_run   the 64-bit division inside `entry` is taken when samples * 1000 + r >= 2^32, one frame of at least
                    4,294,968 samples. Its result is used only by the NEXT entry of the same thread's run, and a run of two
                    entries exists only in finish_files_kernel<256> with nf > 256 (the fused and the 1024-thread forms give
                    every thread one entry): 257 frames of 4.3 M samples are 1.1e9 samples, 4.4 GB of PCM for one clip.
                    The oracle and the API do accept such a rate: `ll_5mhz_two_frames` has two frames of a 5 MHz clip and
                    reaches the 64-bit division that starts a run (`ts:first_division_over_32bit`) instead.
  nt64:last63, nt64:one_byte   NT = 64 is the chain encode's tail, which runs only for lossy stereo. Slices start at multiples
                    of 16 KiB, so both names need an odd DATA length, and silent stereo frames are 126 bytes each: the length
                    is odd only with non-zero coefficients in the file. Those the device reproduces within the f32 transform's
                    tolerance (tests/gpu_util.py compare_lossy_stage: coefficients to 1e-5 relative RMS, an integer next to
                    a rounding boundary may differ by one), not byte for byte, so a case that asserts the oracle's whole file
                    cannot hold them: with the two tone clips of `tone_case` among its clips, chain_stereo_256 differed
                    from the oracle inside the first tone clip's DATA (same length, header and TOC equal to the model's, CRC
                    equal to zlib's). The tone clips run in a test of their own, which checks everything but the oracle's
                    bytes, takes the paths from the lengths the device returned and ASSERTS that they hold both names:
                    the first two clips' DATA is 16,385 and 1983 bytes by the oracle and on the device. If a change of the
                    encoder's rounding moves those lengths the test fails, and FOUND has to be searched again.

The lengths and seeds in FOUND were found by searching the oracle on the CPU (sample counts for the lossless Rice
cases, tone frequencies for the lossy stereo ones); the CPU test proves they still hold for the oracle.
"""
import functools
import os
import re
import struct
import zlib

import numpy as np

import flofile
import signals
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flo_amd", "csrc")

# ------------------------------------------------------------------------------------------------ constants, restated
K_BLK = 64                     # crc_device.hpp kBlk
K_SLICE_ALIGN = 256 * K_BLK    # crc_device.hpp kSliceAlign
K_FEW_CLIPS = 64               # encode_plan.hpp kFewClips
K_FIN_THREADS = 256            # container_kernels.hip kFinThreads; the fused form's TOC chunk
WIDE_THREADS = 1024            # finish_files_kernel<1024> and its TOC chunk
X8N_FAST_BOUND = 256 << 14     # container_kernels.hip x8n_fast: 4 MiB
RUN_REGS = 8                   # TOC entries of a run kept in registers
FRONT_UNROLL = 4               # loads per thread and stride of the front-of-chunk sum
PARTS_TARGET, PARTS_ONE_FROM, PARTS_CAP_FEW, PARTS_CAP_MANY = 2048, 1024, 512, 128   # encode_plan.cpp finish_parts
CHAIN_AUTO = 512               # encode_plan.cpp lossy_form: n_clips * ch from which auto takes the chain forms
FALLBACK_PARTS_MAX = 128       # container_kernels.hip s_part[128]

NOT_REACHED_ALLOWED = {
    "ts:div64_in_run": "needs a run of two entries (nf > 256 among >= 64 clips) of >= 4,294,968 samples each: 1.1e9 samples",
    "nt64:last63": "no oracle-exact case: needs an odd DATA length in the chain form; reached only by the tone test, which asserts it",
    "nt64:one_byte": "no oracle-exact case: needs an odd DATA length in the chain form; reached only by the tone test, which asserts it",
}


def source_constants():
    """The same constants read out of the sources as text -> dict (compared with the names above by the CPU test)."""
    def src(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()

    def one(text, pattern, what):
        m = re.findall(pattern, text)
        assert len(m) == 1, (what, pattern, m)
        return m[0]
    crc, hpp, cpp, ker = src("crc_device.hpp"), src("encode_plan.hpp"), src("encode_plan.cpp"), src("container_kernels.hip")
    out = {}
    out["K_BLK"] = int(one(crc, r"constexpr unsigned kBlk = (\d+);", "kBlk"))
    out["K_SLICE_ALIGN"] = int(one(crc, r"constexpr unsigned kSliceAlign = (\d+) \* kBlk;", "kSliceAlign")) * out["K_BLK"]
    out["K_FEW_CLIPS"] = int(one(hpp, r"constexpr size_t kFewClips = (\d+);", "kFewClips"))
    out["K_FIN_THREADS"] = int(one(ker, r"constexpr int kFinThreads = (\d+);", "kFinThreads"))
    a, b = one(ker, r"if \(n >= \((\d+)ull << (\d+)\)\) return x8n_tab", "x8n_fast bound")
    out["X8N_FAST_BOUND"] = int(a) << int(b)
    assert len(re.findall(r"A\.toc_chunk = kFinThreads;", ker)) == 1, "the fused form's TOC chunk"
    out["WIDE_THREADS"] = int(one(ker, r"A\.toc_chunk = ([1-9]\d*);", "the 1024-thread TOC chunk"))
    assert len(re.findall(r"finish_files_kernel<%d>\)" % out["WIDE_THREADS"], ker)) == 2, "finish_files_kernel<1024> launches"
    out["RUN_REGS"] = int(one(ker, r"for \(unsigned f = f0 \+ (\d+); f < f1; f\+\+\) entry", "the loop behind the registers"))
    assert one(ker, r"uint32_t kfs\[(\d+)\]", "kfs") == str(out["RUN_REGS"]) and one(ker, r"fbb < f1; fbb \+= (\d+)\)", "fbb") == str(out["RUN_REGS"])
    out["FRONT_UNROLL"] = int(one(ker, r"for \(unsigned f = t; f < c0; f \+= (\d+) \* THREADS\)", "front sum stride"))
    out["FALLBACK_PARTS_MAX"] = int(one(ker, r"__shared__ uint32_t s_part\[(\d+)\];", "s_part"))
    body = re.search(r"unsigned finish_parts\(size_t n_clips\) \{(.*?)\n\}", cpp, re.S).group(1)
    out["PARTS_ONE_FROM"] = int(one(body, r"if \(n_clips >= (\d+)\) return 1;", "parts 1"))
    out["PARTS_TARGET"] = int(one(body, r"\((\d+) \+ n_clips - 1\) / \(n_clips \? n_clips : 1\)", "parts target"))
    few, many = one(body, r"n_clips < kFewClips \? (\d+) : (\d+);", "parts caps")
    out["PARTS_CAP_FEW"], out["PARTS_CAP_MANY"] = int(few), int(many)
    out["CHAIN_AUTO"] = int(one(cpp, r"in\.n_clips \* in\.ch >= (\d+) \?", "auto chain threshold"))
    return out


# ------------------------------------------------------------------------------------------------ the independent writer
# (name, offset, struct format) of the header's fields, bytes 0 .. 69; the TOC's frame count follows at 70
HEADER_FIELDS = [("magic", 0, "4s"), ("version_major", 4, "B"), ("version_minor", 5, "B"), ("flags", 6, "<H"),
                 ("sample_rate", 8, "<I"), ("channels", 12, "B"), ("bit_depth", 13, "B"), ("total_samples", 14, "<Q"),
                 ("level", 22, "B"), ("reserved", 23, "3s"), ("data_crc32", 26, "<I"), ("header_size", 30, "<Q"),
                 ("toc_size", 38, "<Q"), ("data_size", 46, "<Q"), ("extra_size", 54, "<Q"), ("meta_size", 62, "<Q"),
                 ("num_frames", 70, "<I")]


def head_and_toc(frames, sample_rate, channels, flags, bit_depth, level, crc):
    """frames: [(bytes, samples)] -> bytes 0 .. 74 + 20 nf as writer.rs:132-224 writes them (no META)."""
    toc = [struct.pack("<I", len(frames))]
    off = cum = 0
    for i, (nbytes, nsamples) in enumerate(frames):
        toc.append(struct.pack("<IQII", i, off, nbytes, (cum * 1000 // sample_rate) & 0xFFFFFFFF))
        off += nbytes
        cum += nsamples
    toc = b"".join(toc)
    head = b"FLO!" + struct.pack("<BBHIBBQB", 1, 2, flags, sample_rate, channels, bit_depth, cum, level) + b"\0\0\0"
    head += struct.pack("<IQQQQQ", crc, 66, len(toc), off, 0, 0)
    assert len(head) == 70
    return head + toc


def walk_frames(data, channels):
    """DATA -> [(bytes, samples)] read frame after frame from offset 0 out of the frames' own headers (type u8, samples u32,
    flags u8, then per channel a u32 length and that many bytes; a type-253 frame holds one channel). No TOC is consulted."""
    frames, p = [], 0
    while p < len(data):
        ft, fs, _ = struct.unpack_from("<BIB", data, p)
        q = p + 6
        for _ in range(1 if ft == 253 else channels):
            q += 4 + struct.unpack_from("<I", data, q)[0]
        assert q <= len(data), f"frame {len(frames)} at DATA byte {p} runs {q - len(data)} bytes past the end of DATA"
        frames.append((q - p, fs))
        p = q
    return frames


def quality_level(q):
    """lossy/mod.rs:19-128 QualityPreset::from_f32 as the header's byte"""
    return 0 if q < 0.2 else 1 if q < 0.45 else 2 if q < 0.65 else 3 if q < 0.85 else 4


def case_header(c, i=0):
    """(sample rate, channels, flags, bit depth, level) of file i of a case, from the case's own parameters"""
    lossy = c["kind"] != "lossless"
    q = c["qualities"][i // len(c["clips"])] if c["kind"] == "ladder" else c["qol"]
    return c["sr"], c["ch"], (1 | (quality_level(q) << 8)) if lossy else 0, 16, 5 if lossy else c["qol"]


def model_head(file_bytes, header=None):
    """A finished file -> what the writer gives for ITS DATA bytes. flofile.parse only cuts DATA out of the file; the frames'
    sizes and sample counts come from walking DATA from offset 0 (walk_frames), not from the file's TOC, and with `header`
    (case_header) nothing but the position of DATA is taken from the file's own header either."""
    p = flofile.parse(file_bytes)
    sr, ch, flags, depth, level = header or (p.sample_rate, p.channels, p.flags, p.bit_depth, p.level)
    return head_and_toc(walk_frames(p.data, ch), sr, ch, flags, depth, level, zlib.crc32(p.data) & 0xFFFFFFFF)


def head_difference(got, want):
    """First differing field of two header + TOC blocks -> text, or None."""
    if got == want:
        return None
    if len(got) != len(want):
        return f"header + TOC length {len(got)}, want {len(want)}"
    for name, off, fmt in HEADER_FIELDS:
        n = struct.calcsize(fmt)
        if got[off:off + n] != want[off:off + n]:
            return f"header field {name}: {struct.unpack(fmt, got[off:off + n])[0]!r}, want {struct.unpack(fmt, want[off:off + n])[0]!r}"
    for i in range((len(want) - 74) // 20):
        g, w = struct.unpack_from("<IQII", got, 74 + 20 * i), struct.unpack_from("<IQII", want, 74 + 20 * i)
        if g != w:
            return f"TOC entry {i} (index, offset, size, ms): {g}, want {w}"
    return "differs outside every field"


# ------------------------------------------------------------------------------------------------ the plan, restated
def finish_parts(n_clips):
    if n_clips >= PARTS_ONE_FROM:
        return 1
    p = (PARTS_TARGET + n_clips - 1) // (n_clips if n_clips else 1)
    return min(p, PARTS_CAP_FEW if n_clips < K_FEW_CLIPS else PARTS_CAP_MANY)


def plan_finish(n_clips, max_frames, crc_ready):
    few = n_clips < K_FEW_CLIPS
    fused = few and max_frames > 0
    return dict(fused=fused, crc_slices=not fused and (few or not crc_ready), threads=WIDE_THREADS if few else K_FIN_THREADS,
                parts=finish_parts(n_clips))


def describe_plan(p):
    """the wording of tests/native/encode_plan_test.cpp's kFinishRows"""
    return f"{'fused' if p['fused'] else 'slices' if p['crc_slices'] else 'noslices'} {p['threads']} {p['parts']}"


def lossy_form(which, ch, n_clips):
    """encode_plan.cpp lossy_form for an ordinary encode (not exact, no analysis buffers): 5, 1 or 2"""
    if ch > 2:
        return 2
    w = which
    if not w:
        w = (5 if ch == 2 else 1) if n_clips * ch >= CHAIN_AUTO else 2
    if w in (3, 4):
        w = 5
    if w == 5 and ch != 2:
        w = 1
    return w


def slice_range(n, parts, part):
    s = (n + parts - 1) // parts
    s = (s + K_SLICE_ALIGN - 1) // K_SLICE_ALIGN * K_SLICE_ALIGN
    beg = min(part * s, n)
    return beg, (s if beg + s < n else n - beg)


# ------------------------------------------------------------------------------------------------ path predicates
def slice_arith_paths(length, nt):
    """crc_slice_reg<nt> on a non-empty slice"""
    stripe = nt * K_BLK
    full, rem = divmod(length, stripe)
    nb, last = divmod(rem, K_BLK)
    p = {f"nt{nt}:full0" if full == 0 else f"nt{nt}:full1" if full == 1 else f"nt{nt}:full2plus"}
    if nb == 0:
        p.add(f"nt{nt}:nb0")
    if nb == nt - 1:
        p.add(f"nt{nt}:nb{nt - 1}")
    if last == 0:
        p.add(f"nt{nt}:last0")
    if last == K_BLK - 1:
        p.add(f"nt{nt}:last63")
    if full > 0 and nb == 0 and last == 0:
        p.add(f"nt{nt}:ends_on_stripe")
    if full > 0 and nb > 0:
        p.add(f"nt{nt}:stripes_then_blocks")
    if full > 0 and last > 0:
        p.add(f"nt{nt}:stripes_then_last_bytes")
    if length == 1:
        p.add(f"nt{nt}:one_byte")
    return p


def layout_paths(n, parts):
    p = {f"parts:{parts}"}
    if n == 0:
        return p | {"layout:data_0_bytes"}
    lens = [slice_range(n, parts, k)[1] for k in range(parts)]
    s = slice_range(n, parts, 0)[1] if parts > 1 and lens[1] else None
    if parts > 1:
        p.add("layout:all_slices_non_empty" if all(lens) else "layout:empty_slice_behind_non_empty")
        if all(lens) and len(set(lens)) == 1:
            p.add("layout:exactly_parts_x_s")
        if s and n % s == 1:
            p.add("layout:one_byte_over_a_boundary")
    return p


def power_paths(n, parts):
    p = set()
    for d, name in ((-2, "pow:n_4MiB-2"), (0, "pow:n_4MiB"), (2, "pow:n_4MiB+2")):
        if n == X8N_FAST_BOUND + d:
            p.add(name)
    p.add("pow:bit_by_bit" if n >= X8N_FAST_BOUND else "pow:three_tables")
    for k in range(parts):
        beg, length = slice_range(n, parts, k)
        if length and n - beg - length >= X8N_FAST_BOUND:
            p.add("pow:slice_distance_ge_4MiB")
    return p


def timestamp_paths(samples, rate, runs):
    """runs: [(f0, f1)] the frames each thread writes one after the other"""
    p = set()
    cum = [0]
    for s in samples:
        cum.append(cum[-1] + s)
    for f0, f1 in runs:
        if f0 >= f1:
            continue
        if cum[f0] * 1000 >= 1 << 32:
            p.add("ts:first_division_over_32bit")
        r = cum[f0] * 1000 % rate
        for f in range(f0, f1 - 1):     # (the last entry's step is computed and dropped)
            add = samples[f] * 1000 + r
            p.add("ts:div64_in_run" if add >= 1 << 32 else "ts:div32_in_run")
            if r:
                p.add("ts:remainder_carry")
                if rate in (44100, 22050, 11025):
                    p.add(f"ts:carry_at_{rate}")
            r = add % rate
    if len(set(samples)) > 1:
        p.add("ts:varying_frame_samples")
    return p


def toc_paths(plan, nf, max_frames, samples, rate):
    p = set()
    if plan["fused"]:
        chunk = K_FIN_THREADS
        chunks = lambda k: (k + chunk - 1) // chunk
        if chunks(max_frames) == 1:
            p.add("fused:one_chunk")
        if nf == 256:
            p.add("fused:nf256")
        if nf == 257:
            p.add("fused:nf257")
        if chunks(nf) < chunks(max_frames):
            p.add("fused:ends_a_chunk_before_the_longest")
        if any(c0 > FRONT_UNROLL * K_FIN_THREADS for c0 in range(0, nf, chunk)):
            p.add("fused:front_sum_second_stride")
        if nf == 0:
            p.add("fused:nf0_beside_clips_with_frames")
        runs = [(f, f + 1) for f in range(nf)]
    elif plan["threads"] == WIDE_THREADS:
        if max_frames == 0:
            p.add("wide:few_clips_all_empty")
        runs = [(f, f + 1) for f in range(nf)]
    else:
        per = (nf + K_FIN_THREADS - 1) // K_FIN_THREADS
        for k in (1, 2, 8, 9):
            if per == k:
                p.add(f"fin256:per{k}")
        if per >= 17:
            p.add("fin256:per17plus")
        if per > RUN_REGS:
            p.add("fin256:loop_behind_the_registers")
        if nf and (K_FIN_THREADS - 1) * per >= nf:
            p.add("fin256:empty_run")
        if nf and nf % per:
            p.add("fin256:partial_last_run")
        if nf in (0, 1, 255, 256, 257, 2048, 2049):
            p.add(f"fin256:nf{nf}")
        runs = [(min(t * per, nf), min(t * per + per, nf)) for t in range(K_FIN_THREADS)] if nf else []
    return p | timestamp_paths(samples, rate, runs)


def clip_paths(plan, n, nf, max_frames, samples, rate, makers):
    """every named path the finish of one clip takes. makers: which CRC makers run for the batch, of "nt256" (crc_slices_kernel,
    the fused kernel, crc_fallback_256) and "nt64" (the encode's tail, if it takes the clip)"""
    parts = plan["parts"]
    p = layout_paths(n, parts) | power_paths(n, parts) | toc_paths(plan, nf, max_frames, samples, rate)
    for k in range(parts):
        length = slice_range(n, parts, k)[1]
        if length:
            for m in makers:
                p |= slice_arith_paths(length, 256 if m == "nt256" else 64)
    return p


REQUIRED_PATHS = {
    "slices, NT = 256": ["nt256:full0", "nt256:full1", "nt256:full2plus", "nt256:nb0", "nt256:nb255", "nt256:last0", "nt256:last63",
                         "nt256:ends_on_stripe", "nt256:stripes_then_blocks", "nt256:stripes_then_last_bytes", "nt256:one_byte"],
    "slices, NT = 64": ["nt64:full0", "nt64:full1", "nt64:full2plus", "nt64:nb0", "nt64:nb63", "nt64:last0", "nt64:last63",
                        "nt64:ends_on_stripe", "nt64:stripes_then_blocks", "nt64:stripes_then_last_bytes", "nt64:one_byte"],
    "slice layout": ["layout:empty_slice_behind_non_empty", "layout:all_slices_non_empty", "layout:exactly_parts_x_s",
                     "layout:one_byte_over_a_boundary", "layout:data_0_bytes", "parts:1", "parts:8", "parts:32", "parts:128", "parts:512"],
    "powers of x": ["pow:n_4MiB-2", "pow:n_4MiB", "pow:n_4MiB+2", "pow:three_tables", "pow:bit_by_bit", "pow:slice_distance_ge_4MiB"],
    "finish_files<256>": ["fin256:per1", "fin256:per2", "fin256:per8", "fin256:per9", "fin256:per17plus", "fin256:loop_behind_the_registers",
                          "fin256:empty_run", "fin256:partial_last_run", "fin256:nf0", "fin256:nf1", "fin256:nf255", "fin256:nf256",
                          "fin256:nf257", "fin256:nf2048", "fin256:nf2049"],
    "fused": ["fused:one_chunk", "fused:nf256", "fused:nf257", "fused:ends_a_chunk_before_the_longest", "fused:front_sum_second_stride",
              "fused:nf0_beside_clips_with_frames"],
    "finish_files<1024>": ["wide:few_clips_all_empty"],
    "timestamps": ["ts:remainder_carry", "ts:carry_at_44100", "ts:carry_at_22050", "ts:carry_at_11025",
                   "ts:div32_in_run", "ts:varying_frame_samples", "ts:first_division_over_32bit", "ts:div64_in_run"],
    "CRC makers": ["maker:tail", "maker:fallback_256", "maker:crc_slices_form1", "maker:crc_slices", "maker:fused"],
}


# ------------------------------------------------------------------------------------------------ the cases
# found by searching the oracle (see the module docstring)
FOUND = {
    "ll_l2_mono48k_16385": ("noise", 12085, 2, 0.02),        # lossless level 2: DATA = 16385 = 16 KiB + 1
    "ll_l2_mono48k_last63": ("noise", 700, 2, 0.02),         # ... DATA = 959 = 14 * 64 + 63
    "lossy_stereo_16385": ("tone_left", 7844, 300, 119808),   # lossy 44.1 kHz stereo q 0.55: DATA = 16385
    "lossy_stereo_last63": ("tone_left", 5491, 300, 2048),    # ... DATA = 1983 = 30 * 64 + 63
}
FOUND_DATA = {"ll_l2_mono48k_16385": 16385, "ll_l2_mono48k_last63": 959, "lossy_stereo_16385": 16385, "lossy_stereo_last63": 1983}


def make_pcm(spec, ch):
    """("zeros", sample-frames) | ("noise", samples, seed, amp) | ("tone_left", Hz, tone sample-frames, sample-frames): a 44.1 kHz
    tone in the first channel only, silence behind it -> interleaved f32"""
    kind = spec[0]
    if kind == "zeros":
        return np.zeros(spec[1] * ch, np.float32)
    if kind == "noise":
        return signals.fast_noise(spec[1] * ch, spec[2], spec[3])
    if kind == "tone_left":
        x = np.zeros(spec[3] * ch, np.float32)
        x[0:ch * spec[2]:ch] = signals.sine(float(spec[1]), 44100, spec[2], 0.4)
        return x
    raise ValueError(kind)


def _raw_samples(data_bytes, rate=48000):
    """mono sample count whose level-0 (Raw) DATA chunk is data_bytes long: frames of `rate` samples, 10 + 2 k bytes each"""
    full, rest = divmod(data_bytes, 10 + 2 * rate)
    if rest == 0:
        return full * rate
    assert rest >= 12 and rest % 2 == 0, data_bytes
    return full * rate + (rest - 10) // 2


def _lossy_nsf(hops):
    """a sample-frame count that gives `hops` lossy frames (encoder.rs:177-179: (n + 2047) / 1024)"""
    return max(hops * 1024 - 2047, 0) + (hops * 7) % 1000 if hops > 1 else 0


VARIANTS_CHAIN = ("tail", "tail_again", "fallback", "form1")


def cases():
    """-> list of dicts: name, kind (lossless | lossy | ladder), sr, ch, qol (level or quality), clips [spec], qualities (ladder),
    variants (many-clips stereo: the four makers), pack (also through pack_files)"""
    out = []
    M4 = X8N_FAST_BOUND

    def add(name, kind, sr, ch, qol, clips, **kw):
        out.append(dict(name=name, kind=kind, sr=sr, ch=ch, qol=qol, clips=clips, qualities=kw.get("qualities"),
                        variants=kw.get("variants", ("auto",)), pack=kw.get("pack", False)))
    # level 0 stores Raw frames of full-scale noise: DATA is an exact function of the sample count
    raw = lambda nbytes, seed: ("noise", _raw_samples(nbytes), seed, 1.0)
    add("ll_raw_4mib_edges", "lossless", 48000, 1, 0, [raw(M4 - 2, 1), raw(M4, 2), raw(M4 + 2, 3), raw(M4 + 40000, 4)])
    add("ll_few_all_empty", "lossless", 44100, 2, 5, [("zeros", 0)] * 3)
    # 16 clips, 100-sample frames of quiet noise (Rice): the fused form's chunks
    nfs = [0, 1, 255, 256, 257, 1301, 700, 3, 0, 513, 2, 1, 5, 30, 100, 7]
    add("ll_fused_chunks", "lossless", 100, 1, 2, [("noise", nf * 100 - (37 if nf > 2 else 0), 10 + i, 0.02) if nf else ("zeros", 0)
                                                    for i, nf in enumerate(nfs)], pack=True)
    # 64 clips (32 slices), Raw: the slice layout's edges
    sizes = [32 * 16384, 32 * 16384 + 2, 32704, 16384, 16384 + 64, 16382, 16386, 32768, 49152 + 4032, 0, 12, 64, 74, 4096, 128 * 1024]
    sizes += [14 + 2 * ((i * 7919) % 3000) for i in range(64 - len(sizes))]
    add("ll_raw_64_layout", "lossless", 48000, 1, 0, [raw(n, 20 + i) if n else ("zeros", 0) for i, n in enumerate(sizes)])
    # 256 clips (8 slices), level 2: odd lengths
    clips = [FOUND["ll_l2_mono48k_16385"], FOUND["ll_l2_mono48k_last63"]]
    clips += [("noise", 1 + (i * 613) % 2500, 100 + i, 0.02) for i in range(254)]
    add("ll_rice_256_odd", "lossless", 48000, 1, 2, clips)
    # 1024 clips (one slice each)
    clips = [("noise", 13000, 5, 0.02), ("noise", 26000, 6, 0.02), ("zeros", 0)]
    clips += [("noise", 1 + (i * 31) % 90, 300 + i, 0.02) for i in range(1024 - len(clips))]
    add("ll_1024_one_slice", "lossless", 8000, 1, 2, clips)
    # 64 clips of 100-sample frames: finish_files_kernel<256> by frame count
    nfs = [0, 1, 255, 256, 257, 300, 2048, 2049, 4097, 2304, 512]
    nfs += [1 + (i * 37) % 40 for i in range(64 - len(nfs))]
    add("ll_fin256_frames", "lossless", 100, 1, 2, [("noise", nf * 100 - (37 if nf > 2 else 0), 40 + i, 0.02) if nf else ("zeros", 0)
                                                     for i, nf in enumerate(nfs)], pack=True)
    # lossy mono on silence, 64 clips: 1024-sample frames against rates that do not divide 1,024,000
    for sr, nf in ((8000, 2049), (44100, 600), (22050, 300), (11025, 520)):
        hops = [nf, 1, 2, 255, 256, 257] + [1 + (i * 11) % 9 for i in range(58)]
        add(f"lossy_mono_{sr}_64", "lossy", sr, 1, 0.55, [("zeros", _lossy_nsf(h)) for h in hops])
    hops = [1, 256, 257, 1300, 700, 2, 1281, 5]
    add("lossy_mono_8000_fused", "lossy", 8000, 1, 0.55, [("zeros", _lossy_nsf(h)) for h in hops])
    # lossy stereo, 256 clips: the chain form, its tail and the three other makers. Silence gives 126 bytes per frame.
    hops = [32, 33, 66, 131, 1, 2, 16, 65, 130, 260, 3, 64]
    clips = [("zeros", _lossy_nsf(h)) for h in hops]
    clips += [("zeros", _lossy_nsf(1 + (i * 29) % 70)) for i in range(256 - len(clips))]
    add("chain_stereo_256", "lossy", 44100, 2, 0.55, clips, variants=VARIANTS_CHAIN, pack=True)
    # ladders: rungs x clips is the finish's clip count
    q4 = [0.0, 0.35, 0.55, 1.0]
    lad = [("zeros", _lossy_nsf(1 + (i * 5) % 12)) for i in range(16)]
    add("ladder_16x3", "ladder", 44100, 2, None, lad, qualities=q4[:3])
    add("ladder_16x4", "ladder", 44100, 2, None, lad, qualities=q4)
    lad = [("zeros", _lossy_nsf(1 + (i * 5) % 4)) for i in range(256)]
    add("ladder_256x3", "ladder", 44100, 1, None, lad, qualities=q4[:3])
    add("ladder_256x4", "ladder", 44100, 1, None, lad, qualities=q4)
    # one lossless frame of 5,000,000 samples: cum * 1000 passes 2^32 at the second entry
    add("ll_5mhz_two_frames", "lossless", 5000000, 1, 5, [("zeros", 5000001)])
    return out


def tone_case():
    """256 lossy stereo clips of which 34 hold a short tone in the left channel, so their DATA lengths are odd or even as the
    coefficients fall. Not one of cases(): its files are not compared with the oracle's (see the module docstring)."""
    clips = [FOUND["lossy_stereo_16385"], FOUND["lossy_stereo_last63"]]
    clips += [("tone_left", 200 + 431 * i, 100 + 37 * i, 1024 * (1 + i % 9) + 13 * i) for i in range(32)]
    clips += [("zeros", _lossy_nsf(1 + (i * 29) % 70)) for i in range(256 - len(clips))]
    return dict(name="chain_stereo_256_tones", kind="lossy", sr=44100, ch=2, qol=0.55, clips=clips, qualities=None,
                variants=VARIANTS_CHAIN, pack=False)


def case(name):
    return next(c for c in cases() + [tone_case()] if c["name"] == name)


@functools.lru_cache(maxsize=None)
def pcm_of(name):
    c = case(name)
    return [make_pcm(s, c["ch"]) for s in c["clips"]]


@functools.lru_cache(maxsize=None)
def oracle_files(name):
    """the oracle's files of a case, computed once: [clip] bytes, for a ladder [rung][clip]"""
    c = case(name)
    cache = {}

    def enc(spec, pcm, q):
        key = (spec, q)       # (many clips of a case share a spec)
        if key not in cache:
            cache[key] = (O.encode_lossless(pcm, c["sr"], c["ch"], 16, q) if c["kind"] == "lossless"
                          else O.encode_lossy(pcm, c["sr"], c["ch"], q))
        return cache[key]
    if c["kind"] == "ladder":
        return [[enc(s, p, q) for s, p in zip(c["clips"], pcm_of(name))] for q in c["qualities"]]
    return [enc(s, p, c["qol"]) for s, p in zip(c["clips"], pcm_of(name))]


def batch_of(kind, ch, files, which=0, tail=True, rungs=1, n_clips=None):
    """What the finish sees for a batch whose finished files are `files` (rung-major for a ladder): the plan, the CRC
    makers and per file (DATA bytes, frames, samples per frame)."""
    parsed = [flofile.parse(f) for f in files]
    clips = [(p.data_size, len(p.frames), [fr.frame_samples for fr in p.frames]) for p in parsed]
    n = len(files) if n_clips is None else n_clips      # (n_clips: `files` is a sample of a larger batch)
    max_frames = max([c[1] for c in clips], default=0)
    form = lossy_form(which, ch, n // rungs) if kind == "lossy" else None
    crc_ready = kind == "lossy" and form == 5 and n >= K_FEW_CLIPS
    plan = plan_finish(n, max_frames, crc_ready)
    names = set()
    if plan["fused"]:
        makers = ["nt256"]
        names.add("maker:fused")
    elif crc_ready:
        makers = ["nt64"] if tail else ["nt256"]
        names.add("maker:tail" if tail else "maker:fallback_256")
        assert plan["parts"] <= FALLBACK_PARTS_MAX
    else:
        makers = ["nt256"]
        names.add("maker:crc_slices_form1" if kind == "lossy" and which == 1 else "maker:crc_slices")
    return dict(plan=plan, makers=makers, maker_names=names, clips=clips, max_frames=max_frames,
                rate=parsed[0].sample_rate if parsed else 0)


def batch_paths(b):
    """-> [set of names per file]"""
    return [clip_paths(b["plan"], n, nf, b["max_frames"], smp, b["rate"], b["makers"]) | b["maker_names"] for n, nf, smp in b["clips"]]


def case_batches(name):
    """the batches a case runs as (one per variant) -> [(variant, batch)]"""
    c = case(name)
    files = oracle_files(name)
    if c["kind"] == "ladder":
        flat = [f for rung in files for f in rung]
        return [("auto", batch_of("ladder", c["ch"], flat, rungs=len(files)))]
    out = []
    for v in c["variants"]:
        out.append((v, batch_of(c["kind"], c["ch"], files, which=1 if v == "form1" else 5 if v != "auto" else 0, tail=v != "fallback")))
    return out


def case_clip_paths(name):
    """-> [set of names per clip], over all variants (a ladder: per file, rung-major)"""
    per = None
    for _, b in case_batches(name):
        bp = batch_paths(b)
        per = bp if per is None else [a | x for a, x in zip(per, bp)]
    return per


def case_paths(name):
    return set().union(*case_clip_paths(name)) if case(name)["clips"] else set()
