"""Path model of the lossy encoder (tests only): which of the hidden paths of flo_amd/csrc/encode_plan.cpp and
lossy_kernels.hip an input takes, restated from the constants, and an independent writer of the frame bytes.

    constants      the thresholds the predicates use; test_lossy_model_cpu.py reads them out of the sources and compares
    plan_lossy     encode_plan.cpp restated, pinned to the rows of tests/native/encode_plan_test.cpp
    write_frames   integers [hops][ch][1024] + scale words [hops][ch][25] -> DATA bytes and frame sizes; it knows the byte
                   layout and nothing of items, blocks, run tables or staging buffers
    frame_paths    per frame: the packer form of each channel and why a form declined, pend, the flush, wide varints, dead
                   blocks, the size against kFrameCap
    batch_paths    per batch: the plan row, clips per workgroup, persistence, the scan blocks, the offset-scan paths
    spectra_cases  hand-made spectra that reach the packer paths, built so that every coefficient is far from its keep
                   threshold and every product far from a half-integer: the device's integers must equal the oracle's
    level_clips    the clips whose masking level does not decay (a band energy that overflows f32)
    geometry / dealing batches: lengths only; the GPU test makes the PCM
"""
import os
import re
import struct

import numpy as np

import psy_ref
import signals
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------------------------------------------- constants
kItemCap = 128            # item form: up to this many non-zeros
kRunTabEntries = 128      # block form: up to kRunTabEntries - 2 runs
kMaxRun = 255             # block form declines a longer run of non-zeros (continuation records)
kFrameCap = 4352
kRedealOffset = 2560      # the general form re-deals its integers through stage + 2560
kScanBlock = 64
kScanFetch = 16
kCompactChunk = 32
kFrontStride = 2048       # the fused kernel's front sum: 256 threads x 8 loads
kOffsetsKeep = 8          # frames per thread lossy_frame_offsets_kernel keeps in registers
kFewClips = 64
kFusedCompactClips = 16
kCoefHandoverBytes = 256 << 20
kDirty44k = 0xBDBE
kChain2qFill = 256        # clips per workgroup: ceil(n / 256) ...
kChain2qMaxClips = 6      # ... at most FLO_C2X_THREADS / 128
kAutoChainWaves = 512     # auto: n_clips * ch >= 512 takes the chain forms
MAX_BLOB = 2058           # the largest sparse blob of 1024 values (found below: the dense vector); kFrameCap's comment allows 2064


def source_constants():
    """the same constants as the sources state them"""
    def read(*p):
        with open(os.path.join(ROOT, "flo_amd", "csrc", *p)) as f:
            return f.read()
    dev, ker, hpp, cpp = read("lossy_device.hpp"), read("lossy_kernels.hip"), read("encode_plan.hpp"), read("encode_plan.cpp")

    def one(pat, text, base=0):
        m = re.findall(pat, text)
        assert len(set(m)) == 1, (pat, m)
        return int(m[0], base)
    c2x = one(r"#define FLO_C2X_THREADS (\d+)", ker)
    return dict(
        kItemCap=one(r"constexpr int kItemCap = (\d+);", dev),
        kRunTabEntries=one(r"constexpr int kRunTabEntries = (\d+);", dev),
        kMaxRun=one(r"act && cnt > (\d+)u", dev),
        kFrameCap=one(r"constexpr int kFrameCap = (\d+);", dev),
        kRedealOffset=one(r"stage \+ (\d+)\);", ker),
        kScanBlock=one(r"constexpr int kScanBlock = (\d+);", ker),
        kScanFetch=one(r"for \(unsigned h0 = fw; h0 < fe; h0 \+= (\d+)\)", ker),
        kCompactChunk=one(r"constexpr int kCompactChunk = (\d+);", ker),
        kFrontStride=one(r"hb < h0; hb \+= (\d+)u \* 8u\)", ker) * 8,
        kOffsetsKeep=one(r"uint32_t keep\[(\d+)\]", ker),
        kFewClips=one(r"constexpr size_t kFewClips = (\d+);", hpp),
        kFusedCompactClips=one(r"constexpr size_t kFusedCompactClips = (\d+);", hpp),
        kCoefHandoverBytes=one(r"kCoefHandoverBytes = \(size_t\)(\d+) << 20;", hpp) << 20,
        kDirty44k=one(r"constexpr uint32_t kDirty44k = (0x[0-9A-Fa-f]+)u;", hpp, 16),
        kChain2qFill=one(r"int chain2q_clips_per_wg\(int n_clips\) \{\s*int g = \(n_clips \+ 255\) / (\d+);", ker),
        kChain2qMaxClips=c2x // one(r"if \(g > FLO_C2X_THREADS / (\d+)\) g = FLO_C2X_THREADS / \d+;", ker),
        kAutoChainWaves=one(r"in\.n_clips \* in\.ch >= (\d+) \?", cpp),
    )


# ---------------------------------------------------------------------------------------------------- the plan
def lossy_form(which, force_path, ch, n_clips, exact=False, debug=False):
    if ch > 2:
        return 2
    w = which or force_path
    if not w:
        w = 1 if debug else ((5 if ch == 2 else 1) if n_clips * ch >= kAutoChainWaves else 2)
    if w in (3, 4):
        w = 5
    if w == 5 and (exact or ch != 2):
        w = 1
    return w


def plan_lossy(which=0, force_path=0, ch=2, n_clips=1, total_frames=0, exact=False, in_coeffs=False, debug=False,
               dirty=kDirty44k, tail=True):
    """-> the description tests/native/encode_plan_test.cpp prints for the same input"""
    form = lossy_form(which, force_path, ch, n_clips, exact, debug)
    if form == 5:
        k = "InCoeffs" if in_coeffs else "Debug" if debug else "Dirty44k" if (dirty | 0x8000) == kDirty44k else "Generic"
        ready = n_clips >= kFewClips
        return "chain2q:" + k + (" ready" if ready else "") + (" tail" if ready and tail else "")
    if form == 1:
        return "chain:" + ("Mono" if ch == 1 else "Stereo") + ("Exact" if exact else "")
    coef = ch == 2 and total_frames * 8192 <= kCoefHandoverBytes
    if ch == 1:
        p1, p2 = "Mono1", "Mono2Exact" if exact else "Mono2"
    elif ch == 2 and not exact and not in_coeffs:
        p1, p2 = "Pair1", "Pair2FromCoef" if coef else "Pair2"
    elif ch == 2:
        p1, p2 = "Stereo1", "Stereo2Exact" if exact else "Stereo2"
    else:
        p1, p2 = "Multi1", "Multi2Exact" if exact else "Multi2"
    compact = "Fused" if n_clips <= kFusedCompactClips else "Offsets1024" if n_clips < kFewClips else "Offsets256"
    return f"frames:{p1},{p2}" + (" coef" if coef else "") + (" scan" if p2 != "Pair2FromCoef" else "") + " " + compact


def chain2q_clips_per_wg(n_clips, override=0):
    if 1 <= override <= kChain2qMaxClips:
        return override
    return max(1, min((n_clips + kChain2qFill - 1) // kChain2qFill, kChain2qMaxClips))


# ---------------------------------------------------------------------------------------------------- the frame writer
def varint(v):
    out = bytearray()
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def sparse_records(q):
    """[(zero run, [values])] of one vector: a record is a run of zeros and the non-zeros behind it, at most 255 of them;
    zeros at the end are a record without values (encoder.rs:284-314)"""
    q = [int(x) for x in q]
    recs, i, n = [], 0, len(q)
    while i < n:
        z = 0
        while i < n and q[i] == 0:
            z, i = z + 1, i + 1
        vals = []
        while i < n and q[i] != 0 and len(vals) < 255:
            vals.append(q[i])
            i += 1
        recs.append((z, vals))
    return recs


def sparse_blob(q):
    out = bytearray()
    for z, vals in sparse_records(q):
        out += varint(z) + bytes([len(vals)]) + struct.pack("<%dh" % len(vals), *vals)
    return bytes(out)


def write_frame(q, sfw):
    """q [ch][1024], sfw [ch][25] -> the frame's bytes: 12 header bytes, 50 ch scale bytes, per channel length + blob"""
    nch = len(q)
    blobs = [sparse_blob(q[c]) for c in range(nch)]
    body = bytes([0, nch]) + b"".join(struct.pack("<25H", *[int(x) for x in sfw[c]]) for c in range(nch))
    body += b"".join(struct.pack("<I", len(b)) + b for b in blobs)
    return struct.pack("<BIB", 253, 1024, 0) + struct.pack("<I", len(body)) + body


def write_frames(q, sfw):
    """-> (DATA bytes, [frame sizes])"""
    frames = [write_frame(q[h], sfw[h]) for h in range(len(q))]
    return b"".join(frames), [len(f) for f in frames]


def split_frames(data, nch):
    """DATA of a lossy clip -> [(frame bytes, [blob per channel])], walking the length words"""
    out, p = [], 0
    while p < len(data):
        assert data[p] == 253 and data[p + 10] == 0 and data[p + 11] == nch, (p, data[p:p + 12])
        blen = struct.unpack_from("<I", data, p + 6)[0]
        end = p + 10 + blen
        c, blobs = p + 12 + 50 * nch, []
        for _ in range(nch):
            ln = struct.unpack_from("<I", data, c)[0]
            blobs.append(data[c + 4:c + 4 + ln])
            c += 4 + ln
        assert c == end, (p, c, end)
        out.append((data[p:end], blobs))
        p = end
    return out


EMPTY_BLOB = b"\x80\x08\x00"   # 1024 zeros


# ---------------------------------------------------------------------------------------------------- packer paths
def channel_form(q):
    """-> (form, reasons): the form the packer wave ends in and what made the forms in front of it decline"""
    q = np.asarray(q)
    nz = q != 0
    n = int(nz.sum())
    if n <= kItemCap:
        return "item", []
    reasons = ["nz_gt_itemcap"]
    d = np.diff(np.concatenate(([0], nz.astype(np.int8), [0])))
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    runs, longest = len(starts), int((ends - starts).max())
    if runs > kRunTabEntries - 2:
        reasons.append("runs_gt_126")
    if longest > kMaxRun:
        reasons.append("run_gt_255")
    return ("general" if len(reasons) > 1 else "block"), reasons


def band_blocks(sample_rate):
    """[8] bit masks: the bands with a bin in each block of 128 positions"""
    band = O.psy_tables(sample_rate)[1].astype(np.int64)
    return [int(np.bitwise_or.reduce(1 << band[128 * k:128 * k + 128])) for k in range(8)]


def frame_paths(q, sizes, sample_rate):
    """q [hops][2][1024] (the integers of a stereo clip), sizes: the frames' sizes -> [set of path names] per frame"""
    q = np.asarray(q)
    band = O.psy_tables(sample_rate)[1].astype(np.int64)
    blocks = band_blocks(sample_rate)
    out, pend = [], 0
    for h in range(q.shape[0]):
        p = set()
        forms = []
        for c in range(2):
            f, why = channel_form(q[h, c])
            forms.append(f)
            p.add(f"form:ch{c}_{f}")
            p.update(f"decline:{w}" for w in why)
            n = int((q[h, c] != 0).sum())
            if n in (0, 1, 63, 64, 65, 127, 128, 129):
                p.add(f"nz:{n}")
            recs = sparse_records(q[h, c])
            for i, (z, vals) in enumerate(recs):
                where = "front" if i == 0 else "behind" if not vals else "between"
                if z in (127, 128, 129):
                    p.add(f"zrun:{where}_{z}")
                if z >= 128:
                    p.add("varint:wide")
            if q[h, c, 0] != 0:
                p.add("run:starts_on_0")
            if q[h, c, 1023] != 0:
                p.add("run:ends_on_1023")
            d = np.diff(np.concatenate(([0], (q[h, c] != 0).astype(np.int8), [0])))
            lens = np.flatnonzero(d == -1) - np.flatnonzero(d == 1)
            for L in (255, 256, 510, 511):
                if (lens == L).any():
                    p.add(f"run:{L}")
            if len(lens) in (126, 127):
                p.add(f"runs:{len(lens)}_{'le' if n <= kItemCap else 'gt'}_itemcap")
        p.add(f"pair:{forms[0]}_{forms[1]}")
        if forms[1] == "general":
            blob0 = len(sparse_blob(q[h, 0]))
            if blob0 >= 2050:
                p.add("redeal:behind_largest_channel0")
                if pend == 15:
                    p.add("redeal:behind_largest_channel0_pend15")
            if blob0 == MAX_BLOB:
                p.add("redeal:behind_dense_channel0")
        alive = 0
        for c in range(2):
            for b in np.unique(band[q[h, c] != 0]):
                alive |= 1 << int(b)
        dead = [k for k in range(8) if not (alive & blocks[k])]
        if len(dead) == 8:
            p.add("blocks:all_dead")
        elif dead == list(range(1, 8)):
            p.add("blocks:only_0_alive")
        elif dead == list(range(7)):
            p.add("blocks:only_7_alive")
        if bin(alive).count("1") == 1:
            b = alive.bit_length() - 1
            if sum(1 for k in range(8) if blocks[k] >> b & 1) > 1:
                p.add(f"blocks:one_band_straddles_{sample_rate}_b{b}")
        p.add(f"pend:{pend}")
        if (pend + sizes[h]) % 16 == 0:
            p.add("flush:ends_on_boundary")
        if sizes[h] >= 4000:
            p.add("size:near_framecap")
        assert pend + sizes[h] <= kFrameCap and sizes[h] <= 120 + 2 * MAX_BLOB
        pend = (pend + sizes[h]) % 16
        out.append(p)
    if q.shape[0] and pend == 0:
        out[-1].add("flush:data_multiple_of_16")
    return out


# ---------------------------------------------------------------------------------------------------- batch paths
def hops_of(n_sample_frames):
    return (n_sample_frames + 1024 + 1023) // 1024


def batch_paths(ch, lens, which=0, n_cus=256, clips_override=0, exact=False):
    """lens: sample-frames per clip -> set of path names of the batch's encode under form `which` (0: auto)"""
    n = len(lens)
    hops = [hops_of(x) for x in lens]
    plan = plan_lossy(which=which, ch=ch, n_clips=n, total_frames=sum(hops), exact=exact)
    p = {"plan:" + plan.split(" ")[0]}
    if plan.startswith("chain2q"):
        g = chain2q_clips_per_wg(n, clips_override)
        p.add(f"deal:g{g}")
        wgs = (n + g - 1) // g
        if wgs > n_cus:
            p.update({"deal:persistent", "deal:slot_takes_a_second_clip"})
            if any(h & 1 for h in hops) and any(not h & 1 for h in hops):
                p.add("deal:table_parity_flips_between_clips")
        if min(wgs, n_cus) * g > n:
            p.add("deal:pair_whose_first_claim_fails")
    if plan.startswith("frames"):
        p.add("compact:" + plan.split(" ")[-1])
        fromcoef = "Pair2FromCoef" in plan
        for h in hops:
            if fromcoef:
                p.add("walk:h_lt_64")
                if h > kScanBlock:
                    p.add("walk:h_eq_64")
                if h > kScanBlock + 1:
                    p.add("walk:h_gt_64")
            else:
                nb = (h + kScanBlock - 1) // kScanBlock
                p.add(f"scan:blocks_{min(nb, 3)}{'plus' if nb >= 3 else ''}")
                if nb >= 3:
                    p.add("scan:warm_up_starts_behind_frame_0")
                if h % kScanFetch:
                    p.add("scan:fetch_group_cut_short")
                if h % kScanBlock == 0:
                    p.add("scan:last_block_full")
                if h % kScanBlock == 1:
                    p.add("scan:last_block_one_frame")
            if plan.endswith("Fused"):
                if h <= kCompactChunk:
                    p.add("fused:one_chunk")
                if h % kCompactChunk == 0:
                    p.add("fused:last_chunk_full")
                if h % kCompactChunk == 1:
                    p.add("fused:last_chunk_one_frame")
                if h > kFrontStride + kCompactChunk:
                    p.add("fused:front_sum_second_stride")
            else:
                t = 1024 if plan.endswith("Offsets1024") else 256
                per = (h + t - 1) // t
                p.add(f"off{t}:per_{'1' if per <= 1 else 'le8' if per <= kOffsetsKeep else 'gt8'}")
        if ch > 2:
            p.add(f"multi:ch{ch}")
    return p


# ---------------------------------------------------------------------------------------------------- hand-made spectra
AMP = np.float32(1e5)     # 100 dB: above the hearing threshold of every bin (96 dB at most), so every kept coefficient has
                          # an SMR of ~14 dB or more against a keep threshold of -19.75 dB at quality 0.55


def _spectrum(frames, nch=2):
    """frames: [[positions of channel c, ...], ...] -> coeffs [hops][ch][1024]: AMP at the positions, the sign and one of
    two sizes by position (30000 and 22500 after scaling: far from a half-integer), zero elsewhere"""
    c = np.zeros((len(frames), nch, 1024), np.float32)
    for h, chans in enumerate(frames):
        for ch, pos in enumerate(chans):
            pos = np.asarray(sorted(set(int(x) for x in pos)), np.int64)
            if pos.size:
                assert pos.min() >= 0 and pos.max() < 1024
                v = np.where(pos % 5 == 2, np.float32(0.75), np.float32(1.0)) * np.where((pos + h) % 3 == 0, -1.0, 1.0)
                c[h, ch, pos] = (AMP * v).astype(np.float32)
    return c


def _singles(n, step=7, start=3):
    return [start + step * i for i in range(n)]


def _run(start, n):
    return list(range(start, start + n))


def _runs(n_runs, length, gap=1, start=0):
    return [start + r * (length + gap) + i for r in range(n_runs) for i in range(length)]


def spectra_cases():
    """-> [(name, coeffs [hops][2][1024], sample_rate, quality)]"""
    out = []
    sr, q = 44100, 0.55

    def add(name, frames, rate=sr):
        out.append((name, _spectrum(frames), rate, q))
    # non-zeros per channel: single positions in channel 0 (as many runs), one run in channel 1
    add("nz_0_1_63_64", [[_singles(n), _run(500, n)] for n in (0, 1, 63, 64)])
    add("nz_65_127_128_129", [[_singles(n), _run(500, n)] for n in (65, 127, 128, 129)])
    # 126 and 127 runs: of one value (item form) and of two (block form; 127 runs: general)
    add("runs_126_127", [[_runs(r, 1, 1, 2), _runs(r, 2, 1, 5)] for r in (126, 127)])
    add("runs_126_127_long", [[_runs(r, 3, 2, 1), _runs(r, 1, 3, 0) + _run(700, 40)] for r in (126, 127)])
    # one long run: from position 0 in channel 0, up to position 1023 in channel 1
    add("run_255_256_510_511", [[_run(0, L), _run(1024 - L, L)] for L in (255, 256, 510, 511)])
    add("run_255_256_inside", [[_run(40, L) + _singles(5, 9, 900), _run(300, L)] for L in (255, 256)])
    # zero runs of 127, 128, 129 in front of, between and behind the items (channel 0) and the runs of a block form (channel 1)
    add("zero_runs_127_128_129", [[[z, 2 * z + 1, 1023 - z],
                                   _run(z, 130) + _run(2 * z + 130, 10) + _run(1000 - z, 24)] for z in (127, 128, 129)])
    # the nine (channel 0, channel 1) pairs of forms
    forms = {"item": _singles(10, 31, 7), "block": _run(100, 200) + _singles(6, 50, 600), "general": _run(90, 300) + _run(500, 9)}
    for f0 in forms:
        add(f"pair_{f0}_x", [[forms[f0], forms[f1]] for f1 in forms])
    # the largest blobs: alternating positions (2050 bytes) and the dense vector (2058), a general-form channel 1 behind
    # them, with 15 bytes pending from the frame in front (143 bytes: 120 + [130 zeros][7 values][887 zeros] + 1024 zeros)
    lead = [_run(130, 7), []]
    add("largest_alternating_pend15", [lead, [list(range(0, 1024, 2)), _run(0, 1024)], [_run(3, 5), _run(1, 2)]])
    add("largest_dense_pend15", [lead, [_run(0, 1024), _run(0, 1024)], [_run(3, 5), _run(1, 2)]])
    add("largest_dense_alternating_odd", [lead, [_run(0, 1024), list(range(1, 1024, 2))], [[], [1023]]])
    # sixteen frames of 161 bytes = 16 * 10 + 1: pend walks 0, 1, ... 15, the last flush ends on a boundary and DATA is 2576 bytes
    add("pend_walk_16", [[_run(130 + 3 * h, 8), _run(h % 3, 7)] for h in range(16)])
    # one band alive, for each band that lies on both sides of a block edge; block 0 only, block 7 only, nothing
    for rate in (44100, 48000):
        band = O.psy_tables(rate)[1].astype(np.int64)
        strad = sorted({int(band[128 * k]) for k in range(1, 8) if band[128 * k] == band[128 * k - 1]})
        fr = [[list(np.flatnonzero(band == b)), []] if i % 2 == 0 else [[], list(np.flatnonzero(band == b))] for i, b in enumerate(strad)]
        for i in range(0, len(fr), 3):
            add(f"one_band_{rate}_{i // 3}", fr[i:i + 3], rate)
    add("blocks_0_none", [[_run(4, 20), _singles(4, 30, 2)], [[], []], [_run(900, 30), []]])
    # block 7 alone: at 44.1 kHz band 24 reaches from block 5 to block 7, at 8 kHz band 17 (3700 Hz up) lies inside block 7
    add("block_7_only_8000", [[[], _run(960, 64)], [_run(950, 30), []], [[], []]], 8000)
    return out


def spectra_cases_other_channels():
    """mono and three channels: under form 2 the stage entry runs lossy_frame_kernel<1, ., .> and lossy_frame_n_kernel (form 1,
    mono: lossy_chain_kernel<1, .>); the three forms of the packer and a pending-byte walk in each"""
    sr, q = 44100, 0.55
    forms = [_singles(10, 31, 7), _run(100, 200) + _singles(6, 50, 600), _run(90, 300) + _run(500, 9), _run(130, 8), []]
    mono = _spectrum([[f] for f in forms], 1)
    three = _spectrum([[forms[(h + c) % 5] for c in range(3)] for h in range(5)], 3)
    return [("mono_item_block_general", mono, sr, q), ("three_channels_item_block_general", three, sr, q)]


def levels_spectra_case():
    """band 2 of channel 0 at the largest level an f32 band energy holds (all of its bins at 1.8e19: the sum of squares stays
    below 3.4e38), 70 silent frames, then a probe frame of ordinary size in every band: whatever is left of the loud frame's level
    after 71 frames decides nothing. Channel 1 carries the probe frame alone."""
    sr = 44100
    band = O.psy_tables(sr)[1].astype(np.int64)
    c = np.zeros((72, 2, 1024), np.float32)
    k = np.flatnonzero(band == 2)
    c[0, 0, k] = np.float32(1.8e19 / np.sqrt(k.size)) * np.where(np.arange(k.size) % 2, -1.0, 1.0).astype(np.float32)
    probe = _spectrum([[_singles(100, 9, 4), _singles(100, 9, 4)]])[0]
    c[71] = probe
    return ("largest_finite_level_then_70_silent", c, sr, 0.55)


def margins(coeffs, sr, q):
    """-> (smallest |margin| in dB over all coefficients, smallest distance of a kept product c * sf from a half-integer)"""
    m = psy_ref.model(coeffs, sr, q)
    mg = m["margin"]
    assert np.isfinite(mg).all()
    prod = (np.asarray(coeffs, np.float32) * m["sf"][..., m["band"]]).astype(np.float64)
    kept = mg > 0
    frac = np.abs(prod[kept] - np.floor(prod[kept]) - 0.5)
    return float(np.abs(mg).min()), float(frac.min()) if kept.any() else 0.5


# ---------------------------------------------------------------------------------------------------- levels that do not decay
LEVEL_FRAMES = 220
LEVEL_VALUES = [("3e38", 3e38, 2), ("2e19", 2e19, 2), ("+inf", np.inf, 2), ("-inf", -np.inf, 2), ("nan", np.nan, 2),
                ("3e38_f70", 3e38, 70), ("3e38_f150", 3e38, 150)]


def level_clip(ch, value, frame):
    """music_like(44100, 1024 * 220, ch, seed=5) with one sample of channel 0 replaced: sample-frame 3000 for frame 2,
    1024 further per frame"""
    x = signals.music_like(44100, 1024 * LEVEL_FRAMES, ch, seed=5).copy()
    if value is not None:       # (None: the clip as it is)
        x[(3000 + 1024 * (frame - 2)) * ch] = np.float32(value)
    return x


def level_cases():
    return [(f"{name}_ch{ch}", ch, v, f) for ch in (1, 2) for name, v, f in LEVEL_VALUES]


def oracle_empty_pattern(pcm, ch):
    """[hops][ch] bool: the oracle's integers of that frame and channel are all zero"""
    o = O.lossy_analyze(pcm, 44100, ch, 0.55)
    return (o["q"] == 0).all(axis=2)


# ---------------------------------------------------------------------------------------------------- batches by length
RAGGED = [0, 1, 1023, 1024, 1025, 2048, 3000, 4100]


def tone_burst(n, ch, i):
    """a short clip that differs from clip to clip: a tone whose frequency and level come from i"""
    t = np.arange(n, dtype=np.float64) / 44100.0
    x = (0.05 + 0.02 * (i % 7)) * np.sin(2 * np.pi * (200.0 + 37.0 * (i % 101)) * t + 0.1 * i)
    out = np.repeat(x[:, None], ch, axis=1)
    if ch > 1:
        out[:, 1] *= 0.5 + 0.05 * (i % 5)
    return np.ascontiguousarray(out, np.float32).reshape(-1)


def ragged_clip(n, ch, i):
    return signals.music_like(44100, n, ch, seed=900 + i) if i % 8 in (3, 5) and i < 16 else tone_burst(n, ch, i)


def dealing_batches(n_cus=256):
    """-> [(name, channels, lens, which, clips override)]"""
    big = 2048 if n_cus == 256 else 6 * n_cus + 1 + (-(6 * n_cus + 1)) % 8
    out = [(f"ragged_{big}_g{g}" if g else f"ragged_{big}", 2, [RAGGED[i % 8] for i in range(big)], 5, g) for g in range(0, 7)]
    for n in (1, 2, 255, 256, 257, 512, 513, 1281):
        out.append((f"stereo_{n}", 2, [RAGGED[(i + 1) % 8] for i in range(n)], 5, 0))
    for ch, n in ((1, 511), (1, 512), (2, 255), (2, 256)):
        out.append((f"auto_ch{ch}_{n}", ch, [RAGGED[(i + 3) % 8] for i in range(n)], 0, 0))
    return out


def geometry_batches():
    """-> [(name, channels, lens)] for form 2 against form 1; frames f -> (f - 1) * 1024 - 100 sample-frames, plus a residue"""
    def nsf(frames, r=0):
        return (frames - 1) * 1024 - 100 + r
    out = [("scan_blocks", 2, [nsf(f, i) for i, f in enumerate((63, 64, 65, 127, 128, 129, 130, 200))])]
    out.append(("scan_blocks_mono", 1, [nsf(f, i) for i, f in enumerate((63, 64, 65, 127, 128, 129, 130, 200))]))
    for n in (16, 17, 63, 64):
        out.append((f"compact_{n}_clips", 2, [nsf(2 + i % 5, i) for i in range(n)]))
    for f in (31, 32, 33, 2081, 2100):
        out.append((f"fused_{f}_frames", 2, [nsf(f, f & 3)]))
    for f in (2049, 2100):
        out.append((f"off256_{f}_frames", 2, [nsf(3 + i % 3, i) for i in range(63)] + [nsf(f)]))
    out.append(("off256_600_frames", 2, [nsf(3 + i % 3, i) for i in range(63)] + [nsf(600)]))      # 3 frames per thread
    out.append(("off1024_1100_frames", 2, [nsf(2 + i % 3, i) for i in range(16)] + [nsf(1100)]))   # 2 frames per thread
    for f in (8193, 8200):
        out.append((f"off1024_{f}_frames", 2, [nsf(2 + i % 3, i) for i in range(16)] + [nsf(f)]))
    for ch in (4, 5, 7):
        out.append((f"multi_ch{ch}", ch, [nsf(3, 1), nsf(66, 2), nsf(2, 3)]))
    return out


def geometry_clip(n, ch, i):
    """silence with three tone bursts (long clips: the oracle is not needed, the forms are compared with each other)"""
    x = np.zeros((n, ch), np.float32)
    for j, at in enumerate((0.1, 0.5, 0.9)):
        a = int(at * max(n - 3000, 0))
        m = min(3000, n - a)
        if m > 0:
            x[a:a + m] = tone_burst(m, ch, 3 * i + j).reshape(m, ch)
    return x.reshape(-1)


HANDOVER_FRAMES = (32768, 32769)      # the coefficient hand-over's last and first-without


# ---------------------------------------------------------------------------------------------------- the path lists
PACKER_PATHS = (
    [f"form:ch{c}_{f}" for c in (0, 1) for f in ("item", "block", "general")] +
    [f"pair:{a}_{b}" for a in ("item", "block", "general") for b in ("item", "block", "general")] +
    ["decline:nz_gt_itemcap", "decline:runs_gt_126", "decline:run_gt_255"] +
    [f"nz:{n}" for n in (0, 1, 63, 64, 65, 127, 128, 129)] +
    ["runs:126_le_itemcap", "runs:127_le_itemcap", "runs:126_gt_itemcap", "runs:127_gt_itemcap"] +
    [f"run:{L}" for L in (255, 256, 510, 511)] + ["run:starts_on_0", "run:ends_on_1023"] +
    [f"zrun:{w}_{z}" for w in ("front", "between", "behind") for z in (127, 128, 129)] + ["varint:wide"] +
    ["redeal:behind_largest_channel0", "redeal:behind_largest_channel0_pend15", "redeal:behind_dense_channel0"] +
    [f"pend:{i}" for i in range(16)] + ["flush:ends_on_boundary", "flush:data_multiple_of_16", "size:near_framecap"] +
    ["blocks:all_dead", "blocks:only_0_alive", "blocks:only_7_alive"] +
    [f"blocks:one_band_straddles_44100_b{b}" for b in (15, 19, 21, 22, 23, 24)] +
    [f"blocks:one_band_straddles_48000_b{b}" for b in (15, 19, 21, 23, 24)] +
    ["packer:take_next_behind_quantiser", "packer:take_next_between_channels", "packer:take_next_before_flush"])
BATCH_PATHS = (
    ["plan:chain2q:Dirty44k", "plan:chain:Mono", "plan:chain:Stereo", "plan:frames:Mono1,Mono2", "plan:frames:Pair1,Pair2FromCoef",
     "plan:frames:Pair1,Pair2", "plan:frames:Multi1,Multi2"] +
    [f"deal:g{g}" for g in range(1, 7)] +
    ["deal:persistent", "deal:slot_takes_a_second_clip", "deal:table_parity_flips_between_clips", "deal:pair_whose_first_claim_fails"] +
    ["compact:Fused", "compact:Offsets1024", "compact:Offsets256"] +
    ["walk:h_lt_64", "walk:h_eq_64", "walk:h_gt_64"] +
    ["scan:blocks_1", "scan:blocks_2", "scan:blocks_3plus", "scan:warm_up_starts_behind_frame_0", "scan:fetch_group_cut_short",
     "scan:last_block_full", "scan:last_block_one_frame"] +
    ["fused:one_chunk", "fused:last_chunk_full", "fused:last_chunk_one_frame", "fused:front_sum_second_stride"] +
    ["off256:per_1", "off256:per_le8", "off256:per_gt8", "off1024:per_1", "off1024:per_le8", "off1024:per_gt8"] +
    ["multi:ch4", "multi:ch5", "multi:ch7"] +
    ["stage:mono_spectra_form1", "stage:mono_spectra_form2", "stage:three_channel_spectra"])
PATHS = PACKER_PATHS + BATCH_PATHS
NOT_REACHED_ALLOWED = {
    "packer:take_next_behind_quantiser": "timing: whether the transform wave has the next frame ready cannot be forced from outside",
    "packer:take_next_between_channels": "timing, as above",
    "packer:take_next_before_flush": "timing, as above",
}


def spectra_reach():
    """{path: [case names]} over the spectra cases, by the oracle's integers and the writer's sizes"""
    table = {}
    for name, c, sr, q in spectra_cases():
        o = O.lossy_quantize(c, sr, q)
        _, sizes = write_frames(o["q"], o["sf_words"])
        for p in set().union(*frame_paths(o["q"], sizes, sr)):
            table.setdefault(p, []).append(name)
    return table


def batch_reach(n_cus=256):
    table = {}
    for name, ch, lens, which, g in dealing_batches(n_cus):
        for p in batch_paths(ch, lens, which, n_cus, g):
            table.setdefault(p, []).append(name)
    for name, ch, lens in geometry_batches():
        for which in (1, 2):
            for p in batch_paths(ch, lens, which, n_cus):
                table.setdefault(p, []).append(name)
    for f in HANDOVER_FRAMES:
        for p in batch_paths(2, [(f - 1) * 1024 - 7], 2, n_cus):
            table.setdefault(p, []).append(f"handover_{f}")
    for name, c, sr, q in spectra_cases_other_channels():       # through the stage entry point, forms 1 and 2
        for p in (["stage:mono_spectra_form1", "stage:mono_spectra_form2"] if c.shape[1] == 1 else ["stage:three_channel_spectra"]):
            table.setdefault(p, []).append(name)
    return table
