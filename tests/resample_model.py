"""A model of what sample-rate conversion decides on the device (flo_amd/csrc/resample_plan.cpp, resample_kernels.hip),
restated in plain Python, the exact reference of its arithmetic, and the case table of tests/test_gpu_resample_paths.py.

* plan(): resample_plan() field for field (tests/test_resample_model_cpu.py pins it to the native dump on a grid of rate
  pairs), n_out_of(), tiles_of(), lane_of(): where an output is made (tile, unit, lane, slot, phase, row).
* paths(): the predicates over a launch - the kernel variant, phases per wave, idle lanes, chunks, the block's tail, how
  far a lane's windows lie apart, the LDS swizzle, the tiles of every clip, the shape of the batch - as a set of
  "name=value" strings, the vocabulary of PATHS; value_paths() adds what a clip's samples reach. Every value of PATHS
  must be reached by a case, or be named in NOT_REACHED_ALLOWED with the reason.
* fma(), chain(): the contract of the kernel's header, exactly: every output is fma(h[p][k], x[..], acc) for k = 0 .. T - 1
  in that order from acc = 0, in f32. dot_reference() is the f64 dot product and its bound, the second reference.
* cases(): the batches, each clip a few tiles at the most.
"""
import math

import numpy as np

# ---- constants restated from resample_plan.hpp (test_resample_model_cpu.py reads them there) --------------------------
LDS_BYTES = 80 * 1024     # kResampleLdsBytes
BLOCK = 4                 # kResampleBlock
TARGET_UNITS = 128        # kResampleTargetUnits
THREADS = 512             # kResampleThreads
FRAME_BYTES = 8           # kResampleFrameBytes
MAX_RATE, MAX_PHASES, MAX_TAPS, MAX_TABLE_BYTES = 384000, 1024, 2048, 1 << 20


def lds_index(f, shift):
    return f + (f >> shift)


def span_of(L, M, taps, q):
    return min((q - 1) * M + (L - 1) * M // L + taps, 0x7FFFFFFF)


def _plane_bytes(L, M, taps, shift, q):
    return (lds_index(span_of(L, M, taps, q) - 1, shift) + 1) * FRAME_BYTES


def plan(in_rate, out_rate):
    """resample_plan(), expression for expression: a dict of its fields, or the word its message names for a rejected pair"""
    if in_rate < 1 or in_rate > MAX_RATE:
        return "in_rate"
    if out_rate < 1 or out_rate > MAX_RATE:
        return "out_rate"
    g = math.gcd(in_rate, out_rate)
    L, M = out_rate // g, in_rate // g
    if L > MAX_PHASES:
        return "L"
    half = 32 if L >= M else (32 * M + L - 1) // L
    if 2 * half > MAX_TAPS:
        return "taps"
    T = 2 * half
    if L * T * 4 > MAX_TABLE_BYTES:
        return "table"
    shift = 31 if M & 1 else (M & -M).bit_length() - 1
    q = 64 * ((TARGET_UNITS + L - 1) // L)
    if _plane_bytes(L, M, T, shift, q) > LDS_BYTES:
        lo, hi = 0, q
        while hi - lo > 1:
            mid = lo + (hi - lo) // 2
            if _plane_bytes(L, M, T, shift, mid) <= LDS_BYTES:
                lo = mid
            else:
                hi = mid
        q = lo
    if q == 0:
        return "LDS"
    if q > 64:
        q -= q % 64
    if q <= 32:
        best = q
        for t in range(q, q // 2, -1):
            if (64 // t) * t > (64 // best) * best:
                best = t
        q = best
    lanes = min(q, 64)
    ppw = 64 // lanes
    chunks = (q + 63) // 64
    block = BLOCK if ppw == 1 else 1
    span = span_of(L, M, T, q)
    return dict(in_rate=in_rate, out_rate=out_rate, L=L, M=M, taps=T, shift=shift, slots=q, lanes_per_phase=lanes, phases_per_wave=ppw,
                chunks=chunks, block=block, units=chunks * ((L + ppw * block - 1) // (ppw * block)), span=span,
                lds_elems=lds_index(span - 1, shift) + 1, tile_outputs=q * L)


DUMP_FIELDS = ("L", "M", "taps", "shift", "slots", "lanes_per_phase", "phases_per_wave", "chunks", "block", "units", "span", "lds_elems",
               "tile_outputs")


def n_out_of(P, n_in):
    return -((-n_in * P["L"]) // P["M"])


def n_in_for(P, n_out):
    """the fewest input frames that give at least n_out outputs (an upsampler's counts skip values: the next one above)"""
    return 0 if n_out <= 0 else ((n_out - 1) * P["M"]) // P["L"] + 1


def tiles_of(P, n_out):
    return (n_out + P["tile_outputs"] - 1) // P["tile_outputs"]


def phase_of(P, r):
    """resample_phase: (e0, p) of phase index r"""
    return (r * P["M"]) // P["L"], (r * P["M"]) % P["L"]


def lane_of(P, j):
    """where output frame j of a clip is made: tile, wave-unit, lane, slot q, phase index r, block member i, row p"""
    L, ppw, lanes, block, chunks = P["L"], P["phases_per_wave"], P["lanes_per_phase"], P["block"], P["chunks"]
    tile, w = divmod(j, P["tile_outputs"])
    q, r = divmod(w, L)
    rb, grp = divmod(r // block, ppw)
    return dict(tile=tile, unit=rb * chunks + q // 64, lane=grp * lanes + q % 64, slot=q, phase=r, member=r % block, row=(r * P["M"]) % L)


def tile_span(P, t):
    """(start, end) of the clip's frames tile t stages: start may be negative, end may lie beyond the clip"""
    i0 = (t * P["tile_outputs"] * P["M"]) // P["L"]
    start = i0 - (P["taps"] // 2 - 1)
    return start, start + P["span"]


# ---- paths -----------------------------------------------------------------------------------------------------------------
PLANE_CHANNELS = (1, 3, 4, 5, 6, 7, 8)
PATHS = {
    "variant": ["variant=stereo_uniform", "variant=stereo_side", "variant=plane_uniform", "variant=plane_side"],
    "planes": ["plane_uniform_channels=%d" % c for c in PLANE_CHANNELS] + ["plane_side_channels=%d" % c for c in PLANE_CHANNELS] +
              ["plane_uniform_pass=two_planes", "plane_side_pass=two_planes", "plane_uniform_last_pass=one_plane_behind_pairs",
               "plane_side_last_pass=one_plane_behind_pairs"],
    "phases_per_wave": ["phases_per_wave=%d" % v for v in (1, 2, 4, 8, 16, 32, 64)],
    "idle_lanes": ["uniform_idle_lanes=0", "uniform_idle_lanes=2", "uniform_idle_lanes=3", "uniform_idle_lanes=31", "uniform_idle_lanes=other"],
    "chunks": ["chunks=1", "chunks=over_1"],
    "block": ["uniform_L_mod_4=0", "uniform_L_mod_4=1", "uniform_L_mod_4=2", "uniform_L_mod_4=3", "uniform_L=1", "uniform_L=2", "uniform_L=3",
              "uniform_L=5", "store=run_of_4", "store=singles_run_straddles_n_out", "store=singles_block_past_L"],
    "windows": ["windows=all_on_one_frame", "windows=one_frame_apart", "windows=24_or_more_apart"],
    "filter": ["L=1024", "taps=64", "taps=2048", "M_over_L=above_5", "upsampler", "downsampler"],
    "swizzle": ["shift=31", "shift=1", "shift=2_to_6", "shift=7_or_more"],
    "clip": ["clip=empty", "clip=n_in_1", "clip=single_output", "clip=exact_tiles", "clip=exact_tiles_plus_1", "clip=exact_tiles_minus_1",
             "tile=first_starts_before_0", "tile=middle_span_inside_clip", "tile=last_ends_beyond_clip", "tile=last_ends_inside_clip"],
    "batch": ["batch=one_clip", "batch=over_512_clips", "batch=empty_run_front", "batch=empty_run_middle", "batch=empty_run_end",
              "batch=stereo_odd_interleaved_middle"],
    "values": ["value=nan_first_frame", "value=nan_last_frame", "value=nan_shared_halo", "value=inf_first_frame", "value=inf_last_frame",
               "value=inf_shared_halo", "value=negative_zero_clip", "value=denormal_clip"],
}
# paths no case reaches, each with the reason
NOT_REACHED_ALLOWED = {
    "tile=last_ends_inside_clip": "the last tile holds output n_out - 1, whose last tap reads frame i + T/2, i = floor((n_out - 1) M / L). "
                                  "n_out >= n_in L / M gives i > n_in - M / L - 1, and T/2 >= 32 max(1, M / L), so that frame lies "
                                  "beyond n_in - 1 + 30: the span of a clip's last tile always ends in the zero padding",
}


def paths(in_rate, out_rate, channels, clip_lengths):
    """the named paths a launch over clips of clip_lengths interleaved samples reaches, by geometry alone"""
    P = plan(in_rate, out_rate)
    assert isinstance(P, dict), (in_rate, out_rate, P)
    L, M, T, Q, ppw = P["L"], P["M"], P["taps"], P["slots"], P["phases_per_wave"]
    uniform, stereo = ppw == 1, channels == 2
    kind = "uniform" if uniform else "side"
    p = {"variant=%s_%s" % ("stereo" if stereo else "plane", kind), "phases_per_wave=%d" % ppw}
    if not stereo:
        p.add("plane_%s_channels=%d" % (kind, channels))
        if channels >= 2:
            p.add("plane_%s_pass=two_planes" % kind)
        if channels >= 3 and channels % 2:
            p.add("plane_%s_last_pass=one_plane_behind_pairs" % kind)
    p.add("chunks=1" if P["chunks"] == 1 else "chunks=over_1")
    if uniform:
        idle = (64 - Q % 64) % 64
        p.add("uniform_idle_lanes=%d" % idle if idle in (0, 2, 3, 31) else "uniform_idle_lanes=other")
        p.add("uniform_L_mod_4=%d" % (L % 4))
        if L in (1, 2, 3, 5):
            p.add("uniform_L=%d" % L)
        for r0 in range(0, L, BLOCK):
            e = [phase_of(P, r)[0] for r in range(r0, min(L, r0 + BLOCK))]
            steps = [b - a for a, b in zip(e, e[1:])]
            if len(e) == BLOCK and e[-1] == e[0]:
                p.add("windows=all_on_one_frame")
            if len(e) == BLOCK and all(s == 1 for s in steps):
                p.add("windows=one_frame_apart")
            if steps and max(steps) >= 24:
                p.add("windows=24_or_more_apart")
    if L == 1024:
        p.add("L=1024")
    if T in (64, 2048):
        p.add("taps=%d" % T)
    if M > 5 * L:
        p.add("M_over_L=above_5")
    p.add("upsampler" if L > M else "downsampler")
    s = P["shift"]
    p.add("shift=31" if s == 31 else "shift=1" if s == 1 else "shift=2_to_6" if s <= 6 else "shift=7_or_more")
    has = []
    for n_il in clip_lengths:
        n_in = n_il // channels
        n_out = n_out_of(P, n_in)
        has.append(n_out > 0)
        p |= clip_paths(P, n_in)
        if stereo and uniform and n_out:
            if L >= BLOCK and n_out >= BLOCK:
                p.add("store=run_of_4")
            if L % BLOCK:
                p.add("store=singles_block_past_L")
            # the last output's block: j of its first member, and whether the whole run of four exists
            r_last = (n_out - 1) % L
            r0 = r_last - r_last % BLOCK
            if r0 + BLOCK <= L and r_last % BLOCK != BLOCK - 1:
                p.add("store=singles_run_straddles_n_out")
    n = len(clip_lengths)
    if n == 1:
        p.add("batch=one_clip")
    if n > 512:
        p.add("batch=over_512_clips")
    # runs of two or more clips without a tile
    i = 0
    while i < n:
        if has[i]:
            i += 1
            continue
        k = i
        while k < n and not has[k]:
            k += 1
        if k - i >= 2 and any(has):
            p.add("batch=empty_run_front" if i == 0 else "batch=empty_run_end" if k == n else "batch=empty_run_middle")
        i = k
    if stereo and any(v % 2 for v in clip_lengths[1:-1]):
        p.add("batch=stereo_odd_interleaved_middle")
    return p


def clip_paths(P, n_in):
    """the paths of one clip of n_in frames"""
    tile = P["tile_outputs"]
    n_out = n_out_of(P, n_in)
    if not n_out:
        return {"clip=empty"}
    p = set()
    if n_in == 1:
        p.add("clip=n_in_1")
    if n_out == 1:
        p.add("clip=single_output")
    if n_out % tile == 0:
        p.add("clip=exact_tiles")
    if n_out > tile and n_out % tile == 1 % tile:
        p.add("clip=exact_tiles_plus_1")
    if n_out % tile == tile - 1 and tile > 1:
        p.add("clip=exact_tiles_minus_1")
    nt = tiles_of(P, n_out)
    for t in sorted({0, 1, nt // 2, nt - 2, nt - 1} & set(range(nt))):
        start, end = tile_span(P, t)
        if t == 0 and start < 0:
            p.add("tile=first_starts_before_0")
        if 0 < t < nt - 1 and start >= 0 and end <= n_in:
            p.add("tile=middle_span_inside_clip")
        if t == nt - 1:
            p.add("tile=last_ends_beyond_clip" if end > n_in else "tile=last_ends_inside_clip")
    return p


def halo_frames(P, n_in):
    """the clip's frames that two neighbouring tiles both stage"""
    nt = tiles_of(P, n_out_of(P, n_in))
    out = []
    for t in range(nt - 1):
        lo, hi = max(tile_span(P, t + 1)[0], 0), min(tile_span(P, t)[1], n_in)
        if lo < hi:
            out.append((lo, hi))
    return out


def value_paths(P, channels, x):
    """what the samples of one interleaved clip reach"""
    n_in = x.size // channels
    p = set()
    if not n_in:
        return p
    f = x[:n_in * channels].reshape(n_in, channels)
    halo = np.zeros(n_in, bool)
    for lo, hi in halo_frames(P, n_in):
        halo[lo:hi] = True
    for name, mask in (("nan", np.isnan(f).any(axis=1)), ("inf", np.isposinf(f).any(axis=1))):
        if mask[0]:
            p.add("value=%s_first_frame" % name)
        if mask[-1]:
            p.add("value=%s_last_frame" % name)
        if (mask & halo).any():
            p.add("value=%s_shared_halo" % name)
    bits = f.view(np.uint32)
    if (bits == 0x80000000).all():
        p.add("value=negative_zero_clip")
    if is_denormal_clip(x):
        p.add("value=denormal_clip")
    return p


def is_denormal_clip(x):
    a = np.abs(x)
    return bool(x.size and np.isfinite(x).all() and (a < 2.0 ** -126).all() and (a > 0).any())


# ---- the exact reference ---------------------------------------------------------------------------------------------------
def _fma64(h, x, a):
    """fma of f64 arrays that hold f32 values, rounded once to f32"""
    with np.errstate(all="ignore"):
        p = h * x
        s = p + a
        bb = s - p
        err = (p - (s - bb)) + (a - bb)
        bits = s.view(np.int64)
        fix = (err != 0) & ((bits & 1) == 0)
        if fix.any():
            fix &= np.isfinite(s) & np.isfinite(err)
            up = (err > 0) == (s > 0)   # the error points away from zero: one ulp up in magnitude
            s = np.where(fix, np.where(up, bits + 1, bits - 1), bits).view(np.float64)
        return s.astype(np.float32)


def fma(h, x, acc):
    """fma(h, x, acc) of f32 arrays, rounded once: the f64 product of two f32 values is exact; it is added to acc by TwoSum;
    where the sum is inexact and its last mantissa bit is even it moves one ulp towards the error (round to odd at 53
    bits), and a sum rounded to odd at 53 >= 2 * 24 + 2 bits rounds to f32 as the exact value does"""
    return _fma64(h.astype(np.float64), x.astype(np.float64), acc.astype(np.float64))


def _gather(P, n_in, n_out):
    L, M, T = P["L"], P["M"], P["taps"]
    j = np.arange(n_out, dtype=np.int64)
    return (j * M) // L - T // 2 + 1 + T, (j * M) % L   # first tap's index into the padded clip, row


def chain(P, table, x, channels):
    """(y, subnormal) of one interleaved f32 clip: y[n_out * channels] f32, every output the ordered FMA chain over the f32
    table; subnormal: whether any partial sum of any chain was a non-zero subnormal"""
    T = P["taps"]
    n_in = x.size // channels
    n_out = n_out_of(P, n_in)
    if not n_out:
        return np.zeros(0, np.float32), False
    xp = np.zeros((n_in + 2 * T + P["M"] + 2, channels))
    xp[T:T + n_in] = x[:n_in * channels].reshape(n_in, channels)
    base, row = _gather(P, n_in, n_out)
    acc = np.zeros((n_out, channels), np.float32)
    tt = np.ascontiguousarray(table.T.astype(np.float64))
    sub = False
    for k in range(T):
        acc = _fma64(tt[k][row][:, None], xp[base + k], acc.astype(np.float64))
        # a non-zero subnormal: 1 <= magnitude bits <= 0x007FFFFF (zero wraps round to 0xFFFFFFFF)
        sub = sub or bool((((acc.view(np.uint32) & np.uint32(0x7FFFFFFF)) - np.uint32(1)) < np.uint32(0x007FFFFF)).any())
    return acc.reshape(-1), sub


def dot_reference(P, table, x, channels):
    """(y_ref, bound) of one interleaved clip in f64: the dot product and (T + 1) 2^-24 sum |h x| + T 2^-126, the bound of T
    products and T - 1 additions in f32 in any order, with or without FMA, flushed denormals allowed"""
    T = P["taps"]
    n_in = x.size // channels
    n_out = n_out_of(P, n_in)
    xp = np.zeros((n_in + 2 * T + P["M"] + 2, channels))
    xp[T:T + n_in] = x[:n_in * channels].reshape(n_in, channels).astype(np.float64)
    base, row = _gather(P, n_in, n_out)
    y, mag = np.zeros((n_out, channels)), np.zeros((n_out, channels))
    tt = np.ascontiguousarray(table.T.astype(np.float64))
    with np.errstate(all="ignore"):
        for k in range(T):
            prod = tt[k][row][:, None] * xp[base + k]
            y += prod
            mag += np.abs(prod)
    return y.reshape(-1), ((T + 1) * 2.0 ** -24 * mag + T * 2.0 ** -126).reshape(-1)


# ---- cases -----------------------------------------------------------------------------------------------------------------
def _noise(rng, n_in, ch):
    # every channel its own noise, so that a swapped or repeated plane shows
    return rng.uniform(-1.0, 1.0, n_in * ch).astype(np.float32)


def _std_clips(P, ch, rng, tiles=3):
    """noise clips around the tile: `tiles` whole tiles and 17 outputs (first, middle and last tile), one tile exactly, one
    output more, one fewer, a single output, a single input frame, none"""
    tile = P["tile_outputs"]
    clips = []
    for name, n_out in (("%d_tiles_17" % tiles, tiles * tile + 17), ("tile", tile), ("tile_plus_1", tile + 1), ("tile_minus_1", tile - 1),
                        ("one_output", 1)):
        clips.append((name, _noise(rng, n_in_for(P, n_out), ch)))
    clips.append(("one_frame", _noise(rng, 1, ch)))
    clips.append(("empty", np.zeros(0, np.float32)))
    return clips


def _few_clips(P, ch, rng):
    """the channel sweeps: a clip of two tiles and five outputs, a clip of three outputs"""
    tile = P["tile_outputs"]
    return [("2_tiles_5", _noise(rng, n_in_for(P, 2 * tile + 5), ch)), ("3_outputs", _noise(rng, n_in_for(P, 3), ch))]


def _value_clips(P, ch, rng):
    """one NaN and one +inf at frame 0, at the last frame and in the halo two tiles share (NaN in the first channel, the
    infinity in the last); a clip of -0.0; a clip of denormals"""
    tile = P["tile_outputs"]
    n_in = n_in_for(P, tile + 9)
    lo, hi = halo_frames(P, n_in)[0]
    clips = []
    for name, v, c in (("nan", np.float32(np.nan), 0), ("inf", np.float32(np.inf), ch - 1)):
        for where, f in (("first", 0), ("last", n_in - 1), ("halo", (lo + hi) // 2)):
            x = _noise(rng, n_in, ch)
            x[f * ch + c] = v
            clips.append(("%s_%s" % (name, where), x))
    n_short = n_in_for(P, 40)
    clips.append(("negative_zero", np.full(n_short * ch, -0.0, np.float32)))
    clips.append(("denormal", (rng.uniform(-1.0, 1.0, n_short * ch) * 2.0 ** -130).astype(np.float32)))
    return clips


def _batch_700(P, ch, rng):
    """700 clips: runs of empty clips at the front, in the middle and at the end, short clips between them, a clip of a tile
    and a bit here and there; odd interleaved counts (a trailing partial frame) in the middle"""
    tile = P["tile_outputs"]
    clips = []
    for i in range(700):
        if i < 37 or 300 <= i < 345 or i >= 651 or i % 7 == 3:
            n_il = 0
        elif i in (40, 299, 345, 650):
            n_il = n_in_for(P, tile + 3) * ch
        else:
            n_il = int(rng.integers(1, 24)) * ch + (1 if i % 5 == 0 else 0)
        clips.append(("c%03d" % i, rng.uniform(-1.0, 1.0, n_il).astype(np.float32)))
    return clips


# (in_rate, out_rate, channels, what the case is there for, clips)
_TABLE = [
    (48000, 44100, 2, "uniform, 3 idle lanes, windows one frame apart, run-of-4 stores", "std+values"),
    (48000, 44100, 1, "plane variant, one channel", "std"),
    (48000, 44100, 2, "700 clips, runs of empty clips, odd interleaved counts", "batch700"),
    (48000, 44100, 2, "a batch of one clip", "one"),
    (44100, 48000, 2, "uniform, 64 slots, odd M, L mod 4 = 0", "std"),
    (96000, 44100, 2, "side by side, 4 phases per wave", "std+values"),
    (166, 7, 2, "2 phases per wave", "std"),
    (166, 7, 1, "2 phases per wave, plane", "few"),
    (48000, 11025, 2, "8 phases per wave, shift 7", "std"),
    (606, 19, 2, "16 phases per wave", "std"),
    (1226, 39, 2, "32 phases per wave", "std"),
    (2426, 77, 2, "64 phases per wave: one slot", "std"),
    (2426, 77, 3, "64 phases per wave, planes", "few"),
    (162, 7, 2, "uniform, 33 slots: 31 idle lanes", "std"),
    (82, 3, 2, "uniform, 62 slots", "std"),
    (94, 3, 2, "uniform, 51 slots: 13 idle lanes", "std"),
    (192000, 8000, 2, "L = 1, 4 chunks, windows of a block all the same", "std"),
    (32000, 48000, 2, "L = 3, 43 chunks", "std"),
    (48000, 32000, 2, "L = 2, 52 chunks", "std"),
    (32, 1, 2, "2048 taps", "std"),
    (32, 1, 1, "2048 taps, plane", "few"),
    (1, 5, 2, "L = 5, every window of a block on one frame", "std"),
    (128, 5, 2, "uniform with shift 7, windows 25 frames apart", "std"),
    (375, 1024, 2, "1024 phases, side by side", "few"),
    (44100, 8000, 2, "side by side, odd M above 5 L", "few"),
] + [(162, 7, c, "plane uniform, %d channels" % c, "few+values" if c == 3 else "few") for c in PLANE_CHANNELS] \
  + [(96000, 44100, c, "plane side by side, %d channels" % c, "few+values" if c == 3 else "few") for c in PLANE_CHANNELS]

_cases = None


def cases():
    """the batches: dicts with name, in_rate, out_rate, ch, why, plan and clips [(name, f32 interleaved)]; built once"""
    global _cases
    if _cases is None:
        _cases = []
        for n, (a, b, ch, why, kind) in enumerate(_TABLE):
            P = plan(a, b)
            rng = np.random.default_rng(1000 + n)
            clips = []
            for part in kind.split("+"):
                clips += (_std_clips(P, ch, rng) if part == "std" else _few_clips(P, ch, rng) if part == "few" else
                          _value_clips(P, ch, rng) if part == "values" else _batch_700(P, ch, rng) if part == "batch700" else
                          [("only", _noise(rng, n_in_for(P, P["tile_outputs"] + 2), ch))])
            _cases.append(dict(name="%d_%d_x%d_%s" % (a, b, ch, kind.replace("+", "_")), in_rate=a, out_rate=b, ch=ch, why=why, plan=P, clips=clips))
    return _cases


def case_paths(c):
    p = paths(c["in_rate"], c["out_rate"], c["ch"], [x.size for _, x in c["clips"]])
    for _, x in c["clips"]:
        p |= value_paths(c["plan"], c["ch"], x)
    return p


# what tests/test_gpu_resample.py converts, by geometry alone: (in_rate, out_rate, channels) and its lengths in outputs
OLD_PAIRS = [(48000, 44100), (44100, 48000), (96000, 44100), (8000, 44100), (44100, 8000), (44100, 22050), (22050, 44100)]
OLD_CASES = [(a, b, ch) for a, b in OLD_PAIRS for ch in (1, 2)] + [(48000, 44100, 6)]


def old_paths():
    p = set()
    for a, b, ch in OLD_CASES:
        P = plan(a, b)
        tile, T = P["tile_outputs"], P["taps"]
        lengths = [n_in_for(P, n) * ch for n in (0, 1, 2, T // 2, tile - 1, tile, tile + 1, 2 * tile + 17) for _ in range(3)]
        p |= paths(a, b, ch, lengths)
    return p
