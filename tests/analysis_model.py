"""A model of the decisions the analysis metadata takes on the device (flo_amd/csrc/analysis_plan.cpp, analysis_device.hpp,
analysis_batch_kernels.hip), restated in plain Python, and the case table of tests/test_gpu_analysis_paths.py.

* geometry(): analysis_plan() field for field (tests/test_analysis_model_cpu.py pins it to the native dump), items() /
  workgroups(): the batched path's work lists.
* paths(): the predicates over a clip's geometry - which K-weighting path, the segment length, how many quantum edges a
  segment holds, the last segment's frames, the tiles, the hash tree's shape ... - as a set of "name=value" strings, the
  vocabulary of PATHS. Every value of PATHS must be reached by a case (or be named in NOT_REACHED with the reason).
* sumsq_chain(): which chunks of the chained f32 sum of squares must be walked sample by sample, from the sequential sum
  itself.
* cases(): the inputs, each the smallest that reaches its path.
"""
import math

import numpy as np

# ---- constants restated from the sources (test_analysis_model_cpu.py reads them there) --------------------------------
EXACT_FRAMES = 65536      # analysis_fast_path; seg_frames' floor; sq_seg
MAX_FAST_CHANNELS = 64    # analysis_fast_path
TILE = 2048               # kAnTile
HALO = 24                 # kAnHalo
SQ_CHUNK = 1024           # kSqChunk
KW_STEP = 32              # kKwStep (batched K-weighting passes: frames staged per step)
LISTS = ("peaks", "loud", "kw", "kscan", "tile", "fast1", "sqchunk", "sq1", "sumsq", "b3", "clip", "fft")   # AnList
PER_WG = dict(peaks=8, tile=4, sqchunk=16, b3=4)   # an_batch_per_wg; every other list 1


def _llround(x):
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def geometry(n, sr, ch, pps, exact_env=False):
    """analysis_plan(), expression for expression"""
    g = dict(n=n, sr=sr, ch=ch, pps=pps, n_peaks=0, hop=0, n_blocks=0, seg_frames=0, warm_frames=0, n_seg=0, fast=0, kseg_frames=0,
             n_kseg=0, kq=0, sq_exact=0, n_sq_seg=0, n_sq_chunks=0, n_chunks=0, points=[0, 0, 0], point_ok=[0, 0, 0],
             shelf=[0.0] * 5, hp=[0.0] * 5, kpow=[0.0] * 16, tp_coef=[0.0] * 49, block_len=[])
    spp = g["spp"] = float(sr) / float(pps)
    if n:
        tp = math.ceil(float(n) / (spp * float(ch)))
        cap = (4000000000 if tp > 4e9 else int(tp)) if tp > 0 else 0
        # (the first window that starts behind the clip ends the count; the condition is monotone: found by bisection)
        lo, hi = 0, cap   # every window below lo starts inside; none from hi on does, or hi is the cap
        while lo < hi:
            mid = (lo + hi) // 2
            if int(float(mid) * spp) * ch < n:
                lo = mid + 1
            else:
                hi = mid
        np_ = lo
        g["n_peaks"] = np_
    if not n:
        return g
    rate = float(sr)
    f0, g_db, q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    k, vh = math.tan(math.pi * f0 / rate), math.pow(10.0, g_db / 20.0)
    vb = math.pow(vh, 0.4996667741545416)
    a0 = 1.0 + k / q + k * k
    g["shelf"] = [(vh + vb * k / q + k * k) / a0, 2.0 * (k * k - vh) / a0, (vh - vb * k / q + k * k) / a0, 2.0 * (k * k - 1.0) / a0,
                  (1.0 - k / q + k * k) / a0]
    f0h, qh = 38.13547087602444, 0.5003270373238773
    kh = math.tan(math.pi * f0h / rate)
    a0h = 1.0 + kh / qh + kh * kh
    g["hp"] = [1.0, -2.0, 1.0, 2.0 * (kh * kh - 1.0) / a0h, (1.0 - kh / qh + kh * kh) / a0h]
    hop = g["hop"] = _llround(rate * 0.1)
    frames = n // ch
    if hop:
        start, block = 0, hop * 4
        while start < frames:
            end = min(start + block, frames)
            if end <= start:
                break
            g["block_len"].append(end - start)
            if end == frames:
                break
            start += hop
    g["n_blocks"] = len(g["block_len"])
    g["seg_frames"] = max(EXACT_FRAMES, 8 * hop)
    g["warm_frames"] = max(8192, sr // 4)
    longest = (n + ch - 1) // ch
    g["n_seg"] = max(1, (longest + g["seg_frames"] - 1) // g["seg_frames"])
    g["fast"] = int(frames > EXACT_FRAMES and hop != 0 and ch <= MAX_FAST_CHANNELS and not exact_env)
    L = 256
    while L < 2048 and L * L * 8 < frames:
        L *= 2
    g["kseg_frames"] = L
    g["n_kseg"] = (frames + L - 1) // L
    g["kq"] = L // hop + 2 if hop else 1
    if g["fast"]:
        sh, hp = g["shelf"], g["hp"]
        for col in range(4):
            v = [0.0] * 4
            v[col] = 1.0
            for _ in range(L):
                y = v[0]
                n1, n2 = -sh[3] * y + v[1], -sh[4] * y
                y2 = hp[0] * y + v[2]
                m1, m2 = hp[1] * y - hp[3] * y2 + v[3], hp[2] * y - hp[4] * y2
                v = [n1, n2, m1, m2]
            for r in range(4):
                g["kpow"][4 * r + col] = v[r]
    g["sq_exact"] = int(n > EXACT_FRAMES)
    g["n_sq_seg"] = 1 if g["sq_exact"] else (n + EXACT_FRAMES - 1) // EXACT_FRAMES
    g["n_sq_chunks"] = (n + 1023) // 1024
    osr, cutoff = float(sr) * 4.0, float(sr) * 0.45
    co = []
    for i in range(49):
        nn = float(i) - 24.0
        sinc = 2.0 * cutoff / osr if abs(nn) < 1e-12 else math.sin(2.0 * cutoff * nn / osr) / (math.pi * nn)
        co.append(sinc * (0.5 * (1.0 - math.cos(2.0 * math.pi * float(i) / 48.0))))
    s = 0.0
    for c in co:
        s += c
    g["tp_coef"] = [c / s for c in co]
    g["n_chunks"] = (9 + 4 * n + 1023) // 1024
    g["points"] = [frames // 4, frames // 2, frames * 3 // 4]
    g["point_ok"] = [int(p + 256 < frames) for p in g["points"]]
    return g


def items(g):
    """an_batch_items: {list: items}"""
    it = dict.fromkeys(LISTS, 0)
    if not g["n"]:
        return it
    ch, longest = g["ch"], (g["n"] + g["ch"] - 1) // g["ch"]
    it["peaks"] = g["n_peaks"]
    if g["fast"]:
        it.update(kw=(g["n_kseg"] + 63) // 64 * ch, kscan=ch, tile=(longest + TILE - 1) // TILE * ch, fast1=1)
    else:
        it["loud"] = g["n_seg"] * ch
    if g["sq_exact"]:
        it.update(sqchunk=g["n_sq_chunks"], sq1=1)
    else:
        it["sumsq"] = g["n_sq_seg"]
    it.update(b3=(g["n_chunks"] + 127) // 128, clip=1, fft=3)
    return it


def workgroups(g):
    return {k: (v + PER_WG.get(k, 1) - 1) // PER_WG.get(k, 1) for k, v in items(g).items()}


def dump_line(g):
    """the integers of one line of `analysis_plan_test dump`, in its order"""
    head = [g["n_peaks"], g["hop"], g["n_blocks"], g["seg_frames"], g["warm_frames"], g["n_seg"], g["fast"], g["kseg_frames"], g["n_kseg"],
            g["kq"], g["sq_exact"], g["n_sq_seg"], g["n_sq_chunks"], g["n_chunks"]] + g["points"] + g["point_ok"]
    it, wg = items(g), workgroups(g)
    return head, [it[k] for k in LISTS], [wg[k] for k in LISTS], [g["spp"]] + g["shelf"] + g["hp"] + g["kpow"] + g["tp_coef"]


# ---- the hash tree ---------------------------------------------------------------------------------------------------
def blake3_shape(n):
    """(chunks, level sizes from the chunks up to the root, bytes of the last chunk, word-path blocks, byte-path blocks)"""
    total = 9 + 4 * n
    chunks = (total + 1023) // 1024
    levels, m = [chunks], chunks
    while m > 1:
        m = m // 2 + (m & 1)
        levels.append(m)
    last = total - (chunks - 1) * 1024
    blocks = (total + 63) // 64
    # an_blake3_chunks_body: the word path for a block at 12 bytes or more that lies wholly inside the message (chunks are
    # multiples of 64 bytes, so a block's offset is global)
    bo = 64 * np.arange(blocks, dtype=np.int64)
    word = int(((bo >= 12) & (bo + 64 <= total)).sum())
    return chunks, levels, last, word, blocks - word


# ---- predicates ------------------------------------------------------------------------------------------------------
def kw_path(g):
    if g["fast"]:
        return "two_pass"
    return "warmup" if g["n_seg"] > 1 else "one_walk"


def kw_segments(g):
    """two-pass path: per segment (frames, quantum edges inside its frames, an edge in the padded lanes behind the last)"""
    frames, L, hop = g["n"] // g["ch"], g["kseg_frames"], g["hop"]
    f0 = np.arange(g["n_kseg"], dtype=np.int64) * L
    f1 = np.minimum(f0 + L, frames)
    edges = (f1 - 1) // hop - f0 // hop
    cnt = int(f1[-1] - f0[-1])
    pad_end = int(f0[-1]) + (cnt + 7) // 8 * 8
    first_edge = (int(f0[-1]) // hop + 1) * hop
    while first_edge < int(f1[-1]):
        first_edge += hop
    return f1 - f0, edges, first_edge < pad_end, bool(((f0[1:] % hop) == 0).any())


def paths(g):
    """the predicate values of one clip, as "name=value" strings"""
    n, ch = g["n"], g["ch"]
    p = set()
    if not n:
        return {"empty"}
    frames = n // ch
    kp = kw_path(g)
    p.add("kw=" + kp)
    p.add("partial_frame=%d" % int(n % ch != 0))
    if kp == "two_pass":
        cnt, edges, pad_edge, on_edge = kw_segments(g)
        p.add("kseg=%d" % g["kseg_frames"])
        p.add("max_edges=%d" % int(edges.max()))
        p.add("kq_slots=%s" % ("over_3" if int(edges.max()) + 1 > 3 else "up_to_3"))
        p.add("seg_starts_on_edge=%d" % int(on_edge))
        p.add("n_kseg_mod64=%s" % {0: "0", 1: "1"}.get(g["n_kseg"] % 64, "other"))
        last = int(cnt[-1])
        p.add("last_seg=%s" % ("1" if last == 1 else "full" if last == g["kseg_frames"] else "part"))
        p.add("last_seg_mod8=%d" % (last % 8))
        p.add("edge_in_pad=%d" % int(pad_edge))
        p.add("frames_mod_hop=%s" % {0: "0", 1: "1", g["hop"] - 1: "hop-1"}.get(frames % g["hop"], "other"))
        tiles = ((n + ch - 1) // ch + TILE - 1) // TILE
        p.add("tiles=%s" % ("1" if tiles == 1 else "many"))
        p.add("last_tile=%s" % ("full" if ((n + ch - 1) // ch) % TILE == 0 else "part"))
        # the tiles are counted from the longest channel: behind a partial frame a shorter channel may have none of the last
        p.add("a_channels_last_tile_empty=%d" % int((frames + TILE - 1) // TILE < tiles))
    elif kp == "warmup":
        p.add("warmup_n_seg=%s" % ("2" if g["n_seg"] == 2 else "over_2"))
        p.add("warmup_seg_frames=%s" % ("65536" if g["seg_frames"] == EXACT_FRAMES else "8_hop"))
    else:
        p.add("one_walk=%s" % ("over_65536_frames" if frames > EXACT_FRAMES else "hop_0" if not g["hop"] else "short"))
    p.add("ch=%s" % ("1" if ch == 1 else "2" if ch == 2 else "64" if ch == 64 else "over_64" if ch > 64 else "3_to_63"))
    p.add("sumsq=%s" % ("chain" if g["sq_exact"] else "one_segment"))
    if g["sq_exact"]:
        p.add("sq_chunks_mod64=%s" % {0: "0", 1: "1"}.get(g["n_sq_chunks"] % 64, "other"))
        p.add("sq_last_chunk=%s" % ("full" if n % SQ_CHUNK == 0 else "part"))
    chunks, levels, last, word, byte = blake3_shape(n)
    p.add("b3_chunks=%s" % (str(chunks) if chunks <= 9 or chunks in (127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025) else "many"))
    odd = sum(1 for m in levels[:-1] if m & 1 and m > 1)
    p.add("b3_odd_levels=%s" % ("0" if odd == 0 else "1" if odd == 1 else "several"))
    p.add("b3_last_chunk=%s" % ("1_byte" if last == 1 else "1024" if last == 1024 else "1021" if last == 1021 else "other"))
    p.add("b3_groups=%s" % ("1" if chunks <= 128 else "many"))
    p.add("b3_tree=%s" % ("leaf" if chunks == 1 else "one_pass" if chunks // 2 <= 256 else "several_passes"))
    p.add("fft_points=%d%d%d" % tuple(g["point_ok"]))
    if any(g["point_ok"]) and n % ch:
        lastp = max(pt for pt, ok in zip(g["points"], g["point_ok"]) if ok)
        p.add("fft_reaches_partial_frame=%d" % int((lastp + 255) * ch + ch - 1 >= frames * ch))
    empty = False
    if g["n_peaks"] < 200000:
        i = np.arange(g["n_peaks"], dtype=np.float64)
        s = (i * g["spp"]).astype(np.uint64) * ch
        e = np.minimum(((i + 1.0) * g["spp"]).astype(np.uint64) * ch, n)
        empty = bool((e <= s).any())
    p.add("peak_windows=%s" % ("some_empty" if empty else "fractional" if g["spp"] != int(g["spp"]) else "whole"))
    return p


PATHS = {
    "k-weighting": ["kw=one_walk", "kw=two_pass", "kw=warmup", "kseg=256", "kseg=512", "kseg=1024", "kseg=2048",
                    "max_edges=0", "max_edges=1", "max_edges=2", "max_edges=3", "max_edges=6", "kq_slots=up_to_3", "kq_slots=over_3",
                    "seg_starts_on_edge=0", "seg_starts_on_edge=1", "n_kseg_mod64=0", "n_kseg_mod64=1", "n_kseg_mod64=other",
                    "last_seg=1", "last_seg=full", "last_seg=part"] + ["last_seg_mod8=%d" % k for k in range(8)] +
                   ["edge_in_pad=0", "edge_in_pad=1", "frames_mod_hop=0", "frames_mod_hop=1", "frames_mod_hop=hop-1", "frames_mod_hop=other",
                    "warmup_n_seg=2", "warmup_n_seg=over_2", "warmup_seg_frames=65536", "warmup_seg_frames=8_hop",
                    "one_walk=short", "one_walk=over_65536_frames", "one_walk=hop_0",
                    "ch=1", "ch=2", "ch=3_to_63", "ch=64", "ch=over_64", "partial_frame=0", "partial_frame=1"],
    "peak tiles": ["tiles=1", "tiles=many", "last_tile=full", "last_tile=part", "a_channels_last_tile_empty=0",
                   "a_channels_last_tile_empty=1"],
    "sum of squares": ["sumsq=one_segment", "sumsq=chain", "sq_chunks_mod64=0", "sq_chunks_mod64=1", "sq_chunks_mod64=other",
                       "sq_last_chunk=full", "sq_last_chunk=part"],
    "blake3": ["b3_chunks=%d" % c for c in list(range(1, 10)) + [127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025]] +
              ["b3_chunks=many", "b3_odd_levels=0", "b3_odd_levels=1", "b3_odd_levels=several", "b3_last_chunk=1_byte", "b3_last_chunk=1021",
               "b3_last_chunk=1024", "b3_last_chunk=other", "b3_groups=1", "b3_groups=many", "b3_tree=leaf", "b3_tree=one_pass",
               "b3_tree=several_passes"],
    "fft": ["fft_points=000", "fft_points=100", "fft_points=110", "fft_points=111", "fft_reaches_partial_frame=0", "fft_reaches_partial_frame=1"],
    "waveform peaks": ["peak_windows=whole", "peak_windows=fractional", "peak_windows=some_empty"],
}
# paths the case table does not reach, each with the reason
NOT_REACHED = {
    "tiles=1": "the tile kernels run on the two-pass path only, which starts beyond 65 536 frames: 33 tiles at least",
    "b3_last_chunk=1024": "9 + 4 n is odd: no message ends on a chunk boundary",
    "fft_reaches_partial_frame=1": "point_ok asks for points + 256 < frames: the last window ends one whole frame before the clip's "
                                   "last whole frame, so the `idx < n` guard of an_fft_body never decides anything",
    "one_walk=hop_0": "needs a rate below 5 Hz: the hash, peaks and FFT of such a clip are covered at ordinary rates, and the loudness is "
                      "the default by construction (no blocks)",
}


# ---- the chained sum of squares --------------------------------------------------------------------------------------
def _binade(S):
    """sq_binade: e with S in [2^e, 2^(e+1)); None for 0, tiny, huge, inf, NaN"""
    S = np.float32(S)
    if not (S >= np.float32(1e-30)) or not (S < np.float32(1e30)):
        return None
    return int(np.frexp(S)[1]) - 1


def sumsq_chain(x):
    """-> dict(result, chunks, must_walk: {chunk: reason}, one_addition). From the sequential f32 sum itself
    (np.cumsum(x * x, dtype=float32) is that recurrence): a chunk cannot be one addition when the sum at its start has no
    binade (below 1e-30: the first chunk always), when a square is not finite (beyond 3e38), when a term reaches
    2^(e + 2), or when the sum leaves its binade inside the chunk."""
    x = np.asarray(x, np.float32).ravel()
    with np.errstate(over="ignore", invalid="ignore"):
        t = x * x
        cs = np.cumsum(t, dtype=np.float32)
    n_chunks = (x.size + SQ_CHUNK - 1) // SQ_CHUNK
    must = {}
    for c in range(n_chunks):
        i0, i1 = c * SQ_CHUNK, min((c + 1) * SQ_CHUNK, x.size)
        S0 = np.float32(0) if c == 0 else cs[i0 - 1]
        e = _binade(S0)
        tc = t[i0:i1]
        if e is None:
            must[c] = "no binade at the start"
        elif not (tc <= np.float32(3.0e38)).all():
            must[c] = "a square that is not finite"
        elif float(tc.max()) >= 2.0 ** (e + 2):
            must[c] = "a term of 2^(e+2) or more"
        elif _binade(cs[i1 - 1]) != e:
            must[c] = "leaves the binade"
    return dict(result=cs[-1] if x.size else np.float32(0), chunks=n_chunks, must_walk=must, one_addition=n_chunks - len(must))


def sumsq_ties(x):
    """how many additions of the sequential sum are rounding ties (t / ulp(S) half-way between two integers) while the sum
    has a binade: the additions whose increment depends on the parity of S"""
    x = np.asarray(x, np.float32).ravel()
    t = x * x
    cs = np.cumsum(t, dtype=np.float32)
    prev = np.concatenate([[np.float32(0)], cs[:-1]])
    ok = prev >= np.float32(1e-30)
    e = np.frexp(prev[ok])[1].astype(np.int64) - 1
    sc = np.ldexp(t[ok].astype(np.float64), (23 - e).astype(np.int32))
    return int((sc - np.floor(sc) == 0.5).sum())


# ---- the cases ---------------------------------------------------------------------------------------------------------
def _noise(frames, ch, seed, extra=0, amp=0.1):
    """noise whose level swells slowly (so that the blocks differ and the range is not zero), a different gain per channel;
    `extra` samples of a trailing partial frame"""
    rng = np.random.default_rng(seed)
    n = frames * ch + extra
    x = rng.standard_normal(n, dtype=np.float32)
    t = np.arange(n, dtype=np.float32) / np.float32(max(ch, 1))
    x *= np.float32(amp) * (np.float32(1.0) + np.float32(0.6) * np.sin(t * np.float32(2 * math.pi / 3777.0)))
    if ch > 1:
        x *= np.tile(np.linspace(1.0, 0.4, ch, dtype=np.float32), frames + 1)[:n]
    return x


def _burst(frames, ch, seed, spans):
    """digital silence with bursts of noise at [start, end) frames, a different burst per channel"""
    rng = np.random.default_rng(seed)
    x = np.zeros((frames, ch), np.float32)
    for a, b in spans:
        x[a:b] = rng.standard_normal((b - a, ch), dtype=np.float32) * np.linspace(0.3, 0.05, ch, dtype=np.float32)
    return x.ravel()


def _spike(frames, ch, seed, at, chan, extra=0):
    """quiet noise with a three-sample alternating spike centred on frame `at` of channel `chan`"""
    x = _noise(frames, ch, seed, extra, amp=0.001).copy()
    for k, v in ((-1, -0.7), (0, 0.9), (1, -0.7)):
        i = (at + k) * ch + chan
        if 0 <= i < x.size:
            x[i] = v
    return x


def _pcm16(n, seed, amp=0.5):
    """16-bit material: rint(x * 32767) / 32768"""
    rng = np.random.default_rng(seed)
    return (np.rint(rng.uniform(-amp, amp, n) * 32767.0) / 32768.0).astype(np.float32)


def _with(x, at, v):
    x = x.copy()
    x[at] = v
    return x


def _tone(frames, ch, sr, hz, amp=0.5):
    t = np.arange(frames, dtype=np.float64)
    return np.repeat((amp * np.sin(2 * math.pi * hz * t / sr)).astype(np.float32), ch)


def _crossing_at(x, chunk, lo=1e-3, hi=0.5):
    """quiet 16-bit material up to `chunk`, loud behind: the sum crosses binades where the loud part starts"""
    y = (x * np.float32(lo / 0.5)).astype(np.float32)
    y = (np.rint(y * 32767.0) / 32768.0).astype(np.float32)
    y[chunk * SQ_CHUNK:] = x[chunk * SQ_CHUNK:]
    return y


_CASES = None


def cases():
    """[dict(name, family, sr, ch, pps, n, make)] - make() builds the samples (deterministic, not kept)"""
    global _CASES
    if _CASES is not None:
        return _CASES
    C = []

    def add(name, family, sr, ch, n, make, pps=50, **kw):
        C.append(dict(name=name, family=family, sr=sr, ch=ch, n=n, pps=pps, make=make, **kw))

    def noise(name, family, sr, ch, frames, extra=0, pps=50):
        add(name, family, sr, ch, frames * ch + extra, lambda: _noise(frames, ch, len(name) * 131 + frames % 9973, extra), pps)

    # K-weighting and block energies
    for fr in (65536, 65537):
        noise(f"kw 8 kHz mono {fr}", "kw", 8000, 1, fr)
    for fr in (524288, 524289, 2097152, 2097153, 8388608, 8388609):
        noise(f"kw 4 kHz mono {fr}", "kw", 4000, 1, fr)
    noise("kw 320 segments", "kw", 8000, 1, 320 * 256)
    noise("kw 321 segments, the last of one frame", "kw", 8000, 1, 320 * 256 + 1)
    for m in range(30, 38):   # hop 2205: m hop - 1 frames leave a last segment of every residue mod 8, the edge right behind it
        noise(f"kw 22050 Hz {m} hops less one", "kw", 22050, 1, m * 2205 - 1)
    for d in (0, 1, -1):
        noise(f"kw 44100 Hz stereo 21 hops {d:+d}", "kw", 44100, 2, 21 * 4410 + d, extra=1 if d == 1 else 0)
    for sr, frs in ((96000, (65537, 76800, 76801)), (192000, (65537, 153600, 153601))):
        for fr in frs:
            noise(f"kw {sr} Hz mono {fr}", "kw", sr, 1, fr)
    for ch in (65, 64):
        for fr in (65537, 140000):
            noise(f"kw 8 kHz {ch} channels {fr}", "kw", 8000, ch, fr)
    noise("kw 96 kHz 65 channels 70000: one walk beyond 65536 frames", "kw", 96000, 65, 70000)
    noise("kw 96 kHz 65 channels 76801: warm-up segments of 8 hops", "kw", 96000, 65, 76801)
    noise("kw 8 kHz 3 channels 70001 and a partial frame", "kw", 8000, 3, 70001, extra=2)
    # localised bursts (8 kHz: hop 800, segments of 256 frames; 25600 is a boundary of both)
    B = 100000
    for name, spans in (("across a segment boundary", [(25856 - 150, 25856 + 150)]), ("across a quantum edge", [(26400 - 150, 26400 + 150)]),
                        ("across both at once", [(25600 - 150, 25600 + 150)]), ("in the first segment", [(0, 200)]),
                        ("in the last segment", [(B - 160, B)]), ("two bursts a block apart", [(40000, 40300), (43100, 43400)])):
        add("burst " + name, "burst", 8000, 2, B * 2, (lambda s=spans, nm=name: _burst(B, 2, len(nm), s)))
    add("burst 65 channels across the segment boundary", "burst", 8000, 65, 140000 * 65, lambda: _burst(140000, 65, 5, [(65536 - 150, 65536 + 150)]))
    add("burst 65 channels inside the warm-up of the second segment", "burst", 8000, 65, 140000 * 65, lambda: _burst(140000, 65, 6, [(60000, 60300)]))
    # non-finite samples and an unstable filter
    for ch, tag in ((1, "two-pass"), (65, "warm-up")):
        fr = 70000 if ch == 1 else 140000
        for where, at in (("first", 100), ("middle", fr // 2 + 3), ("last", fr - 2)):
            for v, vn in ((np.nan, "NaN"), (np.inf, "infinity")):
                add(f"{vn} in the {where} segment, {tag}", "nonfinite", 8000, ch, fr * ch,
                    (lambda fr=fr, ch=ch, at=at, v=v: _with(_noise(fr, ch, 77), at * ch + (ch - 1), v)))
    noise("2 kHz: the shelf filter is unstable", "nonfinite", 2000, 1, 70000)
    # true-peak and sample-peak tiles
    for path, sr, ch, fr in (("one walk", 44100, 2, 3 * TILE + 100), ("two passes", 44100, 2, 33 * TILE + 100)):
        tiles = (fr + TILE - 1) // TILE
        for t in sorted({1, tiles // 2, tiles - 1}):
            for d in (-25, -24, -1, 0, 23, 24, 25):
                add(f"spike {path} tile {t} {d:+d}", "peak", sr, ch, fr * ch, (lambda fr=fr, ch=ch, t=t, d=d: _spike(fr, ch, t, TILE * t + d, ch - 1)))
        for at in (0, 5, 23, fr - 24, fr - 6, fr - 1):
            add(f"spike {path} frame {at}", "peak", sr, ch, fr * ch, (lambda fr=fr, ch=ch, at=at: _spike(fr, ch, at, at, 0)))
        add(f"spike {path} in the trailing partial frame", "peak", sr, ch, fr * ch + 1, (lambda fr=fr, ch=ch: _spike(fr, ch, 9, fr, 0, extra=1)))
    # 33 x 2048 whole frames and channel 0's lone sample behind them: tile 33 exists for channel 0 alone, and the reduction reads
    # channel 1's pair of it all the same
    add("stereo, 33 tiles and one sample (the last tile of channel 1 is empty)", "peak", 44100, 2, 2 * 33 * TILE + 1,
        lambda: _spike(33 * TILE, 2, 11, 33 * TILE, 0, extra=1))
    add("spike three channels, the last channel, partial frame behind", "peak", 22050, 3, 70000 * 3 + 2, lambda: _spike(70000, 3, 4, 34 * TILE, 2, extra=2))
    # sum of squares
    add("16-bit material 2.5 M samples", "sumsq", 44100, 2, 2_500_000, lambda: _pcm16(2_500_000, 1))
    add("16-bit material, quiet, odd length", "sumsq", 44100, 1, 2_100_001, lambda: _pcm16(2_100_001, 2, 0.01))   # quiet: the sum stays in low binades, ties in every 64th term
    for nm, chunk in (("inside a group of 64", 64 * 9 + 30), ("at a group's first chunk", 64 * 9), ("at a group's last chunk", 64 * 9 + 63)):
        add("16-bit material, quiet then loud " + nm, "sumsq", 44100, 2, 2_000_000, (lambda chunk=chunk: _crossing_at(_pcm16(2_000_000, 3), chunk)))
    add("a sum that stalls: loud, then terms below half an ulp", "sumsq", 44100, 2, 1_000_000,
        lambda: np.concatenate([_pcm16(200_000, 4, 0.9), (_pcm16(800_000, 5, 0.9) * np.float32(2.0 ** -13))]).astype(np.float32), stalled=True)
    # BLAKE3: chunk counts (9 + 4 n bytes in chunks of 1024: c chunks from n = 256 c - 258 to 256 c - 3)
    for c in list(range(1, 10)) + [127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 3446]:
        for ch in (1, 2, 3):
            n = 256 * c - 3 - (ch * 7 if c > 1 else 0)
            n = max(n, ch)
            add(f"hash {c} chunks, {ch} channels", "b3", 16000, ch, n, (lambda n=n, c=c, ch=ch: _noise(n // ch, ch, c, n % ch)))
    for c in (2, 5, 128, 129, 300):
        add(f"hash {c} chunks, the last of one byte", "b3", 16000, 2, 256 * (c - 1) - 2, (lambda c=c: _noise(128 * (c - 1) - 1, 2, c + 1)))
        add(f"hash {c} chunks, the last of 1021 bytes", "b3", 16000, 3, 256 * c - 3, (lambda c=c: _noise((256 * c - 3) // 3, 3, c + 2, (256 * c - 3) % 3)))
    # FFT sections
    for fr in (341, 342, 343, 512, 513, 514, 1023, 1024, 1025, 1026):
        noise(f"fft {fr} frames", "fft", 16000, 1, fr)
        noise(f"fft {fr} frames stereo and a partial frame", "fft", 16000, 2, fr, extra=1)
    add("fft one all-zero section", "fft", 16000, 2, 8000 * 2, lambda: _with_zero_section(_noise(8000, 2, 8), 2, 4000, 256))
    add("fft all zeros", "fft", 16000, 2, 8000 * 2, lambda: np.zeros(16000, np.float32))
    add("fft tone on the boundary of two bands", "fft", 16000, 1, 8000, lambda: _tone(8000, 1, 16000, 16000.0 * 8 / 256))
    add("fft tone on the boundary of two peak bands", "fft", 16000, 1, 8000, lambda: _tone(8000, 1, 16000, 16000.0 * 15.5 / 256))
    # waveform peaks
    noise("peaks 100000 a second at 44.1 kHz", "wave", 44100, 2, 3000, pps=100000)
    noise("peaks 7 a second at 22050 Hz", "wave", 22050, 1, 30000, pps=7)      # (3150 samples a window: whole after all)
    noise("peaks 11 a second at 22050 Hz", "wave", 22050, 2, 30000, extra=1, pps=11)   # 2004.5454...: a fractional window
    for ch in (1, 2, 3):
        noise(f"peaks {ch} channels and a partial frame", "wave", 22050, ch, 20000, extra=ch - 1 if ch > 1 else 0, pps=7 if ch == 3 else 50)
    add("peaks a NaN in a window of its own", "wave", 8000, 1, 8000, lambda: _with(_noise(8000, 1, 12), 4000, np.nan), pps=8000)
    _CASES = C
    return C


def _with_zero_section(x, ch, frame, count):
    x = x.copy()
    x[frame * ch:(frame + count) * ch] = 0
    return x


def case(name):
    return next(c for c in cases() if c["name"] == name)


# ---- what a case must give ---------------------------------------------------------------------------------------------
ABS_GATE = 10.0 ** ((-70.0 + 0.691) / 10.0)
_EXPECTED = {}


def exact(g):
    """the whole loudness in the reference's own order: one walk over one segment"""
    return not g["fast"] and g["n_seg"] == 1


def expected(c):
    """The oracle's results for a case and the bound on the device's loudness (kept per case: the values are small).

    Beyond one exact segment the device adds the same squares in another order (segments, then quanta, then blocks) from
    start states that are right to 1e-16, so it cannot be asked to equal the f64 oracle; both are measured against the
    oracle's long-double twin instead. E is the largest relative distance of the f64 oracle's block energies from the
    twin's, over the blocks at or above the absolute gate (no other block enters the loudness or the range, and the gate
    condition below rules out a block that is in for one and out for the other). The device's loudness may lie
    (10 / ln 10) 4 E + 4 ulp from the twin's, its range twice that: an error of E relative in every energy moves
    10 log10 of a mean of energies by (10 / ln 10) E at most, the factor 4 is for the other order of additions and the
    start states, the ulps for the logarithm, the division and the percentile interpolation themselves.
    gates_ok: no block energy lies within 1e-9 relative of the absolute or the relative gate."""
    if c["name"] not in _EXPECTED:
        x = c["make"]()
        assert x.size == c["n"] and x.dtype == np.float32, (c["name"], x.size, c["n"])
        _EXPECTED[c["name"]] = reference(x, c["sr"], c["ch"], c["pps"])
    return _EXPECTED[c["name"]]


def reference(x, sr, ch, pps=50, loudness_only=False):
    """expected() for any clip (not kept); loudness_only: the four loudness values and their bounds alone"""
    from oracle import oracle as O
    x = np.ascontiguousarray(x, np.float32).ravel()
    g = geometry(x.size, sr, ch, pps)
    en, ld = O.block_energies(x, ch, sr), O.block_energies(x, ch, sr, long_double=True)
    m = O.loudness_metrics(x, ch, sr)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        live = np.isfinite(en) & np.isfinite(ld) & (en >= ABS_GATE)
        E = float(np.max(np.abs(en[live] - ld[live]) / ld[live])) if live.any() else 0.0
        gated = en[np.isfinite(en) & (en >= ABS_GATE)]
        gates_ok = True
        if en.size:
            fin = en[np.isfinite(en) & (en > 0)]
            gates_ok = not (np.abs(fin - ABS_GATE) <= 1e-9 * ABS_GATE).any()
            if gated.size:
                rel_gate = 10.0 ** ((-0.691 + 10.0 * math.log10(float(np.sum(gated)) / gated.size) - 10.0 + 0.691) / 10.0)
                gates_ok = gates_ok and not (np.abs(fin - rel_gate) <= 1e-9 * rel_gate).any()
    lufs_ld, lra_ld = O.gated_lufs(ld), O.loudness_range(ld)
    tol = (10.0 / math.log(10.0)) * 4.0 * E
    r = dict(geometry=g, exact=exact(g), E=E, gates_ok=gates_ok, metrics=m, lufs_ld=lufs_ld, lra_ld=lra_ld,
             tol_lufs=tol + 4 * float(np.spacing(abs(lufs_ld))) if math.isfinite(lufs_ld) else 0.0,
             tol_lra=2 * (tol + 4 * float(np.spacing(max(abs(lufs_ld), abs(lra_ld))))) if math.isfinite(lufs_ld) and math.isfinite(lra_ld) else 0.0,
             n_blocks=int(en.size), n_gated=int(gated.size))
    if not loudness_only:
        with np.errstate(over="ignore", invalid="ignore"):
            sumsq = np.cumsum(x * x, dtype=np.float32)[-1]
        r.update(fingerprint=O.spectral_fingerprint(x, ch, sr), peaks=O.waveform_peaks(x, ch, sr, pps), meta=O.analysis_metadata(x, sr, ch, pps),
                 sum_squares=sumsq)
    return r


def same_float(a, b):
    """bit for bit, any NaN matching any NaN"""
    return (math.isnan(a) and math.isnan(b)) or np.float64(a).tobytes() == np.float64(b).tobytes()


def check_loudness(a, e, who):
    """the four loudness values of a device result against a reference(): true and sample peak bit for bit at any length
    (order-free maxima of identically ordered sums), loudness and range bit for bit within one exact segment and within
    the reference's bound of the long-double twin beyond; returns the measured distances"""
    m, d = e["metrics"], {}
    for k in ("true_peak_dbtp", "sample_peak_dbfs"):
        assert same_float(a[k], m[k]), (who, k, a[k], m[k])
    for k, ref, tol in (("integrated_lufs", e["lufs_ld"], e["tol_lufs"]), ("loudness_range_lu", e["lra_ld"], e["tol_lra"])):
        if e["exact"] or not math.isfinite(m[k]):
            assert same_float(a[k], m[k]), (who, k, a[k], m[k])
            d[k] = 0.0
        else:
            d[k] = abs(a[k] - ref)
            print(f"{who}: {k} device {a[k]!r} twin {ref!r} f64 oracle {m[k]!r}: distance {d[k]:.3e}, bound {tol:.3e}, E {e['E']:.3e}")
            assert e["gates_ok"], (who, "a block energy sits on a gate: the bound does not apply to this input")
            assert d[k] <= tol, (who, k, a[k], ref, d[k], tol)
    return d


def check_analysis(a, meta, c, tag=""):
    """one device result (Context.analyze's dict and the META bytes) against expected(c); returns the measured distances"""
    e = expected(c)
    m, fp, who = e["metrics"], e["fingerprint"], (c["name"], tag)
    assert a["peaks"].size == e["peaks"].size and np.array_equal(a["peaks"].view(np.uint32), e["peaks"].view(np.uint32)), (who, "peaks")
    assert a["hash"] == fp["hash"], (who, "hash")
    for k in ("duration_ms", "frequency_peaks", "energy_profile", "avg_loudness"):
        assert a[k] == fp[k], (who, k, a[k], fp[k])
    got, want = np.float32(a["sum_squares"]), e["sum_squares"]
    assert got.view(np.uint32) == want.view(np.uint32) or (np.isnan(got) and np.isnan(want)), (who, "sum_squares", got, want)
    d = check_loudness(a, e, c["name"] + tag)
    if meta is not None:
        assert meta == e["meta"], (who, "META")
    return d
