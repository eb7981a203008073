"""The model of the device's FIR filtering and convolution (flo_batch_convolve, flo_convolve), in numpy: the
definition restated literally, one exact f32 FMA (resample_model._fma64) per tap over all outputs of a clip; the refusals;
the named paths of the kernel; the cases of the device tests; and flo_fir_design's definition in f64.

Definition. Source clip: N whole frames of C channels. Response clip: P whole frames of Ch channels, Ch == 1 or Ch == C.
K = min(taps, P - min(ir_start, P)); h[k, c] is frame ir_start + k of the response, channel (Ch == 1 ? 0 : c). Output sample
(t, c) of T = frames: a = +0.0, then for k = 0 .. K - 1 ascending, m = t + skip - k, xv = x[m, c] if 0 <= m < N else +0.0,
a = fma(h[k, c], xv, a)."""
import numpy as np

import edit_model as E
import resample_model as R

F32 = np.float32
ALL = 0xFFFFFFFF
MAX_TAPS = 65536
FLT_MAX = np.finfo(F32).max
TILE, CHUNK, LANE = 2048, 256, 8   # kConvTileFrames, kConvTapChunk, kConvLaneOutputs (flo_conv_geometry; test_convolve_cpu.py compares)


def job(clip=0, ir=0, frames=0, skip=0, ir_start=0, taps=ALL, reserved=0):
    return dict(clip=clip, ir=ir, frames=frames, skip=skip, ir_start=ir_start, taps=taps, reserved=reserved)


def taps_of(taps, P, ir_start):
    return min(taps, P - min(ir_start, P))


def refusal(src_frames, ch, ir_frames, ir_ch, jobs, size_max=2 ** 64 - 1, same_rate=True):
    """the quantity the error message names, or None for a list of jobs that is accepted"""
    if not same_rate:
        return "sample_rate"
    if not 1 <= ch <= 8:
        return "channels"
    if ir_ch not in (1, ch):
        return "ir_channels"
    tiles = 0
    for g in jobs:
        if g["clip"] >= len(src_frames):
            return "clip"
        if g["ir"] >= len(ir_frames):
            return "ir"
        if g["reserved"]:
            return "reserved"
        if taps_of(g["taps"], ir_frames[g["ir"]], g["ir_start"]) > MAX_TAPS:
            return "taps"
        if g["frames"] + g["skip"] >= 1 << 64:
            return "frames + skip"
        if g["frames"] > size_max // 8 // ch:
            return "frames"
        tiles += -(-g["frames"] // TILE)
        if tiles > 0x7FFFFFFF:
            return "tiles"
    return None


def _subnormal64(a):
    """whether any value of the f64 array is non-zero and below the smallest normal f32 in magnitude"""
    a = np.abs(a)
    return bool(((a > 0) & (a < 2.0 ** -126)).any())


def convolve_clip(x, ch, h, ir_ch, g):
    """(y, subnormal) of one job: y[T * ch] f32; subnormal: whether any product or any partial sum was a non-zero subnormal
    (what a device that flushes them would compute differently)"""
    x, h = np.asarray(x, F32), np.asarray(h, F32)
    N, P, T, skip = x.size // ch, h.size // ir_ch, g["frames"], g["skip"]
    K = taps_of(g["taps"], P, g["ir_start"])
    X = x[:N * ch].reshape(N, ch).astype(np.float64)
    H = h[:P * ir_ch].reshape(P, ir_ch)[g["ir_start"]:g["ir_start"] + K].astype(np.float64) if K else np.zeros((0, ir_ch))
    if ir_ch == 1:
        H = np.repeat(H, ch, axis=1)
    acc = np.zeros((T, ch), F32)
    sub = False
    for k in range(K):
        m0 = skip - k                          # output t meets source frame t + m0
        lo, hi = min(max(0, -m0), T), max(min(T, N - m0), 0)
        xs = np.zeros((T, ch))
        if hi > lo:
            xs[lo:hi] = X[lo + m0:hi + m0]
        with np.errstate(all="ignore"):
            sub = sub or _subnormal64(H[k][None, :] * xs)
        acc = R._fma64(np.broadcast_to(H[k][None, :], (T, ch)), xs, acc.astype(np.float64))
        sub = sub or _subnormal64(acc.astype(np.float64))
    return acc.reshape(-1), sub


def convolve(src, ch, irs, ir_ch, jobs, strict=False):
    """every output clip of the list; strict: assert that no case meets a subnormal"""
    out = []
    for g in jobs:
        y, sub = convolve_clip(src[g["clip"]], ch, irs[g["ir"]], ir_ch, g)
        assert not (strict and sub), ("a subnormal in a bit-for-bit case", g)
        out.append(y)
    return out


def mode_job(mode, n, k, **kw):
    """the job of Batch.convolve's `mode` for a clip of n frames and a response of k taps"""
    skip, frames = {"head": (0, n), "full": (0, n + k - 1 if n and k else 0), "centered": ((k - 1) // 2 if k else 0, n)}[mode]
    return job(frames=frames, skip=skip, **kw)


def same(got, want):
    return E.same(got, want)


# ---- flo_fir_design in f64 ----------------------------------------------------------------------------------------------
LOWPASS, HIGHPASS, BANDPASS, BANDSTOP = 0, 1, 2, 3


def _lp(f, rate, taps, beta):
    H = taps // 2
    d = np.arange(taps, dtype=np.float64) - H
    c = 2.0 * f / rate
    g = c * np.sinc(c * d) * np.i0(beta * np.sqrt(1.0 - (d / H) ** 2)) / np.i0(beta)
    return g / g.sum()


def fir_design64(kind, rate, f_lo, f_hi, taps, beta):
    """the definition in f64 (numpy's sinc and i0)"""
    delta = np.zeros(taps)
    delta[taps // 2] = 1.0
    if kind == LOWPASS:
        return _lp(f_hi, rate, taps, beta)
    if kind == HIGHPASS:
        return delta - _lp(f_lo, rate, taps, beta)
    band = _lp(f_hi, rate, taps, beta) - _lp(f_lo, rate, taps, beta)
    return band if kind == BANDPASS else delta - band


# ---- the named paths ----------------------------------------------------------------------------------------------------
K_EDGES = {"K 0": 0, "K 1": 1, "K lane - 1": LANE - 1, "K lane": LANE, "K lane + 1": LANE + 1, "K chunk - 1": CHUNK - 1, "K chunk": CHUNK,
           "K chunk + 1": CHUNK + 1, "K 2 chunk + 3": 2 * CHUNK + 3}
T_EDGES = {"T 0": 0, "T 1": 1, "T tile - 1": TILE - 1, "T tile": TILE, "T tile + 1": TILE + 1, "T 2 tile - 1": 2 * TILE - 1, "T 2 tile": 2 * TILE,
           "T 2 tile + 1": 2 * TILE + 1}
PATHS = sorted(list(K_EDGES) + list(T_EDGES) + [
    "window before the clip", "window over the clip's start", "window over the clip's end", "window behind the clip", "window inside the clip",
    "N 0", "N below K", "ir_start odd", "taps cut by the response's end", "ir_start at or beyond P", "skip beyond N + K",
    "source alignment 0", "source alignment 1", "source alignment 2", "source alignment 3", "Ch 1", "Ch C", "irs is src"])


def expected_paths(ch, ir_ch):
    """the paths a batch of these channel counts can reach (irs is src has a test of its own): skip * ch floats are the
    source's offset, so the alignment classes are those multiples of ch mod 4"""
    out = set(PATHS) - {"irs is src"} - {"source alignment %d" % a for a in range(4) if a not in {s * ch % 4 for s in range(4)}}
    if ch > 1:
        out.discard("Ch C" if ir_ch == 1 else "Ch 1")
    return out


def paths(g, N, P, ch, ir_ch):
    """the named paths job g reaches. A window is what one workgroup stages for one chunk of taps of one tile: the source
    frames from t0 + skip - (k0 + nc - 1) to t0 + nf - 1 + skip - k0"""
    K, T, skip = taps_of(g["taps"], P, g["ir_start"]), g["frames"], g["skip"]
    got = {name for name, v in K_EDGES.items() if v == K} | {name for name, v in T_EDGES.items() if v == T}
    got.add("Ch 1" if ir_ch == 1 else "Ch C")
    if ir_ch == ch == 1:
        got.add("Ch C")
    if T and K:
        if N == 0:
            got.add("N 0")
        elif N < K:
            got.add("N below K")
        if g["ir_start"] & 1:
            got.add("ir_start odd")
        if g["taps"] != ALL and K < g["taps"]:
            got.add("taps cut by the response's end")
        if skip > N + K:
            got.add("skip beyond N + K")
        got.add("source alignment %d" % (skip * ch % 4))
        for t0 in range(0, T, TILE):
            nf = min(TILE, T - t0)
            for k0 in range(0, K, CHUNK):
                nc = min(CHUNK, K - k0)
                lo, hi = t0 + skip - (k0 + nc - 1), t0 + nf - 1 + skip - k0
                if hi < 0:
                    got.add("window before the clip")
                elif lo >= N:
                    got.add("window behind the clip")
                else:
                    if lo < 0:
                        got.add("window over the clip's start")
                    if hi >= N:
                        got.add("window over the clip's end")
                    if lo >= 0 and hi < N:
                        got.add("window inside the clip")
    if T and g["ir_start"] >= P:
        got.add("ir_start at or beyond P")
    return got


# ---- the cases of the device tests --------------------------------------------------------------------------------------
def noise(n, ch, seed, edges=()):
    """Gaussian noise away from zero with -0.0, the infinities, NaN and +-FLT_MAX planted at `edges` (frames), walking over the
    channels; no denormals"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n * ch) * 0.25).astype(F32).reshape(n, ch)
    x[np.abs(x) < F32(1e-6)] = F32(0.125)
    specials = [-0.0, np.inf, -np.inf, np.nan, FLT_MAX, -FLT_MAX]
    for k, f in enumerate(edges):
        if 0 <= f < n:
            x[f, k % ch] = F32(specials[k % len(specials)])
    return x.reshape(-1)


SOURCE_EDGES = (0, 1, LANE - 1, LANE, CHUNK - 1, CHUNK, TILE - CHUNK, TILE - 1, TILE, TILE + 1, TILE + CHUNK, 2 * TILE - 1, 2 * TILE)
SOURCE_FRAMES = (0, 1, 5, TILE + 1, 2 * TILE + 5, 3 * TILE + 5)
IR_FRAMES = (0, 1, LANE - 1, LANE, LANE + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)


def device_case(ch, ir_ch):
    """(source clips, response clips, jobs) of one batch for a source of `ch` channels and responses of `ir_ch`. No source is
    longer than 3 * TILE + 5 frames; responses 0 .. 8 are plain noise of IR_FRAMES frames, 9 has -0.0 and +-FLT_MAX among its
    taps, 10 an infinity, 11 a NaN, 12 is long (3 * CHUNK + 40 frames)"""
    src = [noise(n, ch, 500 + i, SOURCE_EDGES if i % 2 else ()) for i, n in enumerate(SOURCE_FRAMES)]
    src[4] = noise(SOURCE_FRAMES[4], ch, 504, SOURCE_EDGES)
    irs = [(noise(p, ir_ch, 600 + i) * F32(0.5)).astype(F32) for i, p in enumerate(IR_FRAMES)]
    harsh = noise(LANE + 3, ir_ch, 650).reshape(-1, ir_ch)
    harsh[1, 0], harsh[4, -1], harsh[LANE, 0] = F32(-0.0), F32(FLT_MAX), F32(-FLT_MAX)
    inf, nan = noise(CHUNK + 1, ir_ch, 651).reshape(-1, ir_ch), noise(5, ir_ch, 652).reshape(-1, ir_ch)
    inf[CHUNK, -1] = F32(np.inf)     # the last tap of its channel, past a chunk edge
    nan[2, 0] = F32(np.nan)
    irs += [harsh.reshape(-1), inf.reshape(-1), nan.reshape(-1), (noise(3 * CHUNK + 40, ir_ch, 653) * F32(0.25)).astype(F32)]
    BIG, PLAIN, LONG = 4, 3, 12      # source 2 * TILE + 5 with planted values; source TILE + 1 without; the long response
    jobs = []
    Ts = list(T_EDGES.values())
    for i in range(len(IR_FRAMES)):                       # every short K against every T, every long K against two of them
        for j, T in enumerate(Ts):
            if IR_FRAMES[i] <= LANE + 1 or j % 4 == i % 4:
                jobs.append(job(BIG, i, T, skip=(i + j) % 4))
    n = SOURCE_FRAMES[PLAIN]
    for skip in (0, 1, 2, 3, CHUNK // 2, CHUNK, CHUNK + 1, n - 1, n, n + CHUNK, n + CHUNK + 1, n + CHUNK + 2, n + 5000, 1 << 40, (1 << 64) - 1 - 300):
        jobs.append(job(PLAIN, 7, n if skip in (1, CHUNK + 1, n) else 300, skip=skip))   # the clip slides out of the window, to the largest skip there is
    jobs += [job(BIG, 8, CHUNK - 9), job(BIG, 8, 100, skip=0), job(PLAIN, LONG, TILE + 10, skip=TILE + 700)]   # windows before / behind the clip
    for i in (0, 1, 2):                                   # N = 0, and N below K
        jobs += [job(i, 1, 9), job(i, 7, TILE + 3, skip=CHUNK), job(i, LONG, 40, skip=7)]
    for start, taps in ((1, ALL), (3, 100), (2 * CHUNK - 20, 100), (CHUNK + 3, 7), (CHUNK + 2, ALL), (CHUNK + 3, ALL), (CHUNK + 4, 5), (1 << 63, ALL)):
        jobs.append(job(BIG, 8 if start < 1000 else 7, TILE + 9, skip=start % 3, ir_start=start, taps=taps))   # ir_start below, at and beyond P; taps cut
    jobs += [job(BIG, 8, TILE, taps=0), job(BIG, LONG, TILE + 1, taps=CHUNK + 1), job(BIG, LONG, TILE + 5, skip=(3 * CHUNK + 39) // 2)]
    for i in (9, 10, 11):                                 # special values among the taps, against special values among the samples
        jobs += [job(BIG, i, TILE + CHUNK, skip=s) for s in (0, 5)] + [job(PLAIN, i, 300, skip=2)]
    jobs += [job(5, 7, 3 * TILE + 5, skip=CHUNK // 2), job(5, 2, 3 * TILE + 5 + LANE - 2)]      # three tiles and a ragged fourth
    for t in range(1, 2 * LANE + 2):                      # every ragged length of a lane's run
        jobs.append(job(BIG, 4, TILE + t, skip=t))
    for i, n in enumerate(SOURCE_FRAMES):                 # every source length under every short response, at and around its ends
        for ir in (1, 2, 3, 4):
            for si, skip in enumerate((0, 1, 2, 3, max(n - 1, 0), n, n + 3)):
                T = (n + IR_FRAMES[ir] - 1, n, min(n, TILE) + 1, LANE + 1)[(i + ir + si) % 4]
                jobs.append(job(i, ir, T, skip=skip))
    return src, irs, jobs


def case_paths(src, irs, jobs, ch, ir_ch):
    got = set()
    for g in jobs:
        got |= paths(g, src[g["clip"]].size // ch, irs[g["ir"]].size // ir_ch, ch, ir_ch)
    return got


def work(src, irs, jobs, ch, ir_ch):
    """sum of K * T * C over the jobs: what the model costs"""
    return sum(taps_of(g["taps"], irs[g["ir"]].size // ir_ch, g["ir_start"]) * g["frames"] * ch for g in jobs)
