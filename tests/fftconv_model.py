"""The model of the partitioned FFT convolution (flo_batch_convolve_fft, flo_convolve_fft), in numpy and
scipy.fft, which keeps float32: the operation restated, the exact f64 convolution, and the yardstick both are held to.

The operation. Jobs, K = min(taps, P - min(ir_start, P)), h[k, c], Ch and the skip clamp are convolve_model's. With
B = block_frames, F = 2B, Pn = ceil(K / B): partition p is taps [pB, min((p+1)B, K)) of channel c zero-padded to F, H_p its
real FFT; segment q is source frames [(q-1)B + skip, (q+1)B + skip), +0.0 outside [0, N), X_q its real FFT; output block b is
frames [bB, (b+1)B): Y_b = sum over p = 0 .. Pn-1 ascending of X_{b-p} H_p from zero, and the last B values of irfft(Y_b) are
the block. Segments wholly outside the clip are zero; here they are multiplied like any other, which adds exact zeros.

The yardstick. Per output block and channel, s_b = sum over p of ||segment b-p||_2 ||partition p||_2 in f64: what the
block's F values can reach, and what every rounding of the transforms and of the accumulation is proportional to.
r = max over blocks with s_b > 0 of max|err| / s_b, err against the exact f64 convolution; a block with s_b == 0 must be
zero. Measured on the CPU for B = 256, 512, 1024 on N = 3B+5, K = 2B+70; N = 5000, K = 7, skip 31; N = 2B, K = B,
skip B-1; N = 4B+1, K = 8B+3, skip 3B; N = 20000, K = 16384; N = K = 1 (uniform noise at 0.3, a response of noise under
an exponential): r between 1.1e-8 and 6.0e-8; on the jobs of the device cases at B = 512 up to 6.7e-8; zero-scale blocks 0."""
import numpy as np
import scipy.fft

import convolve_model as CM

F32 = np.float32
ALL = CM.ALL
MAX_TAPS = 1 << 20
R_CAP = 2.0 ** -22      # no model figure may pass this: a sloppy model must not loosen the device's bound
job, mode_job, taps_of = CM.job, CM.mode_job, CM.taps_of


def _parts(x, ch, h, ir_ch, g):
    """(X[N, ch] f32, H[K, ch] f32, T, skip clamped) of one job"""
    x, h = np.asarray(x, F32), np.asarray(h, F32)
    N, P = x.size // ch, h.size // ir_ch
    K = taps_of(g["taps"], P, g["ir_start"])
    X = x[:N * ch].reshape(N, ch)
    H = h[:P * ir_ch].reshape(P, ir_ch)[g["ir_start"]:g["ir_start"] + K] if K else np.zeros((0, ir_ch), F32)
    if ir_ch == 1:
        H = np.repeat(H, ch, axis=1)
    return X, H, g["frames"], min(g["skip"], N + K)


def _segments(X, T, skip, Pn, B):
    """seg[q + Pn - 1] = segment q for q = -(Pn - 1) .. nb - 1: [nseg, 2B, ch] f32"""
    N, ch = X.shape
    nb = -(-T // B)
    lo, hi = (-Pn) * B, nb * B                      # x'[m] = x[m + skip] for m in [lo, hi)
    line = np.zeros((hi - lo, ch), F32)
    a, b = max(lo, -skip), min(hi, N - skip)        # the m whose source frame exists
    if b > a:
        line[a - lo:b - lo] = X[a + skip:b + skip]
    nseg = nb + Pn - 1
    idx = np.arange(nseg)[:, None] * B + np.arange(2 * B)[None, :]
    return line[idx] if nseg > 0 else np.zeros((0, 2 * B, ch), F32)


def _partitions(H, Pn, B):
    K, ch = H.shape
    pad = np.zeros((Pn * B, ch), F32)
    pad[:K] = H
    return pad.reshape(Pn, B, ch)


def model_clip(x, ch, h, ir_ch, g, B):
    """one job through the operation in float32: y[T * ch]"""
    X, H, T, skip = _parts(x, ch, h, ir_ch, g)
    K = H.shape[0]
    Pn, nb = -(-K // B), -(-T // B)
    if T == 0:
        return np.zeros(0, F32)
    if K == 0:
        return np.zeros(T * ch, F32)
    seg = _segments(X, T, skip, Pn, B)
    part = np.zeros((Pn, 2 * B, ch), F32)
    part[:, :B] = _partitions(H, Pn, B)
    with np.errstate(all="ignore"):
        XS = scipy.fft.rfft(seg, axis=1)
        HS = scipy.fft.rfft(part, axis=1)
        assert XS.dtype == np.complex64 and HS.dtype == np.complex64
        Y = np.zeros((nb, B + 1, ch), np.complex64)
        for p in range(Pn):                         # block b meets partition p at segment b - p: index b - p + Pn - 1
            Y += XS[Pn - 1 - p:Pn - 1 - p + nb] * HS[p][None]
        y = scipy.fft.irfft(Y, n=2 * B, axis=1)[:, B:]
    assert y.dtype == F32
    return np.ascontiguousarray(y.reshape(nb * B, ch)[:T]).reshape(-1)


def exact_clip(x, ch, h, ir_ch, g):
    """the convolution in f64: [T, ch]"""
    X, H, T, skip = _parts(x, ch, h, ir_ch, g)
    N, K = X.shape[0], H.shape[0]
    out = np.zeros((T, ch))
    if N and K and T:
        for c in range(ch):
            full = np.convolve(X[:, c].astype(np.float64), H[:, c].astype(np.float64))   # N + K - 1
            n = max(0, min(T, full.size - skip))
            out[:n, c] = full[skip:skip + n]
    return out


def scales(x, ch, h, ir_ch, g, B):
    """s_b per block and channel: [nb, ch] f64"""
    X, H, T, skip = _parts(x, ch, h, ir_ch, g)
    K = H.shape[0]
    Pn, nb = -(-K // B), -(-T // B)
    s = np.zeros((nb, ch))
    if K and nb:
        sn = np.sqrt((_segments(X, T, skip, Pn, B).astype(np.float64) ** 2).sum(axis=1))   # [nseg, ch]
        pn = np.sqrt((_partitions(H, Pn, B).astype(np.float64) ** 2).sum(axis=1))          # [Pn, ch]
        for p in range(Pn):
            s += sn[Pn - 1 - p:Pn - 1 - p + nb] * pn[p][None]
    return s


def ratio(got, exact, s, B):
    """(r, whether every zero-scale block is zero) of got[T * ch] against exact[T, ch] under s[nb, ch]"""
    T, ch = exact.shape
    if T == 0:
        return 0.0, got.size == 0
    nb = s.shape[0]
    err = np.zeros((nb * B, ch))
    err[:T] = np.abs(np.asarray(got, F32).reshape(T, ch).astype(np.float64) - exact)
    worst = err.reshape(nb, B, ch).max(axis=1)
    live = s > 0
    with np.errstate(all="ignore"):
        r = float((worst[live] / s[live]).max()) if live.any() else 0.0
    mag = np.zeros((nb * B, ch))
    mag[:T] = np.abs(np.asarray(got, F32).reshape(T, ch).astype(np.float64))
    zero_ok = not (mag.reshape(nb, B, ch).max(axis=1)[~live] != 0).any()
    return r, zero_ok


def job_ratio(got, x, ch, h, ir_ch, g, B):
    return ratio(got, exact_clip(x, ch, h, ir_ch, g), scales(x, ch, h, ir_ch, g, B), B)


def stored_segments(N, T, K, skip, B):
    """how many segments of a job meet the clip and some block (what the device stores)"""
    if not (N and K and T):
        return 0
    skip = min(skip, N + K)
    Pn, nb = -(-K // B), -(-T // B)
    lo, hi = max((-skip) // B, -(Pn - 1)), min(-(-(N - skip) // B) + 1, nb)   # -ceil(skip / B); ceil((N - skip) / B) + 1
    return max(0, hi - lo)


def reached_blocks(frame, skip, N, K, B, nb):
    """the output blocks a value at source frame `frame` reaches: the segments that hold it, each by every partition"""
    skip = min(skip, N + K)
    Pn = -(-K // B)
    q = (frame - skip) // B
    return [b for b in range(nb) if any(b - Pn + 1 <= s <= b for s in (q, q + 1))]


# ---- inputs -------------------------------------------------------------------------------------------------------------
def noise(n, ch, seed, amp=0.3):
    return np.random.default_rng(seed).uniform(-amp, amp, n * ch).astype(F32)


def decay(n, ch, seed, amp=0.3):
    """noise under an exponential: a response"""
    env = np.exp(-np.arange(n) / max(n / 4.0, 1.0))
    return (np.random.default_rng(seed).uniform(-amp, amp, (n, ch)) * env[:, None]).astype(F32).reshape(-1)


def tones(n, ch, B):
    """bin-centred tones of the F = 2B transform, DC and Nyquist; other bins in every channel"""
    t = np.arange(n)
    x = np.zeros((n, ch))
    for c in range(ch):
        x[:, c] = 0.1 + 0.2 * (1 - 2 * (t & 1)) + 0.3 * np.cos(2 * np.pi * (5 + 3 * c) * t / (2 * B)) + 0.15 * np.sin(2 * np.pi * (B - 2 - c) * t / (2 * B))
    return x.astype(F32).reshape(-1)


def impulse(n, ch, at):
    x = np.zeros((n, ch), F32)
    x[at] = 1.0
    return x.reshape(-1)


CPU_SHAPES = ("N 3B+5, K 2B+70", "N 5000, K 7, skip 31", "N 2B, K B, skip B-1", "N 4B+1, K 8B+3, skip 3B", "N 20000, K 16384", "N K 1")


def cpu_shape(name, B):
    """(x, h, job) of one of the shapes the module's docstring quotes, mono"""
    N, K, skip = {CPU_SHAPES[0]: (3 * B + 5, 2 * B + 70, 0), CPU_SHAPES[1]: (5000, 7, 31), CPU_SHAPES[2]: (2 * B, B, B - 1),
                  CPU_SHAPES[3]: (4 * B + 1, 8 * B + 3, 3 * B), CPU_SHAPES[4]: (20000, 16384, 0), CPU_SHAPES[5]: (1, 1, 0)}[name]
    return noise(N, 1, 11), decay(K, 1, 12), job(0, 0, N + K - 1, skip)


def device_case(ch, ir_ch, B, LB, sweeps=False, big=False):
    """(source clips, response clips, jobs) of one batch. No source is longer than 3 * LB * B + 5 frames, except (big) one of
    20000 against 16384 taps. sweeps: a unit impulse at every position of segment 0 (one clip, the skip walks), and a unit tap
    at every position 0 .. 2B (one response, ir_start walks), where the output is the shifted source"""
    n0, n1 = 3 * LB * B + 5, LB * B + 37
    src = [noise(n0, ch, 1), noise(n1, ch, 2), np.zeros(0, F32), noise(1, ch, 3), tones(4 * B, ch, B), impulse(3 * B, ch, B - 1)]
    p0 = (LB + 1) * B + 1
    irs = [decay(p0, ir_ch, 4), np.zeros(0, F32), impulse(2 * B + 1, ir_ch, 2 * B), decay(2 * B + 70, ir_ch, 5)]
    jobs = []
    for K in (0, 1, B - 1, B, B + 1, 2 * B + 70, p0):                       # K edges, in full
        jobs.append(job(1, 0, n1 + K - 1 if K else n1, taps=K))
    for T in (0, 1, B, B + 1, n0):                                          # T edges
        jobs.append(job(0, 3, T))
    jobs += [job(2, 3, 300), job(3, 3, 2 * B + 80), job(3, 0, 1, taps=1), job(2, 1, 7)]   # N 0 and 1; P 0
    for skip in (B - 1, B, n1 + 5, n1 + 2 * B + 70 + 1000, n1 + 2 * B + 70):  # skip: beyond N, beyond N + K, at N + K
        jobs.append(job(1, 3, B + 9, skip))
    jobs += [job(1, 0, n1, ir_start=7, taps=300), job(1, 0, n1, ir_start=p0), job(1, 0, n1, ir_start=p0 + 5), job(1, 0, 700, ir_start=p0 - 1)]
    for mode in ("head", "full", "centered"):
        jobs.append(mode_job(mode, n0, 2 * B + 70, clip=0, ir=3))
    jobs += [mode_job("full", 4 * B, 2 * B + 70, clip=4, ir=3), job(4, 2, 4 * B, ir_start=2 * B)]   # tones; through h = [1]
    if sweeps:
        jobs += [job(5, 3, 2 * B + 80, skip=s) for s in range(2 * B)]
        jobs += [job(1, 2, B + 40, skip=9, ir_start=2 * B - d) for d in range(2 * B + 1)]
    if big:
        src.append(noise(20000, ch, 6))
        irs.append(decay(16384, ir_ch, 7, 0.05))
        jobs.append(job(len(src) - 1, len(irs) - 1, 20000))
    return src, irs, jobs
