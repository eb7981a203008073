"""The exact reference of the forward transform of the lossy encoder, in float64 NumPy, and the clips every place that hands
coefficients out is held to it on.

A plain restatement of mdct.rs:166-226 plus the framing of encoder.rs:167-239:

    X_h,c[k] = sum_{n < 2048} w[n] * x_c[(h - 1) * 1024 + n] * cos(pi / 1024 * (n + 0.5 + 512) * (k + 0.5)),  k < 1024
    x_c is zero before the clip (1024 sample-frames of pre-roll) and behind it; a trailing partial sample-frame is dropped
    hops = (n_sf + 1024 + 1023) // 1024

w is the oracle's f32 Vorbis window promoted to float64 (data, as in tdec_ref). The basis is tdec_ref's: the angle is
(2 n + 1025)(2 k + 1) * pi / 4096 with the integer product reduced mod 8192 before it meets pi. tdec_ref._basis() carries
the inverse side's factor 2 / 1024 = 2^-9; the forward side has none, so the product is multiplied by 512 - exact, a power
of two.

Errors are normalised per (frame, channel) by that frame's largest |coefficient| of the truth: a frame that holds one
sample under the window's first entry (9e-7) is measured as closely as a full-scale one. A (frame, channel) whose truth is
all zero must hold nothing but zeros of either sign.

Tight class (TIGHT): finite in float64 and in the oracle, at most 6 frames and 8 channels. Edge class (EDGE): one NaN, +inf
or -inf at one sample of one channel; the (frame, channel) pairs whose window holds that sample are left to the oracle's
pattern, every other pair to the tight bound. Inputs that overflow or go subnormal INSIDE the transform (amplitudes beyond
1e34 or below 1e-34) are in neither class: which of their values become inf, NaN or a flushed zero depends on the order of
operations, and proves nothing about the transform."""
import functools

import numpy as np

import lossy_model
import signals
import tdec_ref
from oracle import oracle as O

SR = 44100
QUALITIES = (0.55, 1.0)      # 1.0 selects the exact-threshold instantiations: separate code objects, the transform inlined again
FORMS = (1, 2, 5)


# ------------------------------------------------------------------------------------------------------- the reference
def hops_of(n_sf):
    return (n_sf + 1024 + 1023) // 1024


def windows(pcm, ch):
    """interleaved f32 clip -> [hops][ch][2048] f32: the samples every frame's transform sees, zeros around the clip"""
    p = np.ascontiguousarray(pcm, np.float32).reshape(-1)
    n_sf = p.size // ch
    hops = hops_of(n_sf)
    x = np.zeros(((hops + 1) * 1024, ch), np.float32)
    x[1024:1024 + n_sf] = p[:n_sf * ch].reshape(n_sf, ch)
    out = np.empty((hops, ch, 2048), np.float32)
    for h in range(hops):
        out[h] = x[h * 1024:h * 1024 + 2048].T
    return out


def transform(win):
    """[..., 2048] windows -> [..., 1024] float64 coefficients, from the definition"""
    w = np.asarray(win, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return (w.reshape(-1, 2048) @ tdec_ref._basis()).reshape(w.shape[:-1] + (1024,)) * 512.0


@functools.lru_cache(maxsize=1)
def _cosines():
    n = np.arange(2048, dtype=np.int64)[:, None]
    k = np.arange(1024, dtype=np.int64)[None, :]
    return np.cos((((2 * n + 1025) * (2 * k + 1)) % 8192).astype(np.float64) * (np.pi / 4096.0))


def transform_f32_products(win):
    """The same sum with every product w[n] * x[n] rounded to f32 first, as the reference's windowing loop and both of the
    oracle's float64 evaluations do (oracle/lossy.c: "the windowing product is f32 in the reference"). Not the truth: what
    the CPU test holds the oracle's f64 evaluations to, so that the roundings they add are counted one at a time."""
    xw = (np.asarray(win, np.float32) * O.window(2048)).astype(np.float32).astype(np.float64)
    return (xw.reshape(-1, 2048) @ _cosines()).reshape(xw.shape[:-1] + (1024,))


def affected(win):
    """[hops][ch] bool: the window holds a sample that is not finite"""
    return ~np.isfinite(win).all(axis=-1)


def truth_of(pcm, ch):
    """-> (float64 [hops][ch][1024], skip [hops][ch]): the exact coefficients; where a window holds a non-finite sample the
    pair is marked in `skip` and its row computed with that sample as zero (it is not compared)"""
    win = windows(pcm, ch)
    return transform(np.where(np.isfinite(win), win, np.float32(0.0))), affected(win)


def measure(got, truth, skip=None):
    """got: f32 (or f64) [frames][ch][1024]; truth: float64 of the same shape -> dict(
    worst   = max over (frame, channel) of max_k |got - truth| / max_k |truth|, over pairs whose truth is not all zero,
    at      = (frame, channel, bin) of it,
    rms     = sqrt(sum err^2 / sum truth^2),
    zero_ok = every pair whose truth is all zero holds nothing but +-0, zero_at = the first that does not,
    finite, frames = pairs compared). Pairs marked in `skip` take no part in any of them."""
    g = np.asarray(got).astype(np.float64)
    assert g.shape == truth.shape and g.ndim == 3 and g.shape[2] == 1024, (g.shape, truth.shape)
    nf, ch = g.shape[:2]
    use = np.ones((nf, ch), bool) if skip is None else ~np.asarray(skip, bool)
    finite = bool(np.isfinite(g[use]).all())
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.where(use[..., None], np.abs(g - truth), 0.0)
        tmax = np.abs(truth).max(axis=2)
        live = use & (tmax > 0)
        ratio = np.where(live, err.max(axis=2) / np.where(live, tmax, 1.0), 0.0)
        silent = ~(use & (tmax == 0)) | (g == 0.0).all(axis=2)
        zero_ok = bool(silent.all())
        zero_at = None if zero_ok else tuple(int(x) for x in np.argwhere(~silent)[0])
        if nf and np.isnan(ratio).any():
            f, c = (int(x) for x in np.argwhere(np.isnan(ratio))[0])
        elif nf:
            f, c = (int(x) for x in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
        else:
            f = c = 0
        worst = float(ratio[f, c]) if nf else 0.0
        k = int(np.argmax(np.nan_to_num(err[f, c], nan=np.inf))) if nf else 0
        den = float((np.where(use[..., None], truth, 0.0) ** 2).sum())
        num = float((err ** 2).sum())
        rms = float(np.sqrt(num / den)) if den > 0 else float(np.sqrt(num))
    return dict(worst=worst, rms=rms, at=(f, c, k), zero_ok=zero_ok, zero_at=zero_at, finite=finite, frames=int(live.sum()),
                got=float(g[f, c, k]) if nf else 0.0, want=float(truth[f, c, k]) if nf else 0.0, scale=float(tmax[f, c]) if nf else 0.0)


# ------------------------------------------------------------------------------------------------------------ the cases
IMPULSE_AT = (0, 1, 511, 512, 1023, 1024, 1025, 1535, 1536, 2046, 2047)
TONE_BINS = (0, 1, 31, 32, 511, 512, 1022, 1023)
LENGTHS = (0, 1, 300, 1023, 1024, 1025, 2047, 2048, 2049)
LEVELS = ("1e-30", "1e-5", "1", "3000", "1e30")
WINDOWS = "impulse_windows"      # the 2048 windows that hold a single 1.0: through mdct_forward only (not a clip)


def _noise(n_sf, ch, seed):
    return np.random.default_rng(seed).uniform(-0.9, 0.9, (n_sf, ch)).astype(np.float32).reshape(-1)


def _tone(k0, n_sf, phase):
    t = np.arange(n_sf, dtype=np.float64)
    return np.cos(2.0 * np.pi * ((k0 + 0.5) / 2048.0) * t + phase)


def _stack(chans):
    return np.ascontiguousarray(np.stack(chans, axis=1), np.float32).reshape(-1)


def _makers():
    """name -> (maker of the interleaved f32 clip, channels)"""
    P = functools.partial
    out = {}
    # wiring: independent full-scale noise per channel; a wrong channel, stride or sample is an error of order 1
    for ch in (1, 2, 3, 5, 8):
        out[f"noise_{ch}ch"] = (P(_noise, 2500, ch, 100 + ch), ch)
    # edges: the pre-roll, the predicated loads of the last frames against the fast loads everywhere else, the spare
    # half-frame; the stereo clip of 1025 sample-frames carries one sample more (a partial sample-frame: dropped)
    for ch in (1, 2):
        for n in LENGTHS:
            extra = 1 if (n == 1025 and ch == 2) else 0
            out[f"len_{n}_{ch}ch"] = (P(lambda n, ch, extra: _noise(n + 1, ch, 200 + 10 * n + ch)[:n * ch + extra], n, ch, extra), ch)
    # impulses: one window entry and one fold row each; stereo carries another position in channel 1
    for i, p in enumerate(IMPULSE_AT):
        def one(p=p):
            x = np.zeros(2048, np.float32)
            x[p] = 1.0
            return x

        def two(p=p, r=IMPULSE_AT[(i + 4) % len(IMPULSE_AT)]):
            x = np.zeros((2048, 2), np.float32)
            x[p, 0] = 1.0
            x[r, 1] = 1.0
            return x.reshape(-1)
        out[f"impulse_{p}_1ch"] = (one, 1)
        out[f"impulse_{p}_2ch"] = (two, 2)
    # tones on a bin's centre frequency, amplitude 1.0: the energy sits in one or two bins, what leaks into the quiet ones is
    # what is measured. Stereo: channel 1 carries the mirrored bin at another phase
    for k0 in TONE_BINS:
        out[f"tone_{k0}_1ch"] = (P(lambda k0: _stack([_tone(k0, 3000, 0.25)]), k0), 1)
        out[f"tone_{k0}_2ch"] = (P(lambda k0: _stack([_tone(k0, 3000, 0.25), _tone(1023 - k0, 3000, 1.0)]), k0), 2)
    t = np.arange(3000)
    sq = np.where((t // 32) % 2 == 0, 1.0, -1.0)
    sq2 = np.where((t // 50) % 2 == 0, -1.0, 1.0)
    ny = np.where(t % 2 == 0, 1.0, -1.0)
    out["dc_1ch"] = (lambda: _stack([np.full(3000, 0.5)]), 1)
    out["dc_2ch"] = (lambda: _stack([np.full(3000, 0.5), np.full(3000, -0.5)]), 2)
    out["nyquist_1ch"] = (lambda: _stack([ny]), 1)
    out["nyquist_2ch"] = (lambda: _stack([ny, -ny]), 2)
    out["square_full_scale_1ch"] = (lambda: _stack([sq]), 1)
    out["square_full_scale_2ch"] = (lambda: _stack([sq, sq2]), 2)
    # levels: the largest stays 1e4 below f32 overflow even times 2048
    for lv in LEVELS:
        out[f"level_x{lv}"] = (P(lambda lv: (signals.music_like(SR, 4000, 2, seed=7) * np.float32(float(lv))).astype(np.float32), lv), 2)
    for ch in (1, 2):
        out[f"music_{ch}ch"] = (P(signals.music_like, SR, 5000, ch, 11 + ch), ch)
    return out


def _edge_makers():
    out = {}
    for tag, v in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
        for ch in (1, 2):
            def make(v=v, ch=ch):
                x = signals.music_like(SR, 4000, ch, seed=20 + ch).copy()
                x[1500 * ch + ch - 1] = np.float32(v)       # sample-frame 1500 of the last channel: frames 1 and 2
                return x
            out[f"{tag}_{ch}ch"] = (make, ch)
    return out


_MAKERS = {**_makers(), **_edge_makers()}
CLIPS = list(_makers())                # the tight class's clips (through lossy_analyze, mdct_forward and the encoders)
TIGHT = CLIPS + [WINDOWS]
EDGE = list(_edge_makers())


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (interleaved f32 clip, channels)"""
    make, ch = _MAKERS[name]
    pcm = np.ascontiguousarray(make(), np.float32).reshape(-1)
    pcm.setflags(write=False)
    return pcm, ch


def impulse_windows():
    return np.eye(2048, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """-> (truth float64 [frames][ch][1024], skip [frames][ch], the oracle's own measure): what the oracle's f32 transform
    is off by on this case - the unit the device's error is counted in. O.lossy_analyze's coefficients for a clip,
    O.mdct_forward's for the impulse windows. Computed once per process, on the CPU."""
    if name == WINDOWS:
        win = impulse_windows()
        truth = transform(win)[:, None, :]
        got = np.stack([O.mdct_forward(w) for w in win])[:, None, :]
        skip = np.zeros((2048, 1), bool)
    else:
        pcm, ch = case(name)
        truth, skip = truth_of(pcm, ch)
        got = O.lossy_analyze(pcm, SR, ch, QUALITIES[0])["coeffs"]
    truth.setflags(write=False)
    return truth, skip, measure(got, truth, skip)


@functools.lru_cache(maxsize=1)
def floors():
    """(the largest worst, the largest rms) the oracle shows over the whole tight class: what the same f32 algorithm does on
    another input of the class. A case on which the oracle happens to be at half its usual error (dc, the tones) is not
    held below it"""
    ms = [yardstick(n)[2] for n in TIGHT]
    return max(m["worst"] for m in ms), max(m["rms"] for m in ms)


WORST_MARGIN, RMS_MARGIN = 2.0, 1.5     # tdec_ref's and test_mdct_forward_parity's: a second, independent f32 evaluation of the sum


def bounds(name):
    """(worst, rms) the device may show on the case: nothing fixed in advance, everything from the oracle's own error"""
    m = yardstick(name)[2]
    fw, fr = floors()
    return max(WORST_MARGIN * m["worst"], fw), max(RMS_MARGIN * m["rms"], fr)


def assert_tight(name, path, got):
    """`got`, the device's coefficients of the case along `path`, against the truth. Prints both sides' figures;
    -> (device, oracle) measures"""
    truth, skip, om = yardstick(name)
    assert np.asarray(got).shape == truth.shape, (name, path, np.asarray(got).shape, truth.shape)
    dm = measure(got, truth, skip)
    bw, br = bounds(name)
    f, c, k = dm["at"]
    rw = dm["worst"] / om["worst"] if om["worst"] > 0 else 0.0
    rr = dm["rms"] / om["rms"] if om["rms"] > 0 else 0.0
    print(f"{name:26s} {path:22s} worst: device {dm['worst']:.2e} oracle {om['worst']:.2e} ({rw:.2f} x) at frame {f} channel {c} bin {k}; "
          f"rms: device {dm['rms']:.2e} oracle {om['rms']:.2e} ({rr:.2f} x); {dm['frames']} frames")
    where = (f"{name} {path}: frame {f} channel {c} bin {k}: device {dm['got']!r}, f64 {dm['want']!r}, frame maximum {dm['scale']:.6e}; "
             f"device worst {dm['worst']:.3e} rms {dm['rms']:.3e}, oracle worst {om['worst']:.3e} rms {om['rms']:.3e}, "
             f"bounds {bw:.3e} / {br:.3e}")
    assert dm["finite"], where
    assert dm["zero_ok"], f"{name} {path}: (frame, channel) {dm['zero_at']} is silent in the reference and not on the device"
    assert dm["worst"] <= bw, where
    assert dm["rms"] <= br, where
    return dm, om


# --------------------------------------------------------------------------------------------------------- the kernels
KERNELS = {      # plan (lossy_model.plan_lossy, debug) -> the transform-bearing kernels of flo_amd/csrc/lossy_kernels.hip it launches
    "chain:Mono": "lossy_chain_kernel<1, false>",
    "chain:MonoExact": "lossy_chain_kernel<1, true>",
    "chain:Stereo": "lossy_chain_kernel<2, false>",
    "chain:StereoExact": "lossy_chain_kernel<2, true>",
    "frames:Mono1,Mono2": "lossy_frame_kernel<1, 1 and 2, false>",
    "frames:Mono1,Mono2Exact": "lossy_frame_kernel<1, 2, true>",
    "frames:Pair1,Pair2FromCoef": "lossy_frame2x_kernel<1> (and the hand-over to <2, true>)",
    "frames:Stereo1,Stereo2Exact": "lossy_frame_kernel<2, 1, false> and <2, 2, true>",
    "chain2q:Debug": "lossy_chain2q_kernel<false, 0xFFFF, true>",
    "frames:Multi1,Multi2": "lossy_frame_n_kernel<1 and 2, false>",
    "frames:Multi1,Multi2Exact": "lossy_frame_n_kernel<2, true>",
}


def plan_of(name, form, quality):
    """the plan row ctx.lossy_analyze of the case runs under force_path(form)"""
    pcm, ch = case(name)
    hops = hops_of(pcm.size // ch)
    return lossy_model.plan_lossy(force_path=form, ch=ch, n_clips=1, total_frames=hops, exact=quality >= 0.99, debug=True).split(" ")[0]


def reach(names=None):
    """{plan: [(case, form, quality)]} over the clips"""
    table = {}
    for n in (CLIPS + EDGE if names is None else names):
        for form in FORMS:
            for q in QUALITIES:
                table.setdefault(plan_of(n, form, q), []).append((n, form, q))
    return table
