"""The model of the device's mixing and concatenation (flo_batch_mix, flo_mix), in numpy: the definition restated
literally, the class of a part on a tile, the refusals, and the cases of the device tests. The FMA is resample_model.fma
(the exact f32 FMA, checked against rational arithmetic there); the fade weights are edit_model.weights (f32 `/` and `*`).

Definition. Sources are batches of clips of C channels; clip i has N_i whole sample-frames. Output clip k has T_k frames. Part
p of clip k is live on output frame t when at <= t < at + frames, t < T_k and start + (t - at) < N. u = t - at,
v = frames - 1 - u; w_in = fl32(u / fade_in) if u < fade_in, w_out = fl32(v / fade_out) if v < fade_out, w their f32 product
where both apply. k_p = gain where no fade applies, else fl32(gain * w). Output sample (t, c): a = +0.0, then
a = fma(k_p, x_p[start + u, c], a) for every live part of the clip in list order."""
import numpy as np

import edit_model as E
import resample_model as R

F32 = np.float32
NONE, WHOLE, PARTIAL = 0, 1, 2   # kMixNone, kMixWhole, kMixPartial
MAX_FADE = E.MAX_FADE
FLT_MAX = np.finfo(F32).max
GAINS = (1.0, -1.0, 0.0, 0.5, 1e-3)


def tile_frames(ch):
    return E.tile_frames(ch, ch)


def part(out=0, clip=0, batch=0, start=0, frames=0, at=0, gain=1.0, fade_in=0, fade_out=0):
    return dict(out=out, batch=batch, clip=clip, start=start, frames=frames, at=at, gain=gain, fade_in=fade_in, fade_out=fade_out)


def refusal(src_clip_frames, ch, n_out, out_frames, parts, size_max=2 ** 64 - 1):
    """the quantity the error message names, or None for a list that is accepted. src_clip_frames[b]: the frames of every
    clip of source b (the sources here share context, rate and channels)"""
    if not src_clip_frames:
        return "n_srcs"
    if len(parts) >= 1 << 32:
        return "n_parts"
    most = size_max // 8 // ch
    if any(t > most for t in out_frames):
        return "out_frames"
    last = 0
    for g in parts:
        if g["out"] >= n_out:
            return "out"
        if g["out"] < last:
            return "out"
        last = g["out"]
        if g["batch"] >= len(src_clip_frames):
            return "batch"
        if g["clip"] >= len(src_clip_frames[g["batch"]]):
            return "clip"
        if g["fade_in"] >= MAX_FADE or g["fade_in"] > g["frames"]:
            return "fade_in"
        if g["fade_out"] >= MAX_FADE or g["fade_out"] > g["frames"]:
            return "fade_out"
        if not np.isfinite(F32(g["gain"])):
            return "gain"
        if g["at"] + g["frames"] >= 1 << 64:
            return "at + frames"
        if g["start"] + g["frames"] >= 1 << 64:
            return "start + frames"
    return None


def live_range(g, n_src, T):
    """(lo, hi): the part is live on output frames [lo, hi), hi <= lo when on none"""
    avail = min(g["frames"], max(n_src - g["start"], 0))
    return g["at"], min(g["at"] + avail, T)


def _subnormal(a):
    """whether any value of the f32 array is a non-zero subnormal (zero wraps round to 0xFFFFFFFF)"""
    a = np.ascontiguousarray(a, F32)
    return bool((((a.view(np.uint32) & np.uint32(0x7FFFFFFF)) - np.uint32(1)) < np.uint32(0x007FFFFF)).any())


def coefficients(g, n):
    """k_p of frames u = 0 .. n - 1 of the part, f32"""
    w, on = E.weights(g, n)
    with np.errstate(all="ignore"):
        return np.where(on, F32(g["gain"]) * w, F32(g["gain"])).astype(F32)


def mix_clip(sources, ch, parts, T, strict=False, counts=None):
    """output clip of T frames summed from `parts` (those of this clip, in list order); sources[b][i]: interleaved f32 clips.
    strict: assert that no coefficient and no partial sum is a non-zero subnormal, so that a device that flushes them
    computes the same bits. counts (an int array of T entries, optional) receives the number of parts live on every frame"""
    acc = np.zeros((T, ch), F32)
    for g in parts:
        x = np.asarray(sources[g["batch"]][g["clip"]], F32)
        n_src = x.size // ch
        lo, hi = live_range(g, n_src, T)
        if hi <= lo:
            continue
        n = hi - lo
        X = x[:n_src * ch].reshape(n_src, ch)[g["start"]:g["start"] + n]
        k = coefficients(g, n)
        acc[lo:hi] = R.fma(np.repeat(k, ch).reshape(n, ch), X, acc[lo:hi])
        if counts is not None:
            counts[lo:hi] += 1
        if strict:
            assert not _subnormal(k) and not _subnormal(acc[lo:hi]), ("a subnormal in a bit-for-bit case", g)
    return acc.reshape(-1)


def mix(sources, ch, parts, out_frames, strict=False):
    """every output clip of the list"""
    return [mix_clip(sources, ch, [g for g in parts if g["out"] == k], T, strict) for k, T in enumerate(out_frames)]


def part_in_tile(g, n_src, T, t0, nf):
    """mix_part_in_tile restated frame by frame: NONE when the part is live on no frame of [t0, t0 + nf), WHOLE when it is
    live on every one and none lies in a fade, else PARTIAL"""
    lo, hi = live_range(g, n_src, T)
    live = [lo <= t < hi for t in range(t0, t0 + nf)]
    if not any(live):
        return NONE
    if not all(live):
        return PARTIAL
    _, on = E.weights(g, t0 + nf - g["at"])
    return PARTIAL if on[t0 - g["at"]:].any() else WHOLE


def tile_classes(g, n_src, T, F):
    return [part_in_tile(g, n_src, T, t0, min(F, T - t0)) for t0 in range(0, T, F)]


def same(got, want):
    return E.same(got, want)


# ---- the cases of the device tests ---------------------------------------------------------------------------------------
def source_lengths(F):
    return [0, 1, 3, F - 1, F, F + 1, 2 * F + 5]


def noise(n, ch, seed, F):
    """Gaussian noise with -0.0, the infinities, NaN and +-FLT_MAX planted at the tile edges, walking over the channels; no
    denormals"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n * ch) * 0.25).astype(F32).reshape(n, ch)
    x[np.abs(x) < F32(1e-6)] = F32(0.125)
    specials = [-0.0, np.inf, -np.inf, np.nan, FLT_MAX, -FLT_MAX]
    for k, f in enumerate([0, 1, F - 1, F, F + 1, 2 * F - 1, 2 * F, n - 1]):
        if 0 <= f < n:
            x[f, k % ch] = F32(specials[k % len(specials)])
    return x.reshape(-1)


def plain(n, ch, seed):
    """noise without special values, away from zero"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n * ch) * 0.25).astype(F32)
    x[np.abs(x) < F32(1e-6)] = F32(0.125)
    return x


def many_parts(out, n, F, long_clip):
    """n parts of one output of 3F frames: parts 0, 64 and 129 (those there are) lie on tile 1, every other part is five
    frames somewhere on tile 0, and tile 2 has none"""
    parts = []
    for j in range(n):
        if j in (0, 64, 129):
            parts.append(part(out, long_clip, start=j % 7, frames=F - (j % 3), at=F + (j % 3), gain=(1.0, 0.5, -0.25)[j % 3]))
        else:
            parts.append(part(out, long_clip if j % 2 == 0 else 0, batch=j % 2, start=j, frames=5, at=(3 * j) % (F - 5), gain=GAINS[j % 5]))
    return parts


def device_case(ch):
    """(sources, parts, out_frames) of one batch of outputs for `ch` channels. sources[0] are the clips of a lossless batch,
    sources[1] those of a lossy one; no clip is longer than 3F + 5 frames"""
    F = tile_frames(ch)
    lengths = source_lengths(F)
    a = [noise(n, ch, 200 + i, F) for i, n in enumerate(lengths)]
    b = [noise(2 * F + 5, ch, 300, F), plain(F + 1, ch, 301), noise(3 * F + 5, ch, 302, F)]
    big = len(lengths) - 1   # clip 2F + 5 of either source
    outs = []                # (T, parts without `out`)
    ats = (0, 1, 2, 3, F - 1, F, F + 1)
    seen, k = set(), 0
    for i, n in enumerate(lengths):
        for start in (0, 1, 2, 3, n - 1, n, n + 5):
            if start < 0:
                continue
            for frames in (0, 1, F, F + 1, n - start + 7):
                if frames < 0 or (i, start, frames) in seen:
                    continue
                seen.add((i, start, frames))
                at = ats[k % 7]
                end = at + frames
                T = min((end, end + 3, max(end - 2, 0), end + F, 0)[(k // 7) % 5], 3 * F + 5)   # exact, a gap behind, cut short, a silent tile, empty
                outs.append((T, [part(0, i, 0, start, frames, at, GAINS[k % 5])]))
                k += 1
    outs += [(0, []), (F + 3, []), (3, [])]                                                    # no part at all
    outs.append((2 * F + 9, [part(0, 2, 0, 0, 3, 4), part(0, big, 0, 5, 40, F + 5, 0.5), part(0, 1, 0, 0, 1, 2 * F + 8)]))   # gaps
    outs.append((2 * F, [part(0, big, 0, 0, F + 9, 0, 0.5)]))                                 # whole on tile 0, partial on tile 1
    for d in range(4):                                                                         # every source alignment
        outs.append((2 * F, [part(0, big, 0, d, 2 * F, 0, 1.0), part(0, 0, 1, 4 + d, F, F, -1.0)]))
    for frames in (1, 2, 5, F, 2 * F + 3):                                                     # fades
        for fi in (0, 1, 2, frames):
            for fo in (0, 1, 2, frames):
                if fi > frames or fo > frames:
                    continue
                outs.append((frames + 6, [part(0, big, 0, 3, frames, 2 + (fi + fo) % 3, GAINS[(fi + fo) % 5], fi, fo)]))
    outs += [
        (2 * F + 5, [part(0, big, 0, 0, 2 * F + 5, 0, 1.0, 2 * F + 5, 2 * F + 5)]),           # overlapping over the whole part
        (2 * F + 1, [part(0, big, 0, 1, 2 * F, 1, 0.5, F + 7, F + 9)]),                         # overlapping across a tile boundary
        (3 * F, [part(0, big, 0, 2, 2 * F + 1, 5, 1.0, F - 5, F + 1)]),                         # fades that end on a tile boundary
        (3 * F, [part(0, big, 0, 2, 2 * F + 1, 6, -1.0, F - 5, F + 2)]),                        # ... and one frame off it
        (2 * F, [part(0, 3, 0, 0, 2 * F, 0, 1.0, 40, F + 200)]),                                # the fade-out lies past the source's end
        (F, [part(0, 3, 0, F - 20, 64, 3, 1.0, 64, 64)]),                                       # most of the part lies past the end
    ]
    outs += [
        (2 * F + 5, [part(0, big, 0, 0, 2 * F + 5), part(0, 0, 1, 0, 2 * F + 5, 0, 0.5)]),                  # two parts, two batches, whole tiles
        (2 * F + 5, [part(0, big, 0, 0, 2 * F + 5), part(0, big, 0, 0, 2 * F + 5, F - 1, 0.5)]),   # an echo of the clip on itself
        (3 * F, [part(0, big, 0, 0, 2 * F, 0, 1.0, 0, F), part(0, 2, 1, 0, 2 * F, F, 1.0, F, 0),    # a crossfade and a bed under both
                 part(0, 2, 1, 7, 3 * F - 2, 0, 1e-3)]),
        (F + 9, [part(0, big, 0, 5, 9, F, 1.0), part(0, big, 0, 0, 9, 3, -1.0), part(0, 4, 0, 0, F + 9, 0, 0.5)]),   # list order against time order
        (40, [part(0, big, 0, 3, 40, 0, 1.0), part(0, 1, 1, 0, 40, 0, 0.5), part(0, big, 0, 3, 40, 0, -1.0)]),       # the order of summation shows
    ]
    for n in (63, 64, 65, 130):
        outs.append((3 * F, many_parts(0, n, F, big)))
    longest = MAX_FADE - 1
    outs.append((lengths[5] + 3, [part(0, 5, 0, 0, longest, 0, 1.0, longest, longest), part(0, 5, 0, 1, longest, 2, 0.5, 0, longest)]))
    parts, T = [], []
    for kk, (t, ps) in enumerate(outs):
        T.append(t)
        parts += [dict(g, out=kk) for g in ps]
    return [a, b], parts, T


def alone(sources, parts):
    """(clips, parts) of one output taken alone through flo_mix: the clips its parts name as one source, batch and out 0"""
    index, clips, mine = {}, [], []
    for g in parts:
        key = (g["batch"], g["clip"])
        if key not in index:
            index[key] = len(clips)
            clips.append(sources[g["batch"]][g["clip"]])
        mine.append(dict(g, out=0, batch=0, clip=index[key]))
    return clips, mine
