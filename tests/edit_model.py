"""The model of the device's trimming, fades, padding and channel remixing (flo_batch_edit, flo_batch_active_range, flo_edit;
DESIGN 4.15), in numpy: the definition restated literally, the plan's tile geometry and tile classes, and the cases of the
device tests. The FMA steps are resample_model.fma (the exact f32 FMA, checked against rational arithmetic there); the
products and divisions are numpy's f32 `*` and `/`.

Definition. Clip i has N_i whole sample-frames of Cin channels. Output clip k (segment k) has T = pad_head + frames + pad_tail
frames of Cout channels. Output frame t, u = t - pad_head: +0.0 in every channel where u < 0, u >= frames or start + u >= N.
Otherwise, n = start + u: y[j] = x[n, j] without a matrix; with m[Cout][Cin], a = fl32(m[j][0] * x[n, 0]), then
a = fma(m[j][i], x[n, i], a) for i = 1 .. Cin - 1. w_in = fl32(u / fade_in) if u < fade_in; v = frames - 1 - u,
w_out = fl32(v / fade_out) if v < fade_out. Neither: out = y. One: out = fl32(y * w). Both: out = fl32(y * fl32(w_in * w_out)).
A frame is active when !(|x[n, c]| <= threshold) for some c; first = the smallest active frame, end = the largest plus one,
0 and 0 without one."""
import math

import numpy as np

import resample_model as R

TILE_FLOATS = 4096   # kEditTileFloats
THREADS = 256        # kEditThreads
MAX_MIX = 8          # kEditMaxMix
MAX_FADE = 1 << 24   # kEditMaxFade
INTERIOR, EDGE, FADED = 0, 1, 2
F32 = np.float32


def tile_frames(in_channels, out_channels):
    return (TILE_FLOATS // out_channels) & ~3


def seg(clip=0, start=0, frames=0, pad_head=0, pad_tail=0, fade_in=0, fade_out=0, reserved=0):
    return dict(clip=clip, start=start, frames=frames, pad_head=pad_head, pad_tail=pad_tail, fade_in=fade_in, fade_out=fade_out,
                reserved=reserved)


def out_frames(g):
    return g["pad_head"] + g["frames"] + g["pad_tail"]


def refusal(clip_frames, cin, lossy, segs, cout, matrix, size_max=2 ** 64 - 1):
    """the quantity the error message names, or None for a list of segments that is accepted"""
    if cout < 1:
        return "out_channels"
    if matrix is None and cout != cin:
        return "matrix"
    if matrix is not None:
        if cin > MAX_MIX:
            return "in_channels"
        if cout > MAX_MIX:
            return "out_channels"
        if not np.isfinite(np.asarray(matrix, F32)).all():
            return "matrix"
    if lossy and cout > 8:
        return "out_channels"
    most = size_max // 8 // cout
    for g in segs:
        if g["clip"] >= len(clip_frames):
            return "clip"
        if g.get("reserved", 0):
            return "reserved"
        if g["fade_in"] >= MAX_FADE or g["fade_in"] > g["frames"]:
            return "fade_in"
        if g["fade_out"] >= MAX_FADE or g["fade_out"] > g["frames"]:
            return "fade_out"
        if g["frames"] > most or g["pad_head"] + g["pad_tail"] > most - g["frames"]:
            return "frames"
    return None


def avail(g, n_src):
    return min(g["frames"], max(n_src - g["start"], 0))


def mix(X, matrix):
    """X [n, Cin] f32 -> [n, Cout]: the product of the first column, then the FMA chain over the others in order"""
    m = np.asarray(matrix, F32)
    out = np.empty((X.shape[0], m.shape[0]), F32)
    with np.errstate(all="ignore"):
        for j in range(m.shape[0]):
            a = m[j, 0] * X[:, 0]
            for i in range(1, m.shape[1]):
                a = R.fma(np.full(X.shape[0], m[j, i], F32), X[:, i], a)
            out[:, j] = a
    return out


def weights(g, n):
    """for frames u = 0 .. n - 1 of the cut: (w f32, applies bool)"""
    u = np.arange(n, dtype=np.int64)
    v = g["frames"] - 1 - u
    fin, fout = u < g["fade_in"], v < g["fade_out"]
    with np.errstate(all="ignore"):
        w_in = u.astype(F32) / F32(max(g["fade_in"], 1))
        w_out = v.astype(F32) / F32(max(g["fade_out"], 1))
        w = np.where(fin & fout, w_in * w_out, np.where(fin, w_in, w_out)).astype(F32)
    return w, fin | fout


def edit(x, cin, g, cout, matrix=None):
    """output clip of segment g cut from the interleaved f32 clip x: T * cout samples"""
    x = np.asarray(x, F32)
    n_src = x.size // cin
    X = x[:n_src * cin].reshape(n_src, cin)
    out = np.zeros((out_frames(g), cout), F32)
    n = avail(g, n_src)
    if n:
        cut = X[g["start"]:g["start"] + n]
        y = cut.copy() if matrix is None else mix(cut, np.asarray(matrix, F32).reshape(cout, cin))
        w, on = weights(g, n)
        with np.errstate(all="ignore"):
            y[on] = y[on] * w[on, None]
        out[g["pad_head"]:g["pad_head"] + n] = y
    return out.reshape(-1)


def tile_class(g, n_src, tile, F):
    T = out_frames(g)
    t0, t1 = tile * F, min(tile * F + F, T)
    lo, hi = g["pad_head"], g["pad_head"] + g["frames"]
    cls = INTERIOR
    if t0 < lo or t1 > hi:
        cls |= EDGE
    a, b = max(t0, lo) - lo, min(t1, hi) - lo
    if a < b:
        if b > avail(g, n_src):
            cls |= EDGE
        if a < g["fade_in"]:
            cls |= FADED
        if g["fade_out"] and b > g["frames"] - g["fade_out"]:
            cls |= FADED
    return cls


def tiles_of(frames, F):
    return -(-frames // F)


def tile_classes(g, n_src, F):
    return [tile_class(g, n_src, t, F) for t in range(tiles_of(out_frames(g), F))]


def threshold(db):
    return F32(10.0 ** (float(db) / 20.0))


def active_range(x, ch, thr):
    x = np.asarray(x, F32)
    n = x.size // ch
    with np.errstate(all="ignore"):
        act = ~(np.abs(x[:n * ch].reshape(n, ch)) <= F32(thr))
    idx = np.flatnonzero(act.any(axis=1))
    return (int(idx[0]), int(idx[-1]) + 1) if idx.size else (0, 0)


def ms_frames(ms, rate):
    return int(math.floor(float(ms) * rate / 1000.0 + 0.5))


def trim_segment(clip, first, end, n_src, rate, pre_ms=0.0, post_ms=0.0, fade_ms=0.0):
    """Batch.trim_silence's segment of one clip from its active range"""
    start, stop = (max(first - ms_frames(pre_ms, rate), 0), min(end + ms_frames(post_ms, rate), n_src)) if end else (0, 0)
    f = min(ms_frames(fade_ms, rate), stop - start, MAX_FADE - 1)
    return seg(clip, start, stop - start, fade_in=f, fade_out=f)


def same(got, want):
    """None when the two f32 arrays agree bit for bit (NaN on both sides matching by position), else a description"""
    got, want = np.asarray(got, F32).reshape(-1), np.asarray(want, F32).reshape(-1)
    if got.size != want.size:
        return "%d samples against %d" % (got.size, want.size)
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    d = np.flatnonzero(bad)
    return None if not d.size else "%d of %d samples differ, the first at %d: %r (%#x) against %r (%#x)" % (
        d.size, got.size, d[0], got[d[0]], got.view(np.uint32)[d[0]], want[d[0]], want.view(np.uint32)[d[0]])


# ---- the cases of the device tests ---------------------------------------------------------------------------------------
def _rows(cout, cin, seed):
    rng = np.random.default_rng(seed)
    m = rng.uniform(-1, 1, (cout, cin)).astype(F32)
    m.reshape(-1)[::3] *= F32(-1)
    return m


FORMS = [
    ("1to1_copy", 1, 1, None), ("2to2_copy", 2, 2, None), ("3to3_copy", 3, 3, None),
    ("2to1", 2, 1, np.array([[0.5, 0.5]], F32)), ("1to2", 1, 2, np.array([[1.0], [-0.75]], F32)),
    ("2to2_swap", 2, 2, np.array([[0, 1], [1, 0]], F32)), ("6to2", 6, 2, _rows(2, 6, 62)), ("8to1", 8, 1, _rows(1, 8, 81)),
    ("1to8", 1, 8, _rows(8, 1, 18)), ("8to8", 8, 8, _rows(8, 8, 88)), ("3to2", 3, 2, _rows(2, 3, 32)),
]
FLT_MAX = np.finfo(F32).max
SPECIALS = [-0.0, 1e-41, -3e-39, np.inf, -np.inf, np.nan, FLT_MAX, -FLT_MAX]


def source_lengths(F):
    return [0, 1, 3, F - 1, F, F + 1, 2 * F + 5]


def noise(n, ch, seed, F):
    """Gaussian noise with the special values planted at the tile edges and in the interior, walking over the channels"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n * ch) * 0.25).astype(F32).reshape(n, ch)
    spots = [0, 1, 2, F // 2, F - 2, F - 1, F, F + 1, F + F // 3, 2 * F - 1, 2 * F, n - 2, n - 1]
    for k, f in enumerate(spots):
        if 0 <= f < n:
            x[f, k % ch] = F32(SPECIALS[k % len(SPECIALS)])
    return x.reshape(-1)


def form_case(name):
    """(cin, cout, matrix, clips, segments): one batch of the form, its source clips of every length, and the cuts: every
    start with every length of cut, the pads walking through 0, 1 and F + 3 on either side; then several cuts of the longest
    clip that overlap"""
    _, cin, cout, matrix = next(f for f in FORMS if f[0] == name)
    F = tile_frames(cin, cout)
    lengths = source_lengths(F)
    clips = [noise(n, cin, 100 + i, F) for i, n in enumerate(lengths)]
    pads = (0, 1, F + 3)
    segs, seen, k = [], set(), 0
    for i, n in enumerate(lengths):
        for start in (0, 1, 2, 3, n - 1, n, n + 5):
            if start < 0:
                continue
            for frames in (0, 1, F, F + 1, n - start + 7):
                if frames < 0:
                    continue
                g = seg(i, start, frames, pads[k % 3], pads[(k // 3) % 3])
                key = tuple(sorted(g.items()))
                if key not in seen:
                    seen.add(key)
                    segs.append(g)
                    k += 1
    last = len(lengths) - 1
    segs += [seg(last, 5, F + 9), seg(last, 7, F + 9, 2, 0), seg(last, F - 3, F + 6, 0, 3), seg(last, 6, 2 * F - 1)]
    return cin, cout, matrix, clips, segs


def fade_case(F, cin):
    """(clips, segments) of the fade test: one source of 3F + 5 frames and one of F - 9"""
    clips = [noise(3 * F + 5, cin, 7, F), noise(F - 9, cin, 8, F)]
    segs = []
    for frames in (1, 2, 5, F, 2 * F + 3):
        for fi in (0, 1, 2, frames):
            for fo in (0, 1, 2, frames):
                if fi <= frames and fo <= frames:
                    segs.append(seg(0, 3, frames, fade_in=fi, fade_out=fo))
    segs += [
        seg(0, 0, 3 * F + 5, fade_in=3 * F + 5, fade_out=3 * F + 5),           # overlapping over the whole cut
        seg(0, 1, 2 * F, fade_in=F + 7, fade_out=F + 9),                        # overlapping in the middle, across a tile boundary
        seg(0, 2, 2 * F + 1, pad_head=5, pad_tail=F, fade_in=F - 5, fade_out=F + 1),   # fades that end on a tile boundary
        seg(0, 2, 2 * F + 1, pad_head=6, pad_tail=1, fade_in=F - 5, fade_out=F + 2),   # ... and one frame off it
        seg(1, 0, 2 * F, fade_in=40, fade_out=F + 200),                         # the fade-out lies past the source's end
        seg(1, F - 20, 64, pad_head=3, fade_in=64, fade_out=64),                # most of the cut lies past the end
    ]
    return clips, segs
