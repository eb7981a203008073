"""The split fold of the stereo chain encode (fold_carry_2) against the whole fold (fold_2), as an f32 numpy model.

fold_2 makes row r's (re, im) from one product per half-frame: the new half gives the b-part, the old half the a-part.
fold_carry_2 computes a half's a-parts when the half is new and carries them (8 values per lane and channel instead of 16
samples) into the next frame's fold. The model restates both forms with the same rounding steps (a product rounded to f32,
then one fused multiply-add) and walks a clip's halves through them: every (zr, zi) of every frame must agree bit for bit,
the first frame's carry being the a-parts of the pre-roll's zeros. The window and the twiddles are any f32 values of the
right signs (a sine window, unit twiddles): the identity does not depend on them.
"""
import numpy as np
import pytest

F = np.float32
LANES = np.arange(64)


def fma(a, b, c):
    # one rounding: the f32 product is exact in f64; the f64 sum is rounded once more, identically in both forms
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def mul(a, b):
    return (a * b).astype(F)


def rows(half):
    """half: 1024 samples of one channel -> (even, odd) samples of (row, lane) as load_half_fast_2 hands them out"""
    he, ho = np.empty((8, 64), F), np.empty((8, 64), F)
    for r in range(8):
        i = LANES + 64 * (r & 3)
        he[r], ho[r] = (half[512 + 2 * i], half[511 - 2 * i]) if r < 4 else (half[2 * i], half[1023 - 2 * i])
    return he, ho


def tables():
    n = np.arange(2048, dtype=np.float64)
    window = np.sin(np.pi * (n + 0.5) / 2048).astype(F)
    m = np.arange(512, dtype=np.float64)
    ang = -2 * np.pi * (m + 0.125) / 2048
    tw = np.stack([np.cos(ang), np.sin(ang)], 1).astype(F)
    w = np.empty((8, 64, 4), F)
    for r in range(8):
        i = LANES + 64 * (r & 3)
        eo, oo = (512 + 2 * i, 511 - 2 * i) if r < 4 else (2 * i, 1023 - 2 * i)
        w[r] = np.stack([window[eo], window[oo], window[1024 + eo], window[1024 + oo]], 1)
    t = np.stack([tw[LANES + 64 * r] for r in range(8)])     # (row, lane, (wx, wy))
    return w, t


def rotate(re, im, t):
    zr = fma(-im, t[:, 1], -mul(re, t[:, 0]))
    zi = fma(re, t[:, 1], -mul(im, t[:, 0]))
    return zr, zi


def b_part(he, ho, w):
    return fma(-ho, w[:, 3], -mul(he, w[:, 2]))


def a_part(r, he, ho, w):
    return fma(ho, w[:, 1], -mul(he, w[:, 0])) if r < 4 else fma(-ho, w[:, 1], mul(he, w[:, 0]))


def fold_whole(old, new, w, t):
    (ae, ao), (be, bo) = rows(old), rows(new)
    out = []
    for r in range(8):
        a, b = a_part(r, ae[r], ao[r], w[r]), b_part(be[r], bo[r], w[r])
        out.append(rotate(b, a, t[r]) if r < 4 else rotate(a, b, t[r]))
    return out


def fold_split(new, acar, w, t):
    ne, no = rows(new)
    out = []
    for r in range(8):
        b = b_part(ne[r], no[r], w[r])
        out.append(rotate(b, acar[r], t[r]) if r < 4 else rotate(acar[r], b, t[r]))
        acar[r] = a_part(r, ne[r], no[r], w[r])
    return out


def clips():
    rng = np.random.default_rng(7)
    noise = rng.uniform(-1, 1, 5 * 1024).astype(F)
    special = noise.copy()
    special[[0, 1023, 1024, 2047, 2100]] = [np.inf, -np.inf, 0.0, -0.0, np.inf]
    return {"noise": noise, "plus zero": np.zeros(3 * 1024, F), "minus zero": np.full(3 * 1024, -0.0, F),
            "dc": np.full(3 * 1024, 1.0, F), "inf and signed zeros": special}


@pytest.mark.parametrize("name", list(clips()))
def test_split_fold_equals_whole_fold_bit_for_bit(name):
    x = clips()[name]
    w, t = tables()
    halves = [np.zeros(1024, F)] + [x[i:i + 1024] for i in range(0, x.size, 1024)]     # the pre-roll, then the clip
    zero = np.zeros(64, F)
    acar = [a_part(r, zero, zero, w[r]) for r in range(8)]
    for h in range(1, len(halves)):
        whole = fold_whole(halves[h - 1], halves[h], w, t)
        split = fold_split(halves[h], acar, w, t)
        for r in range(8):
            for part, (a, b) in zip("ri", zip(whole[r], split[r])):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, "frame", h - 1, "row", r, "z" + part)


def test_the_carry_of_the_pre_roll_is_plus_zero():
    # the two products of an a-part of zeros are zeros of opposite sign for either sign of a finite window, and their sum
    # rounds to +0: the kernel's fold_carry_init_2 (fold_2's expressions over zeros) starts every clip from +0
    w, _ = tables()
    zero = np.zeros(64, F)
    for r in range(8):
        for win in (w[r], -w[r]):
            assert np.array_equal(a_part(r, zero, zero, win).view(np.uint32), zero.view(np.uint32))
