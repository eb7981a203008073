"""An exact, inspectable restatement of the lossless encoder's decisions, and the shared list of path cases.

`frame_model` restates, for one frame slice of float32 PCM, everything oracle/lossless.c and oracle/core.c decide:
the converted integers, the silence flag, the mid/side choice, and for every candidate (raw, fixed 0-4, LPC 5-max)
whether it is valid (and why not), its coefficients, shift, residuals, Rice parameter and exact byte size, then the
winner under the reference's candidate order and strict `<`, and the frame type. It uses numpy int64 and Python floats;
Python floats are IEEE doubles without contraction, so Levinson-Durbin in the reference's operation order is exact.

On top of that it derives the DEVICE-side path predicates from the constants lossless_kernels.hip documents, so that a
test can say which hand-optimised path an input takes:

  tiles      a tile is 4096 samples (256 runs of 16); it is composed in LDS ("staged") unless
             lead + tile_bits > 32 * 4096 = 131072, where lead = (8 * (res_pos & 3) + bits of earlier tiles) & 31
  long code  a code with q + 1 + k > 32 (leaves the one-field fast path of the staged writer); q == 255 (the unary cap)
  window     ll_analyze guesses the Rice parameter of an LPC order from Levinson's error,
             kw0 = f(bitlen(sqrt(err / n) * 0.70710678)), counts sizes for k in kw0..kw0+2 and runs a third sweep only
             when d = k - kw0 falls outside {0, 1, 2}. The device takes that sqrt in f64; a case counts as outside the
             window only if d is the same with the guessed mean scaled by 0.99 and by 1.01 (`d_robust`)
  FULL       runs with i0 >= 16 and i0 + 16 <= n skip every bounds test and the warm-up rule
  res_pos&3  byte alignment of each channel's residual stream inside the DATA chunk (sets bit0 and lead)

Paths not reached by any case (the reach test allows only these two names in that list):

  gamma     |gamma| >= 1 in Levinson, and
  err       |error| < 1e-10. Families tried, each at order 12 with n from 13 to 40 (200,000 draws): sequences over
            {-1, 0, 1}, a constant with one sample moved, periodic patterns of period 2-6 over {-2..2}, rounded sines of
            amplitude 3; and on long planes: integer sines, sums of up to six sines, the same with clicks. The lag sums
            are those of the plane padded with zeros, a positive definite Toeplitz matrix, so |gamma| < 1 in exact
            arithmetic and error = det(T_k+1) / det(T_k); the smallest error met was 1.14 (thirteen samples, two -1).
            In f64 neither return was met either.

`max_res` (an LPC residual above 1,000,000 that Levinson accepted) IS reached, by `max_res_discard_l5`: five full-scale
sines at 192 kHz make an order-8 predictor whose coefficients sum to 21.6 in magnitude; three samples placed against the
signs of its largest taps, on a mid plane (L = R, so 17 bits), give a residual of 1,052,996.
"""
import math
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

TILE = 4096
RUN = 16
STAGE_BITS = 32 * 4096
LEVEL_ORDER = (0, 2, 4, 4, 6, 8, 8, 10, 12, 12)
NOT_REACHED_ALLOWED = ("gamma", "err")


# ------------------------------------------------------------------------------------------------ scalar rules
def f32_to_i32(x) -> np.ndarray:
    """core.c flo_o_f32_to_i32 over an array: f32 multiply, clamp (NaN passes through), NaN -> 0, truncation."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = x * np.float32(32767.0)
        v = np.where(v < np.float32(-32768.0), np.float32(-32768.0), v)
        v = np.where(v > np.float32(32767.0), np.float32(32767.0), v)
        v = np.where(np.isnan(v), np.float32(0.0), v)
    return np.trunc(v).astype(np.int64)


def is_silent(x) -> bool:
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return bool(np.all(np.abs(x) < np.float32(1e-7)))


def wrap32(v):
    v = np.asarray(v, np.int64)
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def zigzag(r) -> np.ndarray:
    r = np.asarray(r, np.int64)
    return ((r << 1) ^ (r >> 31)) & 0xFFFFFFFF


def rice_k(res) -> int:
    """core.c flo_o_estimate_rice_parameter_i32."""
    res = np.asarray(res, np.int64)
    n = res.size
    if n == 0:
        return 4
    a = np.abs(res)
    max_abs = int(a.max())
    if max_abs == 0:
        return 0
    mu = 2 * max_abs
    min_k = max(mu.bit_length() - 8, 0) if mu > 255 else 0
    mean = (int(a.sum()) // n) & 0xFFFFFFFF
    k = max(min_k, mean.bit_length())
    return min(k, 15)


def code_bits(res, k) -> np.ndarray:
    """length of every Rice code: min(u >> k, 255) + 1 + k"""
    return np.minimum(zigzag(res) >> k, 255) + 1 + k


def fixed_residuals(s, order) -> np.ndarray:
    """lossless.c flo_o_fixed_predictor_residuals: position i < order uses order i."""
    s = np.asarray(s, np.int64)
    n = s.size
    binom = ([1], [1, -1], [1, -2, 1], [1, -3, 3, -1], [1, -4, 6, -4, 1])
    out = np.zeros(n, np.int64)
    for i in range(n):
        if i >= order:
            break
        out[i] = sum(c * int(s[i - j]) for j, c in enumerate(binom[i]))
    if n > order:
        acc = np.zeros(n - order, np.int64)
        for j, c in enumerate(binom[order]):
            acc += c * s[order - j:n - j]
        out[order:] = acc
    return wrap32(out)


def autocorr(s, order) -> List[int]:
    s = np.asarray(s, np.int64)
    n = s.size
    return [int(np.dot(s[lag:], s[:n - lag])) if lag < n else 0 for lag in range(order + 1)]


def _round_half_away(v: float) -> float:
    t = math.trunc(v)
    if abs(v - t) >= 0.5:
        t += 1 if v > 0 else -1
    return float(t)


def levinson(ac: List[int], order: int):
    """lossless.c flo_o_levinson_durbin_int, operation for operation. -> dict(ok, reason, coeffs, shift, err)"""
    if ac[0] == 0:
        return dict(ok=False, reason="ac0")
    coeffs = [0.0] * order
    error = float(ac[0])
    for i in range(order):
        lam = float(ac[i + 1])
        for j in range(i):
            lam -= coeffs[j] * float(ac[i - j])
        if abs(error) < 1e-10:
            return dict(ok=False, reason="err")
        gamma = lam / error
        if abs(gamma) >= 1.0:
            return dict(ok=False, reason="gamma")
        new = coeffs[:]
        new[i] = gamma
        for j in range(i):
            new[j] = coeffs[j] - gamma * coeffs[i - 1 - j]
        coeffs = new
        error *= 1.0 - gamma * gamma
    max_coeff = 0.0
    for c in coeffs:
        max_coeff = max(max_coeff, abs(c))
    if max_coeff == 0.0 or not math.isfinite(max_coeff):
        return dict(ok=False, reason="max_coeff")
    quot = float(1 << 30) / max_coeff
    fl = math.floor(math.log2(quot)) if math.isfinite(quot) else 255
    shift = min(max(min(fl, 255), 0), 15)
    scale = float(1 << shift)
    q = []
    for c in coeffs:
        v = _round_half_away(c * scale)
        q.append(int(max(min(v, 2147483647.0), -2147483648.0)))
    return dict(ok=True, reason=None, coeffs=q, shift=shift, err=error)


def lpc_residuals(s, coeffs, shift) -> np.ndarray:
    """lossless.c flo_o_calc_residuals_int: warm-up copies, i64 dot, arithmetic shift, truncating cast, wrapping sub."""
    s = np.asarray(s, np.int64)
    n, order = s.size, len(coeffs)
    out = s.copy()
    if n > order:
        pred = np.zeros(n - order, np.int64)
        for j, c in enumerate(coeffs):
            pred += int(c) * s[order - j - 1:n - j - 1]
        pred = wrap32(pred >> shift)
        out[order:] = wrap32(s[order:] - pred)
    return out


def guess_kw0(err: float, n: int, scale: float = 1.0) -> int:
    """ll_analyze's guess of the first Rice parameter of its three-wide window, from Levinson's error."""
    mean = math.sqrt(err / float(n)) * 0.70710678 * scale if err > 0.0 else 0.0
    mi = int(mean) if mean < 4.0e9 else 0xFFFFFFFF
    kg = min(mi.bit_length(), 15)
    return 13 if kg >= 14 else (kg - 1 if kg > 0 else 0)


# ------------------------------------------------------------------------------------------------ records
@dataclass
class Candidate:
    name: str                      # "raw", "fixed0".."fixed4", "lpc5".."lpc12"
    kind: int                      # 0 raw, 1 fixed, 2 LPC
    order: int
    valid: bool = True
    reason: Optional[str] = None   # ac0 / err / gamma / max_coeff / n<=order / max_res
    coeffs: List[int] = field(default_factory=list)
    shift: int = 0
    residuals: Optional[np.ndarray] = None
    k: int = 0
    size: int = 0                  # exact payload bytes
    bits: int = 0
    kw0: Optional[int] = None      # device: first parameter of the window (LPC candidates Levinson accepted)
    d: Optional[int] = None        # device: k - kw0 (LPC candidates that stayed valid)
    d_robust: bool = False         # d unchanged with the guessed mean scaled by 0.99 and 1.01


@dataclass
class ChannelModel:
    ints: np.ndarray               # the plane that is coded (mid or side when use_ms)
    n: int
    cands: List[Candidate]
    winner: Candidate
    order_used: int                # what encode_channel_int returns: 0 for raw and for fixed 0
    # device predicates of the winner's bit stream (filled by file_model once res_pos is known)
    res_pos: int = 0
    tiles: List[dict] = field(default_factory=list)
    long_code: bool = False        # some code of a staged tile has q + 1 + k > 32
    capped: bool = False           # some code has q == 255
    full_runs: int = 0

    def cand(self, name) -> Candidate:
        return next(c for c in self.cands if c.name == name)


@dataclass
class FrameModel:
    silent: bool
    use_ms: bool
    frame_samples: int
    frame_type: int                # 0 silence, 254 raw, else the level's order
    flags: int
    channels: List[ChannelModel]
    planes: List[np.ndarray]       # converted integers per channel BEFORE mid/side (what a decoder must return)
    byte_off: int = 0
    size: int = 0


def channel_model(s, level: int) -> ChannelModel:
    s = np.asarray(s, np.int64)
    n = s.size
    max_order = LEVEL_ORDER[min(level, 9)]
    cands: List[Candidate] = []
    if n == 0:
        w = Candidate("empty", 1, 0, residuals=np.zeros(0, np.int64))
        return ChannelModel(s, 0, [w], w, 0)
    raw = Candidate("raw", 0, 0, size=2 * n, bits=16 * n)
    cands.append(raw)
    for o in range(min(max_order, 4) + 1):
        r = fixed_residuals(s, o)
        k = rice_k(r)
        bits = int(code_bits(r, k).sum())
        cands.append(Candidate(f"fixed{o}", 1, o, residuals=r, k=k, bits=bits, size=(bits + 7) >> 3))
    if level >= 3 and max_order > 4:
        ac = autocorr(s, max_order)
        for o in range(5, max_order + 1):
            c = Candidate(f"lpc{o}", 2, o)
            cands.append(c)
            if n <= o:
                c.valid, c.reason = False, "n<=order"
                continue
            lv = levinson(ac[:o + 1], o)
            if not lv["ok"]:
                c.valid, c.reason = False, lv["reason"]
                continue
            c.coeffs, c.shift = lv["coeffs"], lv["shift"]
            c.kw0 = guess_kw0(lv["err"], n)
            r = lpc_residuals(s, c.coeffs, c.shift)
            c.residuals = r
            if int(np.abs(r).max()) > 1000000:
                c.valid, c.reason = False, "max_res"
                continue
            c.k = rice_k(r)
            c.bits = int(code_bits(r, c.k).sum())
            c.size = (c.bits + 7) >> 3
            c.d = c.k - c.kw0
            c.d_robust = (c.k - guess_kw0(lv["err"], n, 0.99) == c.d) and (c.k - guess_kw0(lv["err"], n, 1.01) == c.d)
    best, winner = None, None
    for c in cands:                       # raw, fixed 0..4, LPC 5..max: strictly smaller wins
        if c.valid and (best is None or c.size < best):
            best, winner = c.size, c
    cm = ChannelModel(s, n, cands, winner, winner.order)
    cm.full_runs = sum(1 for i0 in range(16, n, RUN) if i0 + RUN <= n)
    return cm


def frame_model(x, ch: int, level: int) -> FrameModel:
    """One frame slice (interleaved float32, every channel) -> the reference's decisions (lossless.c encode_frame)."""
    x = np.asarray(x, np.float32)
    ns = x.size // ch
    if is_silent(x):
        return FrameModel(True, False, ns, 0, 0, [], [np.zeros(ns, np.int64) for _ in range(ch)])
    planes = [f32_to_i32(x[c::ch]) for c in range(ch)]
    coded = planes
    use_ms = False
    if ch == 2:
        m = min(planes[0].size, planes[1].size)
        l, r = planes[0][:m], planes[1][:m]
        var_l, var_r, var_s = int(np.dot(l, l)), int(np.dot(r, r)), int(np.dot(l - r, l - r))
        use_ms = var_s < (var_l + var_r) // 2
        if use_ms:
            coded = [l + r, l - r]
    chans = [channel_model(p, level) for p in coded]
    all_raw = all(c.order_used == 0 for c in chans)
    max_order = LEVEL_ORDER[min(level, 9)]
    ft = 254 if all_raw else (max_order if 1 <= max_order <= 12 else 8)
    return FrameModel(False, use_ms, ns, ft, 1 if use_ms else 0, chans, planes)


def _tiles(cm: ChannelModel):
    """Device view of the winner's bit stream: per tile the bit count, lead and the writer that takes it."""
    w = cm.winner
    cm.tiles, cm.long_code, cm.capped = [], False, False
    if w.kind == 0 or cm.n == 0:
        return
    cb = code_bits(w.residuals, w.k)
    q = np.minimum(zigzag(w.residuals) >> w.k, 255)
    cm.capped = bool((q == 255).any())
    tile_bit = 0
    for t0 in range(0, cm.n, TILE):
        bits = int(cb[t0:t0 + TILE].sum())
        lead = (8 * (cm.res_pos & 3) + tile_bit) & 31
        staged = lead + bits <= STAGE_BITS
        long_here = bool((cb[t0:t0 + TILE] > 32).any())
        if staged and long_here:
            cm.long_code = True
        cm.tiles.append(dict(t0=t0, bits=bits, lead=lead, staged=staged, long_code=long_here))
        tile_bit += bits


def file_model(pcm, sr: int, ch: int, level: int) -> List[FrameModel]:
    """Every frame of a clip, with the byte layout of the DATA chunk (ll_layout) and the packer's path predicates."""
    pcm = np.asarray(pcm, np.float32)
    level = min(level, 9)
    total = pcm.size // ch
    nf = (total + sr - 1) // sr
    frames, off = [], 0
    for fi in range(nf):
        fm = frame_model(pcm[fi * sr * ch:min((fi + 1) * sr * ch, pcm.size)], ch, level)
        fm.byte_off = off
        pos = off + 6
        for c in range(ch):
            if fm.silent:
                pos += 4
                continue
            cm = fm.channels[c]
            w = cm.winner
            head = 0
            if fm.frame_type != 254:
                head = 1 + 4 * (w.order if w.kind == 2 else 0) + 1 + 1 + (0 if w.kind == 0 else 1)
            cm.res_pos = pos + 4 + head
            _tiles(cm)
            pos += 4 + head + w.size
        fm.size = pos - off
        off = pos
        frames.append(fm)
    return frames


def expected_ints(frames: List[FrameModel], ch: int) -> np.ndarray:
    """What a correct decoder returns for the file: the converted integers, interleaved, frame_samples per frame.
    Mid/side frames come back through (m + s) / 2, (m - s) / 2, which is exact for m = l + r, s = l - r."""
    out = []
    for fm in frames:
        a = np.zeros((fm.frame_samples, ch), np.int64)
        for c in range(ch):
            p = fm.planes[c][:fm.frame_samples]
            a[:p.size, c] = p
        out.append(a.reshape(-1))
    return np.concatenate(out).astype(np.int32) if out else np.zeros(0, np.int32)


def undecodable(frames: List[FrameModel]) -> bool:
    """The reference's own quirk: a Raw-typed frame whose channel holds Rice bytes (fixed order 0 won) is read back as
    raw PCM. So is a raw winner on a mid plane that left 16 bits (`s as i16` wraps). Decided from the model's frame
    type, channel kinds and integers only, never from an outcome."""
    return any((fm.frame_type == 254 and any(c.winner.kind != 0 for c in fm.channels)) or
               any(c.winner.kind == 0 and c.n and (c.ints.max() > 32767 or c.ints.min() < -32768) for c in fm.channels)
               for fm in frames if not fm.silent)


def paths(frames: List[FrameModel], level: int) -> set:
    """Names of the device paths the model says this clip takes (the vocabulary of the reach table)."""
    p = set()
    for fm in frames:
        if fm.silent:
            p.add("silent_frame")
            continue
        p.add("ms" if fm.use_ms else "lr")
        lens = {pl.size for pl in fm.planes}
        if len(lens) > 1:
            p.add("odd_stereo_slice" if len(fm.planes) == 2 else "ragged_channels")
            if fm.use_ms:
                p.add("odd_stereo_slice_ms")
        kinds = [c.winner.kind for c in fm.channels]
        if 0 in kinds and any(k != 0 for k in kinds):
            p.add("raw_next_to_rice")
        for cm in fm.channels:
            w = cm.winner
            kn = ("raw", "fixed", "lpc")[w.kind]
            p.add(f"win_{kn}")
            if cm.n:
                p.add(f"res_pos{cm.res_pos & 3}_{kn}")
            if cm.full_runs:
                p.add("full_run")
            if cm.full_runs == 1:
                p.add("one_full_run")
            if cm.n and cm.n <= RUN:
                p.add("first_run_is_last")
            if 0 < cm.n <= 4 and any(c.kind == 1 and c.order >= cm.n for c in cm.cands):
                p.add("warmup_longer_than_plane")  # a fixed order the plane never leaves the warm-up of
            if w.kind == 1 and w.order >= 1 and cm.n >= 2:
                p.add("warmup_fixup")
            for t in cm.tiles:
                p.add(("staged_" if t["staged"] else "unstaged_") + kn)
                if 0 <= STAGE_BITS - (t["lead"] + t["bits"]) < 64:
                    p.add("tile_just_under_limit")
                if 0 < (t["lead"] + t["bits"]) - STAGE_BITS < 64:
                    p.add("tile_just_over_limit")
                if not t["staged"]:
                    p.add("unstaged")
                    if t["long_code"]:
                        p.add("unstaged_long_code")
            if any(not a["staged"] and not b["staged"] for a, b in zip(cm.tiles, cm.tiles[1:])):
                p.add("two_unstaged_in_a_row")
            if any(a["staged"] != b["staged"] for a, b in zip(cm.tiles, cm.tiles[1:])):
                p.add("staged_next_to_unstaged")
            if cm.long_code:
                p.add("staged_long_code")
            if w.kind and cm.n:
                u = zigzag(w.residuals)
                q = np.minimum(u >> w.k, 255)
                staged = np.repeat([t["staged"] for t in cm.tiles], TILE)[:cm.n]
                for total in (32, 33, 34):
                    if ((q + 1 + w.k == total) & staged).any():
                        p.add(f"staged_code_of_{total}_bits")
                for qq in (63, 64, 254, 255):
                    if ((q == qq) & staged).any():
                        p.add(f"staged_q{qq}")
                if (u == 65535).any():
                    p.add("zigzag_65535")
                lc = np.flatnonzero((q + 1 + w.k > 32) & staged)
                if (lc % RUN == 0).any():
                    p.add("long_code_first_of_run")
                if (lc % RUN == RUN - 1).any():
                    p.add("long_code_last_of_run")
                if (lc % TILE == TILE - 1).any():
                    p.add("long_code_last_of_tile")
                if (lc == cm.n - 1).any():
                    p.add("long_code_last_of_frame")
            for c in cm.cands:
                if c.kind != 2:
                    continue
                if not c.valid:
                    p.add("invalid_" + c.reason)
                elif c.d_robust and c.d < 0:
                    p.add("sweep3_below")
                elif c.d_robust and c.d > 2:
                    p.add("sweep3_above")
                elif c.d_robust:
                    p.add("window_hit")
            lp = [c for c in cm.cands if c.kind == 2 and c.valid and c.d_robust]
            if any(c.d < 0 or c.d > 2 for c in lp) and any(0 <= c.d <= 2 for c in lp):
                p.add("sweep3_some_orders")
            if w.kind == 2 and w.d_robust and not 0 <= w.d <= 2:
                p.add("sweep3_winner")
            valid = [c for c in cm.cands if c.valid]
            later = valid[valid.index(w) + 1:]
            if any(c.size == w.size for c in later):
                p.add("tie_first_wins")            # an equal size later in the order must not replace the winner
            if any(c.size == w.size and c.bits < w.bits for c in later):
                p.add("tie_later_has_fewer_bits")  # fewer bits, the same bytes after (bits + 7) >> 3: still the first
            if w.kind == 0 and any(c.size == 2 * cm.n for c in later):
                p.add("tie_rice_equals_raw")
            if any(c.size == w.size + 1 and 0 < c.bits - w.bits < 8 for c in valid):
                p.add("rounding_decides")          # within a byte of each other in bits, a byte apart after rounding
            if cm.n and not np.any(cm.ints):
                p.add("zero_plane")
    return p


# ------------------------------------------------------------------------------------------------ the case list
# Every case is (name, group, pcm, sr, ch, level): one or two frames, as small as its path allows. Where exact integers
# matter the floats are made by exact() and the integers are read back through f32_to_i32, never assumed.
# Groups: "packer" (ll_pack's writers), "search" (ll_analyze), "prepare" (ll_prepare), "level0" (level 0 can only emit
# Raw-typed frames, whose Rice channels the reference cannot decode: kept apart so that no packer case is exempt).
def exact(v) -> np.ndarray:
    v = np.asarray(v, np.float64)
    return ((v + 0.5 * np.sign(v)) / 32767.0).astype(np.float32)


def _il(*planes) -> np.ndarray:
    return np.stack([np.asarray(p, np.float32) for p in planes], axis=1).reshape(-1)


def _dense(sr, bursts, seed=7, bg="noise", amp=32768):
    """+-2 LSB noise (or a slow triangle, which lets a fixed predictor of order >= 1 win) with full-scale noise bursts."""
    rng = np.random.default_rng(seed)
    v = rng.integers(-2, 3, sr)
    if bg == "triangle":
        v = v + np.abs((np.arange(sr) % 32000) - 16000) - 8000
    for pos, length in bursts:
        v[pos:pos + length] = rng.integers(-amp, amp, min(length, sr - pos))
    return v


def _limit(length):
    rng = np.random.default_rng(11)
    v = rng.integers(-2, 3, 96000)
    burst = rng.integers(-4192, 4193, 4096)
    v[4096:4096 + length] = burst[:length]
    return v


def _spikes(n, values, positions):
    v = np.zeros(n, np.int64)
    for i, p in enumerate(positions):
        v[p] = values[i % len(values)]
    return v


def _long_codes(n, values, positions, ramp_seed):
    """A zero plane with isolated samples (fixed order 0 wins it: residuals equal the samples) next to a ramp channel
    (a fixed predictor of order >= 1 wins it, so the frame is ALPC-typed and the reference can decode it; level 0 itself
    only ever emits Raw-typed frames)."""
    v = _spikes(n, values, positions)
    rng = np.random.default_rng(ramp_seed)
    ramp = 3 * np.arange(n) - 9000 + rng.integers(-1, 2, n)
    return _il(exact(v), exact(ramp))


def _resonator(seed, r, th, amp, n=6000):
    rng = np.random.default_rng(seed)
    imp = np.zeros(n)
    idx = rng.choice(n, n // 100, replace=False)
    imp[idx] = rng.choice([-1.0, 1.0], idx.size)
    y = np.zeros(n)
    a1, a2 = 2 * r * math.cos(th), -r * r
    for i in range(n):
        y[i] = imp[i] + (a1 * y[i - 1] if i >= 1 else 0.0) + (a2 * y[i - 2] if i >= 2 else 0.0)
    return np.clip(np.round(y * amp), -32768, 32767).astype(np.int64)


def _sine_click(n, amp, f, sr=48000.0):
    v = np.round(amp * np.sin(2 * np.pi * f * np.arange(n) / sr)).astype(np.int64)
    v[n // 2] = -32768 if v[n // 2] > 0 else 32767
    return v


def _tonal(n, seed, amp=9000):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    v = amp * np.sin(0.05 * t + seed) + 0.4 * amp * np.sin(0.31 * t) + rng.integers(-20, 21, n)
    return np.round(v).astype(np.int64)


def _max_res_plane(n=192000, order=8, taps=3):
    """Five sines whose order-8 predictor has large alternating coefficients, and three samples set against the signs of
    its largest taps: the residual at the sample behind them exceeds 1,000,000 once the plane is doubled (mid)."""
    sines = ((1.9883038419099819, 5.483029476028994), (1.6065002785053861, 0.9378417547836553),
             (0.9299420637617408, 2.238307364950159), (0.38400979217019354, 1.2407567226497478),
             (0.2041873697458989, 4.005263600715148))
    t = np.arange(n)
    s = np.zeros(n)
    for f, ph in sines:
        s += np.sin(f * t + ph)
    v = np.round(s / np.abs(s).max() * 32767).astype(np.int64)
    c0 = np.array(levinson(autocorr(2 * v, order), order)["coeffs"])
    p = n // 2
    v[p] = 32767
    for j in np.argsort(-np.abs(c0))[:taps]:
        v[p - 1 - j] = -32767 if c0[j] > 0 else 32767
    return v


LENGTHS = (1, 2, 3, 4, 5, 6, 12, 13, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 8193)
TIES = {
    "tie_rounding_decides": (2, [0, 3, 9, 3, -2, 2, 8, 5, 3, 8, 7, 4, 8, 5, 4, 6, 7, 2, -4, 1, 4, 8]),
    "tie_first_wins": (5, [-33, 18, -17, 3, 34, -18, 18, -27, -14, 38, -6, 1, -17, -31, -6, 10, -4, 22, -11, 9, 22, 34, -6,
                           -37, 18, 2, 30, -3, -11, -35, -3, 11, 22, 29, -23, 8, 25, -19]),
    "tie_later_has_fewer_bits": (2, [-23, 16, 11, 28, 25, 39, 38, 32, -28, -37, -1, -13, 32, 24, -6, 6, 7, 32, -39, -1, 14]),
    "tie_rice_equals_raw": (5, [3595, 6308, -12331, 21676, -18921, 13942, -24660, 6110, -14931, -12743, -9327, 16966, 17395,
                                -14924, 2320, -25488, 23430, 27772, -8227, 2401, 2240, 16434, -25819, 1753, 20609, 6695,
                                3374, -27967, 25448]),
}

_CASES = None


def cases():
    """-> list of dict(name, group, pcm, sr, ch, level); built once."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []

    def add(name, group, pcm, sr, ch, level):
        out.append(dict(name=name, group=group, pcm=np.ascontiguousarray(pcm, np.float32), sr=sr, ch=ch, level=level))

    # ---- packer: dense tiles that leave the staging buffer
    add("dense96_tile0_l5", "packer", exact(_dense(96000, [(0, 4096)])), 96000, 1, 5)
    add("dense96_middle_l5", "packer", exact(_dense(96000, [(8192, 4096)])), 96000, 1, 5)
    add("dense96_straddle_l5", "packer", exact(_dense(96000, [(4096 + 1000, 4096)])), 96000, 1, 5)
    add("dense96_middle_l2", "packer", exact(_dense(96000, [(8192, 4096)], bg="triangle")), 96000, 1, 2)
    add("dense96_ms_l5", "packer", _il(exact(_dense(96000, [(8192, 4096)])), exact(_dense(96000, [(8192, 4096)]))), 96000, 2, 5)
    add("dense96_3ch_l5", "packer", _il(exact(_dense(96000, [(8192, 4096)])), exact(_dense(96000, [], seed=8)),
                                          exact(_dense(96000, [(20480, 4096)], seed=9))), 96000, 3, 5)
    add("dense192_middle_l5", "packer", exact(_dense(192000, [(8192, 4096)])), 192000, 1, 5)
    add("dense192_last_tile_l5", "packer", exact(_dense(192000, [(46 * 4096, 3584)])), 192000, 1, 5)
    add("dense192_straddle_l5", "packer", exact(_dense(192000, [(6144, 4096)])), 192000, 1, 5)
    add("dense192_two_tiles_l5", "packer", exact(_dense(192000, [(8192, 8192)])), 192000, 1, 5)
    add("dense192_middle_l2", "packer", exact(_dense(192000, [(8192, 4096)], bg="triangle")), 192000, 1, 2)
    add("dense96_middle_l0", "level0", exact(_dense(96000, [(8192, 4096)])), 96000, 1, 0)
    add("dense192_middle_l0", "level0", exact(_dense(192000, [(8192, 4096)])), 192000, 1, 0)
    # ---- packer: a tile just under and just over the 131072-bit limit (found by scaling the burst length)
    add("limit_under", "packer", exact(_limit(3087)), 96000, 1, 5)
    add("limit_over", "packer", exact(_limit(3088)), 96000, 1, 5)
    # ---- packer: long codes inside staged tiles. k = 8: q = 23, 24, 25 (q + 1 + k = 32, 33, 34), 63, 64, 254, 255
    n = 4096 + 40
    pos = [0, 15, 16, 31, 32, 47, 2048, 4079, 4080, 4095, 4096, 4111, n - 2, n - 1]
    k8 = [23 << 7, 24 << 7, 25 << 7, 63 << 7, 64 << 7, 254 << 7, 32767, -(23 << 7), -(64 << 7) - 1, -32767]
    for rot in range(3):
        add(f"long_codes_k8_rot{rot}", "packer", _long_codes(n, k8[3 * rot:] + k8[:3 * rot], pos, rot), n, 2, 2)
    add("long_codes_neg32768", "packer", _long_codes(n, [-32768, 32767, -32768, 12345], pos, 5), n, 2, 2)
    k0 = [-16, 16, -17, -32, 32, 127, -127, 64, -64]          # k = 0: u = 31, 32, 33, 63, 64, 254, 253, 128, 127
    for rot in range(2):
        add(f"long_codes_k0_rot{rot}", "packer", _long_codes(n, k0[4 * rot:] + k0[:4 * rot], pos, 7 + rot), n, 2, 2)
    add("long_codes_k8_l0", "level0", exact(_spikes(n, k8, pos)), n, 1, 0)
    # ---- packer: every byte alignment of res_pos for raw, fixed and LPC winners; raw next to Rice, odd payload sizes
    for i, nn in enumerate((1501, 1502, 1503, 1504, 1507, 1505, 1506, 1509, 1510)):
        rng = np.random.default_rng(40 + i)
        noise = rng.integers(-32768, 32768, nn)
        ramp = 2 * np.arange(nn) - 1500 + rng.integers(-3, 4, nn)
        order = [[noise, ramp, _tonal(nn, i), noise[::-1]], [_tonal(nn, i), noise, ramp, _tonal(nn, i + 9)],
                 [ramp, _tonal(nn, i), noise, ramp[::-1]]][i % 3]
        add(f"align_{nn}", "packer", _il(*[exact(p) for p in order]), 1000, 4, 5)
    add("align_lpc3", "packer", _il(exact(_tonal(1512, 1)), exact(-_tonal(1512, 4)), exact(_tonal(1512, 9))), 1512, 3, 5)
    # ---- search: the third sweep from both sides, some orders only, and a winner that needs it
    rng = np.random.default_rng(3)
    v = np.zeros(20000, np.int64)
    idx = rng.choice(20000, 200, replace=False)
    v[idx] = rng.choice([-20000, 20000], idx.size)
    add("sweep3_below_l5", "search", _il(exact(v), exact(_tonal(20000, 1))), 20000, 2, 5)
    add("sweep3_below_l9", "search", _il(exact(v), exact(_tonal(20000, 1))), 20000, 2, 9)
    add("sweep3_above_some_l9", "search", exact(_sine_click(48000, 32000, 50.0)), 48000, 1, 9)
    add("sweep3_winner_l5", "search", exact(_resonator(3, 0.8, 2.0, 3000)), 6000, 1, 5)
    add("sweep3_winner_l9", "search", exact(_resonator(3, 0.9, 1.0, 12000)), 6000, 1, 9)
    # ---- search: ties and rounding
    for name, (level, ints) in TIES.items():
        add(name, "search", exact(ints), len(ints), 1, level)
    # ---- search: Levinson's early returns
    z = np.zeros(3000, np.int64)
    add("ac0_zero_side_l5", "search", _il(exact(_tonal(3000, 2)), exact(_tonal(3000, 2))), 3000, 2, 5)
    add("ac0_zero_channel_of_three_l9", "search", _il(exact(_tonal(3000, 3)), exact(z), exact(_tonal(3000, 4))), 3000, 3, 9)
    imp = z.copy()
    imp[1234] = 9000
    add("max_coeff_single_impulse_l5", "search", _il(exact(imp), exact(_tonal(3000, 5))), 3000, 2, 5)
    mr = exact(_max_res_plane())
    add("max_res_discard_l5", "search", _il(mr, mr), 192000, 2, 5)
    # ---- search: plane lengths around the order, the warm-up, the run and the tile
    for nn in LENGTHS:
        for level in (2, 5, 9):
            add(f"len{nn}_l{level}", "search", exact(_tonal(nn, nn % 7, 6000)), 8193, 1, level)
    # ---- search: every level on one input whose winner differs across levels
    for level in range(10):
        add(f"levels_l{level}", "level0" if level == 0 else "search", _il(exact(_sine_click(12000, 16000, 100.0)), exact(_tonal(12000, 6))), 12000, 2, level)
    # ---- prepare: the mid/side decision's integer division: pairs (1,0) x X and (1,1) x Y
    for name, x in (("ms_tie_stays_lr", 20), ("ms_floor_stays_lr", 19), ("ms_takes_ms", 18)):
        l = np.ones(x + 10, np.int64)
        r = np.concatenate([np.zeros(x, np.int64), np.ones(10, np.int64)])
        add(name, "prepare", _il(exact(l), exact(r)), 100, 2, 5)
    # ---- prepare: odd stereo slice (a trailing lone L sample), with and without mid/side
    t5 = exact(_tonal(501, 1))
    add("odd_stereo_ms", "prepare", _il(t5, t5)[:-1], 501, 2, 5)
    add("odd_stereo_lr", "prepare", _il(t5, exact(-_tonal(501, 1)))[:-1], 501, 2, 5)
    # ---- prepare: len % ch != 0
    for ch in (3, 5, 8):
        full = _il(*[exact(_tonal(300, c, 3000 + 500 * c)) for c in range(ch)])
        add(f"ragged_{ch}ch", "prepare", full[:-(ch - 1)], 300, ch, 5)
        add(f"ragged_{ch}ch_two_frames", "prepare", full[:-1], 200, ch, 5)
    # ---- prepare: the silence threshold
    thr = np.float32(1e-7)
    below = np.nextafter(thr, np.float32(0))
    add("silence_all_just_below", "prepare", np.full(600, below, np.float32), 300, 2, 5)
    one = np.zeros(600, np.float32)
    one[77] = thr
    add("silence_one_at_threshold", "prepare", one, 300, 2, 5)
    sub = np.zeros(600, np.float32)
    sub[::2] = np.float32(-0.0)
    sub[1::3] = np.float32(1e-40)
    sub[5::7] = np.float32(-1e-45)
    add("silence_negzero_subnormal", "prepare", sub, 300, 2, 5)
    # ---- prepare: conversion edges
    one_f = np.float32(1.0)
    edge = [1.0, -1.0, np.nextafter(one_f, np.float32(2)), np.nextafter(one_f, np.float32(0)), np.nextafter(-one_f, np.float32(-2)),
            np.nextafter(-one_f, np.float32(0)), -32768 / 32767.0, 32767 / 32767.0, 1.0001, -1.0001, 1.5, -3.0, np.inf, -np.inf,
            np.nan, 0.0, 1 / 32767.0, -1 / 32767.0, np.nextafter(np.float32(1 / 32767.0), np.float32(0)), 0.5, -0.5, 3e38, -3e38]
    conv = np.resize(np.array(edge, np.float32), 700)
    add("conversion_edges_mono", "prepare", conv, 700, 1, 5)
    add("conversion_edges_stereo", "prepare", np.concatenate([conv, conv[::-1]]), 700, 2, 5)
    _CASES = out
    return out


# Every path the lossless encode tests must reach, by kernel. tests/test_ll_model_cpu.py asserts that each has a case.
REQUIRED_PATHS = {
    "ll_pack": [
        "unstaged", "unstaged_fixed", "unstaged_lpc", "unstaged_long_code", "two_unstaged_in_a_row",
        "staged_next_to_unstaged", "tile_just_under_limit", "tile_just_over_limit", "staged_fixed", "staged_lpc",
        "staged_long_code", "staged_code_of_32_bits", "staged_code_of_33_bits", "staged_code_of_34_bits", "staged_q63",
        "staged_q64", "staged_q254", "staged_q255", "zigzag_65535", "long_code_first_of_run", "long_code_last_of_run",
        "long_code_last_of_tile", "long_code_last_of_frame", "raw_next_to_rice", "win_raw", "win_fixed", "win_lpc",
    ] + [f"res_pos{a}_{k}" for a in range(4) for k in ("raw", "fixed", "lpc")],
    "ll_analyze": [
        "window_hit", "sweep3_below", "sweep3_above", "sweep3_some_orders", "sweep3_winner", "tie_first_wins",
        "tie_later_has_fewer_bits", "tie_rice_equals_raw", "rounding_decides", "invalid_ac0", "invalid_max_coeff",
        "invalid_n<=order", "invalid_max_res", "warmup_fixup", "warmup_longer_than_plane", "first_run_is_last", "one_full_run",
        "full_run", "zero_plane",
    ],
    "ll_prepare": ["ms", "lr", "silent_frame", "odd_stereo_slice", "odd_stereo_slice_ms", "ragged_channels"],
}

EXPECTED_UNDECODABLE = 9   # cases exempt from the decode-equals-the-integers check (see undecodable)
