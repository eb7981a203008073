"""NumPy model of the fidelity reports (flo_batch_fidelity / flo_compare, definitions in include/flo_hip.h), in the
documented order: per 1024-frame block and channel, lane l of 64 holds positions l + 64 k and adds them in k ascending,
the lanes combine by an xor butterfly over 32 .. 1; per clip, the blocks are added in order from 0.0. Every sum is an
IEEE f64 addition in that order, so the model's bits are the library's. Non-finite samples follow the header's rule: the
sums carry NaN and inf as the additions give them and the dB values follow from the sums (a NaN block value stays NaN
through the clamp); a NaN term takes no part in a maximum (np.fmax) and is not counted as clipped."""
import numpy as np

BLOCK_DTYPE = np.dtype([("signal", "<f8"), ("error", "<f8"), ("peak_error", "<f4"), ("peak_out", "<f4"), ("clipped", "<u4"),
                        ("n", "<u4")])
LANE = np.arange(64)


def _lane_sums(t):
    """t [n_blocks, 1024, ch] f64 terms -> [n_blocks, ch]: lane sums in k order, then the butterfly"""
    nb, _, ch = t.shape
    t = t.reshape(nb, 16, 64, ch)         # position j = l + 64 k -> [k][l]
    acc = t[:, 0].copy()
    for k in range(1, 16):
        acc = acc + t[:, k]
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, LANE ^ o]
    return acc[:, 0]


def _seq(v):
    """the sequential f64 sum of v [n, ch] over n, from 0.0"""
    s = np.zeros(v.shape[1:], np.float64)
    for row in v:
        s = s + row
    return s


def snr_db(signal, error):
    signal, error = np.float64(signal), np.float64(error)
    if error == 0.0:
        return np.inf
    if signal == 0.0:
        return -np.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        return 10.0 * np.log10(signal / error)


def seg_value(signal, error):
    """a qualifying block's segmental term: 60 for an error of exactly 0, else clamp(10 log10(signal / error), -10, 60),
    NaN where that is NaN"""
    signal, error = np.float64(signal), np.float64(error)
    if error == 0.0:
        return 60.0
    with np.errstate(invalid="ignore", divide="ignore"):
        v = 10.0 * np.log10(signal / error)
    return v if np.isnan(v) else min(max(v, -10.0), 60.0)


def fidelity(source, decoded, ch):
    """source, decoded: interleaved f32 (whole frames are taken). Returns (per-channel dict, block records [n_blocks, ch])."""
    x = np.asarray(source, np.float32).reshape(-1)
    y = np.asarray(decoded, np.float32).reshape(-1)
    ns, nd = x.size // ch, y.size // ch
    cmp = min(ns, nd)
    nb, ndb = -(-cmp // 1024), -(-nd // 1024)
    X = np.zeros((ndb * 1024, ch), np.float32)
    Y = np.zeros((ndb * 1024, ch), np.float32)
    X[:cmp] = x[:cmp * ch].reshape(cmp, ch)
    Y[:nd] = y[:nd * ch].reshape(nd, ch)
    t = np.arange(ndb * 1024)[:, None]
    inm = np.broadcast_to(t < cmp, X.shape)
    tailm = np.broadcast_to((t >= cmp) & (t < nd), X.shape)
    xd, yd = X.astype(np.float64), Y.astype(np.float64)
    zero = np.float64(0.0)
    with np.errstate(invalid="ignore"):
        d = yd - xd                       # (inf - inf = NaN is the rule, not an accident)
        sig = _lane_sums(np.where(inm, xd * xd, zero).reshape(ndb, 1024, ch))
        err = _lane_sums(np.where(inm, d * d, zero).reshape(ndb, 1024, ch))
        tail = _lane_sums(np.where(tailm, yd * yd, zero).reshape(ndb, 1024, ch))
        # maxima from 0 with fmax: a NaN term takes no part; NaN > 1 is false
        pe = np.fmax.reduce(np.where(inm, np.abs(d), zero).reshape(ndb, 1024, ch), axis=1, initial=0.0)
        po = np.fmax.reduce(np.where(inm, np.abs(Y), np.float32(0)).reshape(ndb, 1024, ch), axis=1, initial=np.float32(0))
        cl = ((np.abs(Y) > np.float32(1.0)) & inm).reshape(ndb, 1024, ch).sum(axis=1)
    blocks = np.zeros((nb, ch), BLOCK_DTYPE)
    blocks["signal"], blocks["error"] = sig[:nb], err[:nb]
    blocks["peak_error"] = pe[:nb].astype(np.float32)   # (the f64 maximum, rounded once)
    blocks["peak_out"] = po[:nb].astype(np.float32)
    blocks["clipped"] = cl[:nb]
    blocks["n"] = np.minimum(cmp - 1024 * np.arange(nb), 1024)[:, None]
    r = dict(signal=_seq(sig[:nb]), error=_seq(err[:nb]), tail_energy=_seq(tail),
             peak_error=np.fmax.reduce(blocks["peak_error"], axis=0, initial=np.float32(0)),
             peak_out=np.fmax.reduce(blocks["peak_out"], axis=0, initial=np.float32(0)),
             clipped=blocks["clipped"].astype(np.uint64).sum(axis=0) if nb else np.zeros(ch, np.uint64),
             compared_frames=cmp, source_frames=ns, decoded_frames=nd, n_blocks=nb)
    r["snr_db"] = np.array([snr_db(r["signal"][c], r["error"][c]) for c in range(ch)])
    seg, seg_n = np.zeros(ch), np.zeros(ch, np.int64)
    for b in range(nb):
        for c in range(ch):
            s, e, n = blocks[b, c]["signal"], blocks[b, c]["error"], blocks[b, c]["n"]
            if s / np.float64(n) >= 1e-10:          # (false for a NaN signal: such a block does not qualify)
                seg[c] = seg[c] + seg_value(s, e)
                seg_n[c] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        r["seg_snr_db"] = np.where(seg_n > 0, seg / np.maximum(seg_n, 1), np.nan)
    r["seg_blocks"] = seg_n
    return r, blocks


BIT_FIELDS = ("signal", "error", "tail_energy", "peak_error", "peak_out", "clipped", "seg_blocks")


def _one_nan(a):
    """a copy with every NaN of its float values (fields) replaced by one NaN: which of the NaN encodings an operation
    returns (x86 and gfx950 differ in the sign of inf - inf) is not part of the contract, that the value is NaN is"""
    a = np.array(a)
    for v in ([a[f] for f in a.dtype.names] if a.dtype.names else [a]):
        if v.dtype.kind == "f":
            v[np.isnan(v)] = np.nan
    return a


def assert_matches(got: dict, want: dict, want_blocks=None, tag=""):
    """a library report (flo_amd.fidelity_dict) against the model: every sum, peak and count bit for bit (NaN for NaN), the dB
    values within 1e-9 dB"""
    for k in BIT_FIELDS:
        g, w = np.asarray(got[k]), np.asarray(want[k]).astype(np.asarray(got[k]).dtype)
        assert _one_nan(g).tobytes() == _one_nan(w).tobytes(), (tag, k, g, w)
    for k in ("compared_frames", "source_frames", "decoded_frames", "n_blocks"):
        assert got[k] == want[k], (tag, k, got[k], want[k])
    for k in ("snr_db", "seg_snr_db"):
        g, w = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        with np.errstate(invalid="ignore"):
            same = (g == w) | (np.isnan(g) & np.isnan(w)) | (np.abs(g - w) <= 1e-9)
        assert same.all(), (tag, k, g, w)
    if want_blocks is not None:
        gb = got["blocks"]
        assert gb.shape == want_blocks.shape, (tag, gb.shape, want_blocks.shape)
        assert gb.dtype == want_blocks.dtype, (tag, gb.dtype)
        assert _one_nan(gb).tobytes() == _one_nan(want_blocks).tobytes(), (tag, "blocks")
