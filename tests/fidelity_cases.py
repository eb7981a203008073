"""The named cases of the fidelity reports' path tests (test_gpu_fidelity_paths.py on the device, test_fidelity_cpu.py for
what can be said without one). Every case says what it is there for, by tags; PREDICATES holds one predicate per tag, over
the report the model (fidelity_ref.py) expects, and the tests assert it, so no case goes vacuous when a generator changes.
Everything is deterministic and built from seeded generators. No fixtures and no pytest hooks here.

Pair cases (flo_compare): `file()` gives the PCM a file is encoded from (forms "lossless": fid_compare_kernel, "lossy": the
fused lossy_decode_kernel<kDecCompare>) or a ready file's bytes (form "ready"); `source(decoded)` gives the source, for
most cases whatever the decode is. At most 130 blocks and 3 channels.
Batch cases (flo_batch_fidelity): `clips()` gives the clips' PCM; each runs lossy fused, lossy unfused and lossless."""
import functools

import numpy as np

import signals

SR = 44100
MAX_PAIR_BLOCKS, MAX_PAIR_CHANNELS = 130, 3
MAX_BATCH_FLOATS = 1 << 21             # interleaved floats of a whole batch case
SEG_FLOOR = 1e-10                      # a block qualifies for the segmental mean with signal / n >= this


def _f32(x):
    return np.ascontiguousarray(x, np.float32).reshape(-1)


@functools.lru_cache(maxsize=None)
def _music(frames, ch, seed):
    x = signals.music_like(SR, frames, ch, seed=seed)
    x.setflags(write=False)            # (shared between cases: whoever changes a clip copies it first)
    return x


def _noise(frames, ch, seed, amp):
    return signals.fast_noise(frames * ch, seed, amp)


# ------------------------------------------------------------------------------------------------------------ predicates
def _dec_blocks(w):
    return -(-w["decoded_frames"] // 1024)


def _chunk(b):
    return b // 64


def _in_end_zero(w, blocks):           # decoded blocks wholly past the compared range: in_end == 0, the block is all tail
    return _dec_blocks(w) - w["n_blocks"] >= 1 and w["compared_frames"] <= 1024 * (_dec_blocks(w) - 1)


def _tail_across_chunks(w, blocks):    # the blocks that hold tail lie in more than one chunk of the totals' walk
    first, last = w["compared_frames"] // 1024, _dec_blocks(w) - 1
    return _chunk(last) > _chunk(first) and bool(np.all(w["tail_energy"] > 0.0))


def _nb_other_chunk(w, blocks):        # the compared blocks end in an earlier chunk than the decoded ones
    return _chunk(max(w["n_blocks"], 1) - 1) < _chunk(_dec_blocks(w) - 1)


def _empty_source(w, blocks):
    return w["source_frames"] == 0 and w["n_blocks"] == 0 and w["decoded_frames"] > 0 and blocks.shape[0] == 0


def _cmp_is_decoded(w, blocks):
    return w["compared_frames"] == w["decoded_frames"] < w["source_frames"]


def _partial_decoded_last(w, blocks):  # in_end == dec_end < 1024 in the last block
    return w["compared_frames"] == w["decoded_frames"] and w["decoded_frames"] % 1024 != 0 and int(blocks["n"][-1, 0]) < 1024


def _zero_tail(w, blocks):
    return bool(np.all(w["tail_energy"] == 0.0))


def _plus_inf_no_blocks(w, blocks):
    return bool(np.all(w["snr_db"] == np.inf) and np.all(np.isnan(w["seg_snr_db"])) and np.all(w["seg_blocks"] == 0)) and w["n_blocks"] > 0


def _minus_inf(w, blocks):
    return bool(np.all(w["snr_db"] == -np.inf) and np.all(w["seg_blocks"] == 0) and np.all(w["error"] > 0.0))


def _exact_60(w, blocks):
    return bool(np.all(w["error"] == 0.0) and np.all(w["seg_snr_db"] == 60.0) and np.all(w["seg_blocks"] > 0) and
                np.all(w["snr_db"] == np.inf))


def _minus_6db(w, blocks):             # error = 4 x signal exactly, block by block
    ok = blocks["error"] == 4.0 * blocks["signal"]
    return bool(ok.all() and np.all(w["seg_blocks"] > 0) and np.all(np.abs(w["seg_snr_db"] - 10.0 * np.log10(0.25)) < 1e-9))


def _all_at_minus_10(w, blocks):
    return bool(np.all(w["seg_snr_db"] == -10.0) and np.all(w["seg_blocks"] == w["n_blocks"]) and w["n_blocks"] > 1)


def _excluded_between_included(w, blocks):
    q = blocks["signal"] / blocks["n"] >= SEG_FLOOR                       # [n_blocks, ch]
    inner = q[:-1]                                                        # (the partial last block has a tag of its own)
    alternating = bool(np.all(inner[1:] != inner[:-1])) and inner.shape[0] >= 4
    return alternating and bool(np.all(w["seg_blocks"] == q.sum(axis=0))) and bool(np.all(q.sum(axis=0) < w["n_blocks"]))


def _partial_last_by_n(w, blocks):     # qualifies with the division by its own n, would not with 1024
    s, n = blocks["signal"][-1], blocks["n"][-1]
    return bool(np.all(n < 1024) and np.all(s / 1024.0 < SEG_FLOOR) and np.all(s / n >= SEG_FLOOR))


def _clipped_and_loud(w, blocks):
    return bool(np.all(w["clipped"] > 0) and np.all(w["peak_out"] > 1.0))


def _nan_error(w, blocks):             # every block's error is NaN although its signal qualifies it
    return bool(np.all(np.isnan(blocks["error"])) and np.all(w["seg_blocks"] == w["n_blocks"]) and w["n_blocks"] == 4 and
                np.all(np.isnan(w["seg_snr_db"])) and np.all(np.isnan(w["snr_db"])))


def _nonfinite_sums(w, blocks):        # NaN and inf block sums next to finite ones, in every channel
    s = blocks["signal"]
    return bool(np.isnan(s).any() and np.isinf(s).any() and np.all(np.isfinite(s).any(axis=0)) and
                np.all(~np.isfinite(w["signal"])) and np.isinf(blocks["peak_error"]).any())


PREDICATES = {
    "in_end_zero_blocks": _in_end_zero, "tail_across_chunks": _tail_across_chunks, "nb_in_an_earlier_chunk": _nb_other_chunk,
    "empty_source": _empty_source, "compared_is_decoded": _cmp_is_decoded, "partial_decoded_last_block": _partial_decoded_last,
    "zero_tail": _zero_tail, "plus_inf_and_no_block": _plus_inf_no_blocks, "minus_inf": _minus_inf, "exact_60": _exact_60,
    "minus_6_db": _minus_6db, "all_at_minus_10": _all_at_minus_10, "excluded_between_included": _excluded_between_included,
    "partial_last_block_by_its_n": _partial_last_by_n, "clipped_and_loud": _clipped_and_loud, "nan_error": _nan_error,
    "nonfinite_sums": _nonfinite_sums,
}
CHUNK_EDGES = (63, 64, 65, 127, 128, 129)
for _n in CHUNK_EDGES:
    PREDICATES[f"decoded_blocks_{_n}"] = (lambda n: lambda w, blocks: _dec_blocks(w) == n)(_n)


# ------------------------------------------------------------------------------------------------------------ pair cases
class Pair:
    def __init__(self, name, there_for, ch, file, source, forms=("lossless", "lossy"), file_key=None, bits=16, derived=False):
        self.name, self.there_for, self.ch, self.file, self.source, self.forms = name, tuple(there_for), ch, file, source, forms
        self.file_key = file_key or name      # cases with one key share one file (and its decode)
        self.bits = bits                      # the lossless file's bit depth
        self.derived = derived                # the source is made from the device's decode


SHORT_SOURCES = (0, 1, 1023, 1024, 1025, 64 * 1024, 64 * 1024 + 1)
LONG_FILES = (1, 1023, 1025, 65 * 1024 + 5)
LONG_EXTRA = (1, 1024, 5000)
THRESHOLD_AMPS = (0.9e-5, 1.1e-5)       # amp^2 = 0.81e-10 and 1.21e-10: either side of SEG_FLOOR
THRESHOLD_BLOCKS, THRESHOLD_LAST, THRESHOLD_LAST_AMP = 12, 10, 5e-5   # 10 x 25e-10 / 1024 < 1e-10 <= 25e-10


def threshold_source():
    """2 channels, THRESHOLD_BLOCKS whole blocks of constant magnitude (random signs) alternating between THRESHOLD_AMPS,
    the channels in opposite phase, then a last block of THRESHOLD_LAST frames at THRESHOLD_LAST_AMP"""
    rng = np.random.default_rng(41)
    frames = THRESHOLD_BLOCKS * 1024 + THRESHOLD_LAST
    x = np.where(rng.integers(0, 2, (frames, 2)) == 1, 1.0, -1.0)
    for b in range(THRESHOLD_BLOCKS):
        for c in range(2):
            x[1024 * b:1024 * (b + 1), c] *= THRESHOLD_AMPS[(b + c) % 2]
    x[1024 * THRESHOLD_BLOCKS:] *= THRESHOLD_LAST_AMP
    return _f32(x)


def _threshold_file():
    src = threshold_source()
    pad = np.zeros((THRESHOLD_BLOCKS + 1) * 1024 * 2, np.float32)
    pad[:src.size] = src
    return _f32(pad + _noise((THRESHOLD_BLOCKS + 1) * 1024, 2, 42, 3e-6))


def nonfinite_source():
    x = _music(5000, 2, 61).copy()
    x[2 * 100 + 0] = np.nan          # block 0, channel 0
    x[2 * 2100 + 1] = np.inf         # block 2, channel 1
    x[2 * 3500 + 0] = -np.inf        # block 3, channel 0
    x[2 * 4999 + 1] = np.nan         # the partial last block, channel 1
    return x


def _ready(name):
    import tdec_ref
    return dict(tdec_ref.edge_cases())[name]


def pair_cases():
    out = []
    const = lambda v: (lambda dec: v())                      # a source that does not depend on the decode
    short_file = lambda: _music(130 * 1024 - 7, 2, 11)       # 130 decoded blocks, lossless (a partial last one) and lossy
    for k in SHORT_SOURCES:
        tags = ["in_end_zero_blocks", "tail_across_chunks", "nb_in_an_earlier_chunk"] + (["empty_source"] if k == 0 else [])
        out.append(Pair(f"short_source_{k}", tags, 2, short_file, const(lambda k=k: short_file()[:2 * k]), file_key="short_file"))
    for n in LONG_FILES:
        f = lambda n=n: _music(n, 3, 20 + n % 97)
        for k in LONG_EXTRA:
            src = const(lambda f=f, n=n, k=k: np.concatenate([f(), _noise(k, 3, n + k, 0.2)]))
            tags = ["compared_is_decoded", "zero_tail"] + (["partial_decoded_last_block"] if n % 1024 else [])
            out.append(Pair(f"long_source_{n}_plus_{k}", tags, 3, f, src, forms=("lossless",), file_key=f"long_file_{n}"))
            if k >= 1024:   # (a lossy file decodes to whole blocks: the source must pass the next multiple of 1024)
                out.append(Pair(f"long_source_lossy_{n}_plus_{k}", ["compared_is_decoded", "zero_tail"], 3, f, src,
                                forms=("lossy",), file_key=f"long_file_{n}"))
    for n in CHUNK_EDGES:
        f = lambda n=n: _music(n * 1024 - 3, 2, 30 + n)
        out.append(Pair(f"chunk_edges_{n}_full", [f"decoded_blocks_{n}"], 2, f, const(f), file_key=f"chunk_file_{n}"))
        out.append(Pair(f"chunk_edges_{n}_short", [f"decoded_blocks_{n}", "in_end_zero_blocks"], 2, f,
                        const(lambda f=f, n=n: f()[:2 * ((n - 40) * 1024 - 3)]), file_key=f"chunk_file_{n}"))
    zeros = lambda: np.zeros(5000 * 2, np.float32)
    tune = lambda: _music(5000, 2, 51)
    out.append(Pair("silence_both", ["plus_inf_and_no_block"], 2, zeros, const(zeros)))
    out.append(Pair("silent_source", ["minus_inf"], 2, tune, const(zeros), file_key="tune"))
    out.append(Pair("exact", ["exact_60"], 2, tune, lambda dec: _f32(dec).copy(), file_key="tune", derived=True))
    out.append(Pair("negated", ["minus_6_db"], 2, tune, lambda dec: -_f32(dec), file_key="tune", derived=True))
    out.append(Pair("unrelated_loud", ["all_at_minus_10"], 1, lambda: _noise(8000, 1, 52, 1.0),
                    const(lambda: _f32(np.float32(0.01) * _noise(8000, 1, 53, 1.0)))))
    out.append(Pair("threshold_blocks", ["excluded_between_included", "partial_last_block_by_its_n"], 2, _threshold_file,
                    const(threshold_source), bits=24))
    out.append(Pair("loud", ["clipped_and_loud"], 2, lambda: _noise(5000, 2, 54, 3.0), const(lambda: _noise(5000, 2, 54, 3.0)),
                    forms=("lossy",)))
    out.append(Pair("nan_decode", ["nan_error"], 2, lambda: _ready("tiny_words"), const(lambda: _music(4096, 2, 55)),
                    forms=("ready",)))
    out.append(Pair("nonfinite_source", ["nonfinite_sums"], 2, tune, const(nonfinite_source), file_key="tune"))
    return out


PAIRS = {p.name: p for p in pair_cases()}
PAIR_IDS = [(p.name, form) for p in PAIRS.values() for form in p.forms]


# ----------------------------------------------------------------------------------------------------------- batch cases
# Batch predicates are over the list of the clips' expected reports.
def _b_empties(ws, ch):
    z = [w["decoded_frames"] == 0 and w["source_frames"] == 0 and w["n_blocks"] == 0 for w in ws]
    return z[0] and z[-1] and any(a and b for a, b in zip(z[1:-1], z[2:-1])) and not all(z)


def _b_unaligned(ws, ch):              # (clip, channel) units that do not fill the last workgroup of four waves
    return ch % 4 != 0 and (len(ws) * ch) % 4 != 0 and any(_dec_blocks(w) > 64 for w in ws)


def _b_eight(ws, ch):
    return ch == 8 and any(_dec_blocks(w) > 64 for w in ws)


def _b_many(ws, ch):
    silent = sum(1 for w in ws if np.all(w["signal"] == 0.0))
    return len(ws) >= 150 and all(1 <= _dec_blocks(w) <= 3 for w in ws) and 0 < silent < 10


def _b_nonfinite(ws, ch):
    bad = [not np.all(np.isfinite(w["signal"])) for w in ws]
    return bad == [False, True, False]


BATCH_PREDICATES = {"empty_clips_first_middle_last": _b_empties, "units_not_a_multiple_of_4": _b_unaligned, "eight_channels": _b_eight,
                    "many_short_clips": _b_many, "nonfinite_clip_between_ordinary_ones": _b_nonfinite}


class BatchCase:
    def __init__(self, name, there_for, ch, clips):
        self.name, self.there_for, self.ch, self.clips = name, tuple(there_for), ch, clips


EMPTIES = (0, 1, 1024, 0, 0, 3000, 0)   # frames (a lossless batch takes zero-length clips like a lossy one)
CHANNEL_FRAMES = (1, 1025, 65 * 1024 + 1)
MANY = 150


def many_short_frames(i):
    return 1 + (37 * i) % 3000          # 1 .. 3 blocks


def _channel_clips(ch):
    out = []
    for k, n in enumerate(CHANNEL_FRAMES):
        x = _music(n, ch, 70 + 10 * ch + k)
        if k != 1:
            x = np.concatenate([x, np.float32([0.25] * (1 + k % (ch - 1)))])   # n_interleaved % ch != 0
        out.append(x)
    return out


def nonfinite_batch_clips():
    bad = _music(3000, 2, 91).copy()
    bad[2 * 10], bad[2 * 1500 + 1], bad[2 * 2500] = np.nan, np.inf, -np.inf
    return [_music(2500, 2, 90), bad, _music(1100, 2, 92)]


def batch_cases():
    out = [BatchCase("empties", ["empty_clips_first_middle_last"], 2, lambda: [_music(n, 2, 80 + i) for i, n in enumerate(EMPTIES)])]
    for ch in (3, 5):   # 3 clips x 3 or 5 channels: 9 and 15 units
        out.append(BatchCase(f"channels_{ch}", ["units_not_a_multiple_of_4"], ch, lambda ch=ch: _channel_clips(ch)))
    out.append(BatchCase("channels_8", ["eight_channels"], 8, lambda: _channel_clips(8)))   # (8 n is always a multiple of 4)
    out.append(BatchCase("many_short", ["many_short_clips"], 2, lambda: [
        np.zeros(2 * many_short_frames(i), np.float32) if i % 29 == 7 else _music(many_short_frames(i), 2, 300 + i) for i in range(MANY)]))
    out.append(BatchCase("nonfinite_batch", ["nonfinite_clip_between_ordinary_ones"], 2, nonfinite_batch_clips))
    return out


BATCHES = {b.name: b for b in batch_cases()}
BATCH_FORMS = ("fused", "unfused", "lossless")
