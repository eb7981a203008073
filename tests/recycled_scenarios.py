"""The scenarios of tests/test_gpu_recycled_memory.py: what every entry point that takes blocks from the device pool
(flo_amd/csrc/devpool.cpp) or recycled pinned buffers (stager_pinned_get) hands back, as records that must not depend on
what those blocks held before.

A scenario is a function (ctx) -> [(label, bytes)] of everything its calls return, restricted to the fields the API
defines (no struct padding, no slack of an np.empty array). SCENARIOS lists them in the order the test runs them, each
with `covers`: the C entry points it drives. LEFTOVERS are the A, B, A sequences: (ctx) -> (A on a fresh object, A, A
after a larger and harsher B on the same object). tests/test_recycled_memory_cpu.py holds `covers` against
flo_amd._native.EXPORTS; EXEMPT names the entry points that touch neither device nor pinned memory, with the reason.

Inputs are built once and kept; where the suite has a CPU-side anchor (the oracle's lossless files and integers, the
analysis model) the record is checked against it inside the scenario, on every run."""
import ctypes as C
import functools
import os

import numpy as np

import analysis_model as AM
import flo_amd
import signals
from conftest import EXAMPLES
from oracle import oracle as O
from test_gpu_analysis_paths import FIELDS as ANALYSIS_FIELDS   # the fields of an analysis the API defines
from test_gpu_fidelity import _raw as fidelity_raw              # the defined fields of fidelity reports

SR = 44100
LENGTHS = [0, 1, 1023, 1024, 5000, 3072]          # sample-frames of the batch scenarios' clips
GRID_X = [i / 16 for i in range(17)] + [0.99, 0.9899]   # test_gpu_ladder.GRID_X
LADDER5 = [0.0, 0.5, 0.9899, 0.99, 1.0]            # test_gpu_ladder.LADDER5
FILLS = (None, 0x00, 0x7F, 0xFF, None)             # the order of the passes: the benign ones first

SUSPECT = "stereo, 33 tiles and one sample (the last tile of channel 1 is empty)"

SCENARIOS = []
LEFTOVERS = []

# entry points no scenario needs: they touch no device memory and no pinned memory
EXEMPT = {
    "flo_free": "frees a host buffer the library returned",
    "flo_last_error": "returns the context's message string",
    "flo_last_create_error": "returns a host string",
    "flo_ctx_device_info": "copies device properties read at creation",
    "flo_ctx_profile_enable": "sets a host flag",
    "flo_ctx_profile_query": "reads host-side sums of event times",
    "flo_ctx_profile_reset": "destroys events and clears host sums",
    "flo_ctx_stream": "returns the stream handle",
    "flo_debug_stream_delay": "sets a host atomic (tests/test_gpu_late_streams.py)",
    "flo_debug_stream_delays": "reads a host counter",
    "flo_debug_delay_enqueue": "queues a kernel that touches no memory",
    "flo_ctx_reserve_cus": "sets a host field of the encode plan",
    "flo_ctx_reserved_cus": "reads that host field",
    "flo_ctx_upload_path": "reports what the upload probe measured (the probe's own scratch is hipMalloc'ed and written by its copies)",
    "flo_probe_container": "parses a file on the host",
    "flo_get_toc": "parses a file on the host",
    "flo_seek_to_time": "parses a file on the host",
    "flo_rate_pick": "host arithmetic on the caller's arrays",
    "flo_resample_filter": "builds the filter table on the host",
    "flo_resample_out_frames": "host arithmetic",
    "flo_spectral_similarity": "the host score of two fingerprints",
    "flo_batch_clip_device_ptr": "returns an address",
    "flo_dist_unique_id": "needs several ranks (RCCL); tests/test_gpu_dist.py",
    "flo_dist_create": "needs several ranks (RCCL); tests/test_gpu_dist.py",
    "flo_dist_destroy": "needs several ranks (RCCL); tests/test_gpu_dist.py",
    "flo_dist_gather_submit": "needs several ranks (RCCL); tests/test_gpu_dist.py",
    "flo_dist_gather_flush": "needs several ranks (RCCL); tests/test_gpu_dist.py",
    "flo_dist_gather_result": "needs several ranks (RCCL); tests/test_gpu_dist.py",
    "flo_dist_stream": "needs several ranks (RCCL); tests/test_gpu_dist.py",
    "flo_dist_table_submit": "needs several ranks (RCCL); tests/test_gpu_dist.py",
    "flo_dist_table_flush": "needs several ranks (RCCL); tests/test_gpu_dist.py",
    "flo_dist_table_result": "needs several ranks (RCCL); tests/test_gpu_dist.py",
}
# what every scenario drives through the test itself: the switch, and the calls behind every Context method
ALWAYS = ["flo_debug_pool_fill"]


def scenario(name, covers):
    def deco(fn):
        SCENARIOS.append(dict(name=name, covers=list(covers), run=fn))
        return fn
    return deco


def leftover(name, covers):
    def deco(fn):
        LEFTOVERS.append(dict(name=name, covers=list(covers), run=fn))
        return fn
    return deco


def first_difference(a, b):
    """None when two records are identical, else a description of the first entry that differs"""
    if [k for k, _ in a] != [k for k, _ in b]:
        return "the records' labels differ: %r against %r" % ([k for k, _ in a][:8], [k for k, _ in b][:8])
    for (k, x), (_, y) in zip(a, b):
        if x != y:
            if len(x) != len(y):
                return "%s: %d bytes against %d" % (k, len(x), len(y))
            at = next(i for i in range(len(x)) if x[i] != y[i])
            return "%s: first difference at byte %d of %d: %s against %s" % (k, at, len(x), x[at:at + 16].hex(), y[at:at + 16].hex())
    return None


# ---- inputs ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def music(frames, ch, seed):
    x = signals.music_like(SR, frames, ch, seed=seed)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def synth(frames, ch, clip_id):
    x = np.ascontiguousarray(O.synth_clip(frames, ch, clip_id=clip_id), np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def noise(frames, ch, seed, amp=1.0):
    """full-scale noise"""
    x = (np.random.default_rng(seed).uniform(-amp, amp, frames * ch)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def overflowing(frames, ch, seed):
    """full-scale noise with one sample of 3e38 in the third frame: that frame's band energies overflow f32, so the masking
    levels and the inf marks behind it stay set (tests/lossy_model.py level_clip)"""
    x = noise(frames, ch, seed).copy()
    if frames > 3000:
        x[3000 * ch] = np.float32(3e38)
    x.setflags(write=False)
    return x


def batch_clips(ch=2, seed=40):
    return [music(n, ch, seed + i) for i, n in enumerate(LENGTHS)]


def harsh_clips(ch=2, seed=70):
    """the same lengths, full-scale noise, the longest clip overflowing"""
    return [overflowing(n, ch, seed + i) if n == max(LENGTHS) else noise(n, ch, seed + i) for i, n in enumerate(LENGTHS)]


@functools.lru_cache(maxsize=None)
def many_short():
    """test_gpu_ladder's many_short: 70 clips of one to three frames, more than kFewClips"""
    return tuple(music(1 + (37 * i) % 2000, 2, 200 + i) for i in range(70))


@functools.lru_cache(maxsize=None)
def oracle_file(kind, frames, ch, seed, arg):
    """input files of the decode scenarios: the oracle's, so that they do not depend on the code under test"""
    x = {"music": music, "noise": noise, "synth": synth}[kind](frames, ch, seed)
    return O.encode_lossy(x, SR, ch, arg) if isinstance(arg, float) else O.encode_lossless(x, SR, ch, 16, arg)


def example(name):
    with open(os.path.join(EXAMPLES, name), "rb") as f:
        return f.read()


def _b(a):
    return np.ascontiguousarray(a).tobytes()


def analysis_raw(a):
    """the fields test_gpu_analysis_paths.FIELDS names, and the peaks"""
    out = _b(a["peaks"])
    for k in ANALYSIS_FIELDS:
        v = a[k]
        out += _b(np.float64(v)) if isinstance(v, float) else _b(v) if isinstance(v, np.generic) else repr(v).encode()
    return out


class forced:
    """ctx.force_path(which) for a block"""

    def __init__(self, ctx, which):
        self.ctx, self.which = ctx, which

    def __enter__(self):
        self.ctx.force_path(self.which)

    def __exit__(self, *exc):
        self.ctx.force_path(0)


# Set by the threaded harness (tests/concurrent_harness.py) for as long as several threads are inside the library, and by
# nobody else: while it is set, env(...) leaves the environment alone. The library calls getenv per call, and a setenv
# beside another thread's getenv is a data race in libc: the test would crash for a reason of its own. The block still runs
# and still produces its records under its usual labels. That is sound because both variables the scenarios set select paths
# which the per-feature tests hold byte-equal to the default path - FLO_FIDELITY_UNFUSED:
# test_gpu_fidelity.py::test_lossy_batch_matches_the_model_fused_and_unfused; FLO_FPINDEX_CHUNK_REFS:
# test_gpu_similarity.py::test_results_do_not_depend_on_the_chunking - so the record is the same either way and a
# comparison with the single-thread record (made with the variables set) stands. Single-thread users never set it.
ENV_FROZEN = False


class env:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.frozen = ENV_FROZEN
        if self.frozen:
            return
        self.old = os.environ.get(self.name)
        os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.frozen:
            return
        if self.old is None:
            del os.environ[self.name]
        else:
            os.environ[self.name] = self.old


# ---- 1. one-shot encodes ---------------------------------------------------------------------------------------------
@scenario("one-shot lossy encodes", ["flo_ctx_create", "flo_encode_lossy", "flo_ctx_force_path"])
def lossy_encodes(ctx):
    st = music(5000, 2, 1)
    rec = [("stereo 5000 q 0.55", ctx.encode_lossy(st, SR, 2, 0.55)), ("stereo 5000 q 1.0", ctx.encode_lossy(st, SR, 2, 1.0)),
           ("mono 1 sample", ctx.encode_lossy(music(1, 1, 2), SR, 1, 0.55)), ("3 channels 3000", ctx.encode_lossy(music(3000, 3, 3), SR, 3, 0.55))]
    for which in (1, 2, 5):
        with forced(ctx, which):
            rec.append(("stereo 5000 form %d" % which, ctx.encode_lossy(st, SR, 2, 0.55)))
    return rec


@functools.lru_cache(maxsize=None)
def _oracle_lossless(frames, ch, clip_id, level):
    return O.encode_lossless(synth(frames, ch, clip_id), SR, ch, 16, level)


@scenario("one-shot lossless encodes", ["flo_encode_lossless"])
def lossless_encodes(ctx):
    rec = []
    for level in (0, 5, 9):
        for frames, ch in ((50000, 2), (3, 1)):
            f = ctx.encode_lossless(synth(frames, ch, 7), SR, ch, 16, level)
            assert f == _oracle_lossless(frames, ch, 7, level), ("the oracle's file", frames, ch, level)
            rec.append(("%d ch %d frames level %d" % (ch, frames, level), f))
    return rec


# ---- 2. one-shot decodes ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_i32(f):
    return O.decode_lossless_i32(f)[0]


_SCENARIO_1 = {}


def _scenario_1_lossy(ctx):
    """the device's own lossy files of scenario 1 (which shows them identical under every fill), made once; the lossless
    files of scenario 1 are the oracle's byte for byte"""
    if not _SCENARIO_1:
        _SCENARIO_1.update({k: f for k, f in lossy_encodes(ctx)[:3]})
    return [("scenario 1 " + k, f, src) for (k, f), src in zip(_SCENARIO_1.items(), (music(5000, 2, 1), music(5000, 2, 1), music(1, 1, 2)))]


def _decode_files(files, with_scenario_1=False):
    def run(ctx):
        rec = []
        for name, f, src in files() + (_scenario_1_lossy(ctx) if with_scenario_1 else []):
            info = flo_amd.probe_container(f)
            rec.append((name + " decode", _b(ctx.decode(f))))
            if not info.is_transform:
                i32 = ctx.decode_lossless_i32(f)
                assert np.array_equal(i32, _oracle_i32(f)), ("the oracle's integers", name)
                rec.append((name + " integers", _b(i32)))
            for k in sorted({0, min(1, info.n_frames - 1), info.n_frames - 1}):
                rec.append((name + " frame %d" % k, _b(ctx.decode_frame_at(f, k))))
            if src is not None:
                rec.append((name + " compare", fidelity_raw([ctx.compare(src, f, blocks=True)])))
        return rec
    return run


def _small_files():
    return [("lossy stereo 5000", oracle_file("music", 5000, 2, 1, 0.55), music(5000, 2, 1)),
            ("lossy 3 channels 3000", oracle_file("music", 3000, 3, 3, 0.55), music(3000, 3, 3)),
            ("lossless stereo 50000", oracle_file("synth", 50000, 2, 7, 5), synth(50000, 2, 7)),
            ("lossless mono 3", oracle_file("synth", 3, 1, 7, 9), synth(3, 1, 7)),
            ("example lossless", example("audio_lossless.flo"), None), ("example lossy", example("audio_lossy.flo"), None)]


def _harsh_files():
    return [("lossy noise 40 frames", oracle_file("noise", 40000, 2, 5, 1.0), noise(40000, 2, 5)),
            ("lossless noise 3 frames", oracle_file("noise", 100000, 2, 6, 0), noise(100000, 2, 6))]


DECODE_COVERS = ["flo_decode", "flo_decode_lossless_i32", "flo_decode_frame_at", "flo_compare"]
decodes = scenario("one-shot decodes", DECODE_COVERS)(_decode_files(_small_files, with_scenario_1=True))


# ---- 3. analysis -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def analysis_cases():
    """the smallest case of each family, and the case with an empty last tile"""
    small = {}
    for c in AM.cases():
        if c["family"] not in small or c["n"] < small[c["family"]]["n"]:
            small[c["family"]] = c
    names = [c["name"] for c in small.values()]
    return tuple(names + ([SUSPECT] if SUSPECT not in names else []))


@functools.lru_cache(maxsize=None)
def _case_input(name):
    x = AM.case(name)["make"]()
    x.setflags(write=False)
    return x


def _analysis_of(names):
    def run(ctx):
        rec = []
        for name in names():
            c, x = AM.case(name), _case_input(name)
            a, meta = ctx.analyze(x, c["sr"], c["ch"], c["pps"]), ctx.analysis_metadata(x, c["sr"], c["ch"], c["pps"])
            AM.check_analysis(a, meta, c)
            rec += [(name + " analysis", analysis_raw(a)), (name + " META", meta)]
        return rec
    return run


ANALYSIS_COVERS = ["flo_analyze", "flo_analysis_metadata"]
analysis = scenario("analysis", ANALYSIS_COVERS)(_analysis_of(analysis_cases))


# ---- 4. stage calls and resample -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stage_inputs():
    st = music(5000, 2, 11)
    o = O.lossy_analyze(st, SR, 2, 0.55)
    coeffs = np.ascontiguousarray(o["coeffs"], np.float32)
    rng = np.random.default_rng(3)
    smr = rng.uniform(-20, 40, coeffs.size).astype(np.float32).reshape(-1, 1024)
    return st, coeffs, smr, np.ascontiguousarray(o["q"], np.int16)


@scenario("stage calls and resample", ["flo_mdct_forward", "flo_lossy_analyze", "flo_lossy_quantize", "flo_lossy_quantize_smr",
                                       "flo_sparse_pack", "flo_lossy_pack_frames", "flo_resample"])
def stages(ctx):
    st, coeffs, smr, q = _stage_inputs()
    rec = [("mdct_forward", _b(ctx.mdct_forward(music(3 * 2048, 1, 12))))]
    a = ctx.lossy_analyze(st, SR, 2, 0.55)
    rec += [("lossy_analyze " + k, _b(a[k])) for k in ("coeffs", "q", "sf_words")]
    for exact in (False, True):
        g = ctx.lossy_quantize(coeffs, SR, 0.55, exact=exact)
        rec += [("lossy_quantize exact %d %s" % (exact, k), _b(g[k])) for k in ("q", "sf_words")]
    gq, gsf = ctx.lossy_quantize_smr(coeffs, smr, SR, 0.55)
    rec += [("quantize_smr q", _b(gq)), ("quantize_smr sf", _b(gsf)), ("quantize_smr sf only", _b(ctx.lossy_quantize_smr(coeffs, None, SR, 0.55)[1]))]
    for form in (0, 1, 2):
        rec.append(("sparse_pack form %d" % form, b"|".join(ctx.sparse_pack(q, form))))
    for which in (5, 1, 2):
        with forced(ctx, which):
            p = ctx.lossy_pack_frames(coeffs, SR, 0.55)
        rec += [("pack_frames form %d %s" % (which, k), _b(p[k]) if k != "data" else p[k]) for k in ("q", "sf_words", "data", "frame_sizes")]
    rec.append(("resample 44100 to 48000", _b(ctx.resample(music(3000, 2, 13), 44100, 48000, 2))))
    rec.append(("resample 48000 to 44100", _b(ctx.resample(music(3000, 2, 13), 48000, 44100, 2))))
    return rec


# ---- 5. / 6. batches -------------------------------------------------------------------------------------------------
def _torch_full(n, value, dtype):
    import torch
    t = torch.full((max(int(n), 1),), value, dtype=dtype, device="cuda:0")
    torch.cuda.synchronize()
    return t


def _device_ranges(base, offs, sizes):
    """the bytes of (offset, size) ranges of device memory the library owns"""
    out = []
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    for o, s in zip(offs, sizes):
        buf = np.zeros(max(int(s), 1), np.uint8)
        if s:
            assert hip.hipMemcpy(buf.ctypes.data, base + int(o), int(s), 2) == 0
        out.append(buf[:int(s)].tobytes())
    return b"|".join(out)


def _results(b, tag, lossy):
    """everything an encoded and synchronised batch hands back"""
    import torch
    rec = [(tag + " fetch %d" % i, b.fetch(i)) for i in range(b.n_clips)]
    rec.append((tag + " fetch with META", b.fetch(b.n_clips - 1, b"\x81\xa5title\xa3abc")))
    total = b.data_bytes()
    rec.append((tag + " data_bytes", repr(total).encode()))
    files = sum(len(f) for _, f in rec[:b.n_clips])
    for name, fn, cap in (("pack_files", b.pack_files, files + 16 * b.n_clips + 64), ("pack_streams", b.pack_streams, total + 16 * b.n_clips + 64)):
        dst = _torch_full(cap, 7, torch.uint8)
        offs = fn(dst.data_ptr(), dst.numel())
        b.sync()
        torch.cuda.synchronize()
        rec.append((tag + " " + name, repr(offs).encode() + dst.cpu().numpy()[:offs[-1]].tobytes()))
    base, offs, sizes = b.device_streams()
    rec.append((tag + " device_streams", repr((offs, sizes)).encode() + _device_ranges(base, offs, sizes)))
    fb, fo, fs = C.c_void_p(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()   # (no Python wrapper)
    b.ctx._chk(b._L.flo_batch_device_files(b._h, C.byref(fb), C.byref(fo), C.byref(fs)))
    offs, sizes = [fo[i] for i in range(b.n_clips)], [fs[i] for i in range(b.n_clips)]
    rec.append((tag + " device_files", repr((offs, sizes)).encode() + _device_ranges(fb.value, offs, sizes)))
    rep = b.fidelity(blocks=True)
    rec.append((tag + " fidelity", fidelity_raw(rep)))
    if lossy:
        with env("FLO_FIDELITY_UNFUSED", "1"):
            rec.append((tag + " fidelity unfused", fidelity_raw(b.fidelity(blocks=True))))
    n_dec = sum(int(r["decoded_frames"]) for r in rep) * b.channels
    dst = _torch_full(n_dec + 8, 7.0, torch.float32)
    offs = b.decode_to(dst.data_ptr(), dst.numel())
    b.sync()
    torch.cuda.synchronize()
    rec.append((tag + " decode_to", repr(offs).encode() + dst.cpu().numpy().tobytes()))
    return rec


def _upload(b, clips):
    for i, x in enumerate(clips):
        b.upload(i, x)


def _lossy_batch_record(b, forms=(0, 1, 2, 5), extras=True):
    rec = []
    for which in forms:
        b.encode(which)
        b.sync()
        rec += _results(b, "form %d" % which, True)
    if not extras:
        return rec
    an, metas = b.analyze_all(50), b.analysis_metadata_all(50)
    rec += [("analyze_all %d" % i, analysis_raw(a)) for i, a in enumerate(an)]
    rec += [("analysis_metadata_all %d" % i, m) for i, m in enumerate(metas)]
    rec.append(("analysis_metadata of the last clip", b.analysis_metadata(b.n_clips - 1)))
    rec.append(("size_curve", _b(b.size_curve(GRID_X))))
    with b.encode_ladder(LADDER5) as lad:
        rec.append(("ladder file_bytes", _b(lad.file_bytes)))
        for j in range(lad.n_rungs):
            rec += [("ladder fetch %d rung %d" % (i, j), lad.fetch(i, j)) for i in range(lad.n_clips)]
            base, offs, sizes = lad.device_files(j)
            rec.append(("ladder device_files rung %d" % j, repr((offs, sizes)).encode() + _device_ranges(base, offs, sizes)))
    r = b.resample(48000)
    try:
        rec += [("resample 48000 clip %d" % i, _b(r.download_pcm(i))) for i in range(r.n_clips)]
    finally:
        r.close()
    b.set_quality(0.3)
    b.encode(0)
    b.sync()
    rec += [("quality 0.3 fetch %d" % i, b.fetch(i)) for i in range(b.n_clips)]
    b.set_quality(0.55)
    return rec


LOSSY_BATCH_COVERS = ["flo_batch_create", "flo_batch_destroy", "flo_batch_upload", "flo_batch_encode", "flo_batch_sync", "flo_batch_data_bytes",
                      "flo_batch_fetch", "flo_batch_pack_files", "flo_batch_pack_streams", "flo_batch_device_streams", "flo_batch_device_files", "flo_batch_decode",
                      "flo_batch_fidelity", "flo_batch_analyze_all", "flo_batch_analysis_metadata_all", "flo_batch_analysis_metadata",
                      "flo_batch_size_curve", "flo_batch_encode_ladder", "flo_ladder_shape", "flo_ladder_file_bytes", "flo_ladder_fetch",
                      "flo_ladder_device_files", "flo_ladder_destroy", "flo_batch_resample", "flo_batch_clip_device_data", "flo_batch_set_quality"]


def _lossy_batch_of(clips, forms=(0, 1, 2, 5)):
    def run(ctx):
        cs = clips()
        b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [x.size for x in cs], SR, 2, 0.55)
        try:
            _upload(b, cs)
            return _lossy_batch_record(b, forms)
        finally:
            b.close()
    return run


lossy_batch = scenario("lossy batch of six ragged clips", LOSSY_BATCH_COVERS)(_lossy_batch_of(batch_clips))
lossy_batch_many = scenario("lossy batch of 70 short clips", LOSSY_BATCH_COVERS)(_lossy_batch_of(many_short))


def _lossless_batch_record(b):
    b.set_bit_depth(16)
    b.encode(0)
    b.sync()
    rec = _results(b, "lossless", False)
    rec += [("analyze_all %d" % i, analysis_raw(a)) for i, a in enumerate(b.analyze_all(50))]
    return rec


@scenario("lossless batch of six ragged clips", ["flo_batch_set_bit_depth", "flo_batch_fill_synthetic"])
def lossless_batch(ctx):
    cs = batch_clips(seed=50)
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSLESS, [x.size for x in cs], SR, 2, 5)
    try:
        _upload(b, cs)
        rec = _lossless_batch_record(b)
    finally:
        b.close()
    s = flo_amd.Batch(ctx, flo_amd.MODE_LOSSLESS, [2 * 3000, 2 * 1], SR, 2, 5)   # PCM the device makes itself
    try:
        s.fill_synthetic(clip_id0=3)
        rec += [("synthetic pcm %d" % i, _b(s.download_pcm(i))) for i in range(2)]
        s.encode(0)
        s.sync()
        rec += [("synthetic fetch %d" % i, s.fetch(i)) for i in range(2)]
    finally:
        s.close()
    return rec


# ---- 7. corpus -------------------------------------------------------------------------------------------------------
def _corpus_files():
    return [oracle_file("synth", 50000, 2, 7, 5), oracle_file("music", 5000, 2, 1, 0.55)]


def _windows(corpus, L, starts_of):
    import torch
    fi, st = [], []
    for f, n in enumerate(int(x) for x in corpus.lengths):
        for s in starts_of(n):
            fi.append(f)
            st.append(s)
    out = torch.full((len(fi), L, corpus.channels), 7.0, device="cuda:0")
    torch.cuda.synchronize()
    corpus.decode_windows(np.array(fi, np.uint32), np.array(st, np.uint64), L, out=out)
    corpus.sync()
    torch.cuda.synchronize()
    return [("windows of %d at %r" % (L, st), out.cpu().numpy().tobytes())]


def _corpus_a(corpus):
    return _windows(corpus, 1500, lambda n: (0, n // 2, n - 5, n + 7))


def _corpus_b(corpus):
    return _windows(corpus, 9 * SR, lambda n: (0, 1, n // 3, n // 2, n - 1))


CORPUS_COVERS = ["flo_corpus_create", "flo_corpus_destroy", "flo_corpus_format", "flo_corpus_file_frames", "flo_corpus_decode_windows",
                 "flo_corpus_sync"]


@scenario("corpus windows", CORPUS_COVERS)
def corpus_windows(ctx):
    c = flo_amd.Corpus(_corpus_files(), ctx)
    try:
        return _corpus_a(c)
    finally:
        c.close()


# ---- 8. streaming decoders ---------------------------------------------------------------------------------------------
def _sdec_feed(decs, files, label):
    """each file in two halves; behind each half decode_streams with max_frames 1 once, then 0"""
    rec = []
    for half in (0, 1):
        for d, f in zip(decs, files):
            d.feed(f[:len(f) // 2] if half == 0 else f[len(f) // 2:])
        for cap in (1, 0):
            r = flo_amd.decode_streams(decs, max_frames=cap)
            rec.append(("%s half %d cap %d" % (label, half, cap),
                        _b(r.offsets) + _b(r.status) + r.out.cpu().numpy().tobytes()))
        rec.append(("%s half %d counters" % (label, half),
                    repr([(int(d.state()), d.frames_available(), d.available_frames(), d.current_frame_index(), d.buffered_bytes(), d.info())
                          for d in decs]).encode()))
    return rec


def _sdec_files_a():
    return [oracle_file("music", 3500, 2, 21, 0.55), oracle_file("synth", 50000, 2, 7, 5)]   # 5 lossy frames, 2 lossless frames


def _sdec_files_b():
    return [oracle_file("noise", 40000, 2, 5, 1.0), oracle_file("noise", 100000, 2, 6, 0)]


def _sdec_serial(d, f):
    """next_frame twice, then decode_available, on one decoder"""
    d.reset()
    d.feed(f)
    rec = [("next_frame %d" % k, _b(d.next_frame())) for k in range(2)]
    d.reset()
    d.feed(f)
    rec.append(("decode_available", _b(d.decode_available())))
    return rec


SDEC_COVERS = ["flo_sdec_create", "flo_sdec_destroy", "flo_sdec_attach", "flo_sdec_last_error", "flo_sdec_feed", "flo_sdec_state", "flo_sdec_info",
               "flo_sdec_frames_available", "flo_sdec_available_frames", "flo_sdec_current_frame_index", "flo_sdec_buffered_bytes",
               "flo_sdec_next_frame", "flo_sdec_decode_available", "flo_sdec_reset", "flo_sdec_decode_ready"]


def _sdec_a(decs):
    files = _sdec_files_a()
    for d in decs:
        d.reset()
    rec = _sdec_feed(decs, files, "streams")
    for d, f in zip(decs, files):
        rec += [(("lossy " if f is files[0] else "lossless ") + k, v) for k, v in _sdec_serial(d, f)]
    return rec


def _sdec_b(decs):
    files = _sdec_files_b()
    for d in decs:
        d.reset()
    rec = _sdec_feed(decs, files, "streams")
    for d, f in zip(decs, files):
        rec += _sdec_serial(d, f)
    return rec


@scenario("streaming decoders", SDEC_COVERS)
def streaming_decoders(ctx):
    decs = [flo_amd.StreamingDecoder(ctx), flo_amd.StreamingDecoder()]   # (the second is attached by decode_streams)
    try:
        decs[0]._err()
        return _sdec_a(decs)
    finally:
        for d in decs:
            d.close()


# ---- 9. streaming encoders ---------------------------------------------------------------------------------------------
def _stream_encoders(ctx, clips, lossless_clip, tick):
    """three lossy encoders and a lossless one through encode_streams over two ticks, then finalize; one more lossy and one
    more lossless stream through push_samples / next_frame / flush"""
    encs = [flo_amd.LossyStreamingEncoder(SR, 2, q, ctx) for q in (0.55, 0.55, 1.0)] + [flo_amd.StreamingEncoder(SR, 2, 16, ctx)]
    rec = []
    try:
        srcs = list(clips) + [lossless_clip]
        for t in range(2):
            for e, x in zip(encs, srcs):
                cut = tick * 2 if e is encs[-1] else x.size // 4 * 2   # (the lossless stream: `tick` sample-frames first)
                e.append_samples(x[:cut] if t == 0 else x[cut:])
            r = flo_amd.encode_streams(encs, ctx)
            rec.append(("tick %d status" % t, _b(r.status) + repr([(e.pending_samples(), e.pending_frames()) for e in encs]).encode()))
        rec += [("stream %d file" % i, e.finalize()) for i, e in enumerate(encs)]
    finally:
        for e in encs:
            e.close()
    for name, e, x in (("pushed lossy", flo_amd.LossyStreamingEncoder(SR, 2, 0.55, ctx), clips[0]),
                       ("pushed lossless", flo_amd.StreamingEncoder(SR, 2, 16, ctx), lossless_clip)):
        try:
            e.push_samples(x)
            k = 0
            while True:
                f = e.next_frame() or e.flush()
                if f is None or k > 64:
                    break
                rec.append(("%s frame %d" % (name, k), repr((f.index, f.timestamp_ms, f.samples)).encode() + f.data))
                k += 1
            rec.append((name + " file", e.finalize()))
        finally:
            e.close()
    return rec


STREAM_COVERS = ["flo_stream_create", "flo_stream_destroy", "flo_stream_push", "flo_stream_pending_samples", "flo_stream_pending_frames",
                 "flo_stream_next_frame", "flo_stream_flush", "flo_stream_finalize", "flo_stream_create_lossy", "flo_stream_append",
                 "flo_stream_encode_ready"]


def _streams_a(ctx):
    return _stream_encoders(ctx, [music(5000, 2, 31), music(3072, 2, 32), music(1023, 2, 33)], synth(60000, 2, 9), 30000)


def _streams_b(ctx):
    return _stream_encoders(ctx, [overflowing(40000, 2, 34), noise(30000, 2, 35), noise(20000, 2, 36)], noise(140000, 2, 37), 70000)


streaming_encoders = scenario("streaming encoders", STREAM_COVERS)(_streams_a)


# ---- 10. fingerprint index ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fingerprints(n, seed):
    from test_similarity_cpu import rand_fps
    rng = np.random.default_rng(seed)
    f, c = rand_fps(rng, n), rand_fps(rng, 20)
    pick = rng.integers(0, 20, n)
    for fld in ("energy_profile", "frequency_peaks", "avg_loudness"):   # test_gpu_similarity.clustered
        f[fld] = np.clip(c[fld][pick].astype(np.int32) + rng.integers(-4, 5, f[fld].shape), 0, 255).astype(np.uint8)
    return f


def _fp_a(ix):
    rec = []
    with env("FLO_FPINDEX_CHUNK_REFS", "256"):
        for k in (3, 16, 40):
            i, s = ix.topk_self(k)
            rec.append(("topk_self %d" % k, _b(i) + _b(s)))
        i, s = ix.topk(_fingerprints(5, 8), 16)
        rec.append(("topk of 5 queries", _b(i) + _b(s)))
        rec.append(("pairs 0.95", b"".join(_b(a) for a in ix.pairs(0.95))))
    return rec


def _fp_b(ix):
    rec = []
    with env("FLO_FPINDEX_CHUNK_REFS", "256"):
        i, s = ix.topk_self(64)
        rec.append(("topk_self 64", _b(i) + _b(s)))
        i, s = ix.topk(_fingerprints(700, 9), 64)
        rec.append(("topk of 700 queries", _b(i) + _b(s)))
        rec.append(("pairs 0.5", b"".join(_b(a) for a in ix.pairs(0.5))))
    return rec


FP_COVERS = ["flo_fpindex_create", "flo_fpindex_destroy", "flo_fpindex_topk", "flo_fpindex_topk_self", "flo_fpindex_pairs"]


@scenario("fingerprint index", FP_COVERS)
def fingerprint_index(ctx):
    ix = flo_amd.FingerprintIndex(_fingerprints(300, 7), ctx)
    try:
        return _fp_a(ix)
    finally:
        ix.close()


# ---- 11. rate-targeted encodes and the free functions ------------------------------------------------------------------
@scenario("rate-targeted encodes and free functions", ["flo_encode_batch_to_size", "flo_encode_batch", "flo_encode_batch_ladder"])
def rate_and_free_functions(ctx):
    clips = [music(5000, 2, 61), music(1, 2, 62), music(3071, 2, 63)[:-1]]
    files, chosen, fits = ctx.encode_batch_to_size(clips, SR, 2, GRID_X, [4000, 200, 3000])
    rec = [("to_size file %d" % i, f) for i, f in enumerate(files)] + [("to_size choice", repr((chosen, fits)).encode())]
    rec += [("encode_batch lossy %d" % i, f) for i, f in enumerate(ctx.encode_batch(flo_amd.MODE_LOSSY, clips, SR, 2, 0.55))]
    rec += [("encode_batch lossless %d" % i, f) for i, f in enumerate(ctx.encode_batch(flo_amd.MODE_LOSSLESS, clips, SR, 2, 5))]
    for i, fs in enumerate(flo_amd.encode_ladder_many(clips, SR, 2, LADDER5)):
        rec += [("encode_ladder_many %d rung %d" % (i, j), f) for j, f in enumerate(fs)]
    rec.append(("size_curve", _b(flo_amd.size_curve(clips[0], SR, 2, GRID_X))))
    # the C entry point on host buffers (no Python wrapper)
    k, rungs = len(clips), np.array(LADDER5, np.float32)
    ptrs = (C.c_void_p * k)(*[c.ctypes.data for c in clips])
    lens = (C.c_size_t * k)(*[c.size for c in clips])
    outs, olens = (C.c_void_p * (k * rungs.size))(), (C.c_size_t * (k * rungs.size))()
    assert ctx._L.flo_encode_batch_ladder(ctx._h, k, ptrs, lens, SR, 2, rungs.size, rungs.ctypes.data, None, None, outs, olens) == 0
    for i in range(k * rungs.size):
        rec.append(("flo_encode_batch_ladder %d" % i, C.string_at(outs[i], olens[i])))
        ctx._L.flo_free(outs[i])
    return rec


# ---- leftovers: A, B, A ----------------------------------------------------------------------------------------------
def _fresh_context(fn):
    c = flo_amd.Context(0)
    try:
        return fn(c)
    finally:
        c.close()


@leftover("one-shot decodes", DECODE_COVERS + ["flo_ctx_create", "flo_ctx_destroy"])
def decodes_aba(ctx):
    a, b = _decode_files(_small_files), _decode_files(_harsh_files)
    fresh = _fresh_context(a)
    first = a(ctx)
    b(ctx)
    return fresh, first, a(ctx)


def _harsh_analysis():
    return ("kw 4 kHz mono 524289", "infinity in the middle segment, two-pass", "NaN in the last segment, two-pass",
            "spike two passes in the trailing partial frame")


@leftover("analysis", ANALYSIS_COVERS)
def analysis_aba(ctx):
    a, b = _analysis_of(lambda: (SUSPECT, "fft 341 frames stereo and a partial frame")), _analysis_of(_harsh_analysis)
    fresh = _fresh_context(a)
    first = a(ctx)
    b(ctx)
    return fresh, first, a(ctx)


@leftover("lossy batch", LOSSY_BATCH_COVERS)
def lossy_batch_aba(ctx):
    fresh = _lossy_batch_of(batch_clips, forms=(0, 5))(ctx)
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [2 * n for n in LENGTHS], SR, 2, 0.55)
    try:
        _upload(b, batch_clips())
        first = _lossy_batch_record(b, forms=(0, 5))
        _upload(b, harsh_clips())
        _lossy_batch_record(b, forms=(0, 5))
        _upload(b, batch_clips())
        return fresh, first, _lossy_batch_record(b, forms=(0, 5))
    finally:
        b.close()


@leftover("corpus windows", CORPUS_COVERS)
def corpus_aba(ctx):
    fresh = corpus_windows(ctx)
    c = flo_amd.Corpus(_corpus_files(), ctx)
    try:
        first = _corpus_a(c)
        _corpus_b(c)
        return fresh, first, _corpus_a(c)
    finally:
        c.close()


@leftover("streaming decoders", SDEC_COVERS)
def streaming_decoders_aba(ctx):
    fresh = streaming_decoders(ctx)
    decs = [flo_amd.StreamingDecoder(ctx), flo_amd.StreamingDecoder(ctx)]
    try:
        first = _sdec_a(decs)
        _sdec_b(decs)
        return fresh, first, _sdec_a(decs)
    finally:
        for d in decs:
            d.close()


@leftover("streaming encoders", STREAM_COVERS)
def streaming_encoders_aba(ctx):
    fresh = _fresh_context(_streams_a)
    first = _streams_a(ctx)
    _streams_b(ctx)
    return fresh, first, _streams_a(ctx)


@leftover("fingerprint index", FP_COVERS)
def fingerprint_index_aba(ctx):
    fresh = fingerprint_index(ctx)
    ix = flo_amd.FingerprintIndex(_fingerprints(300, 7), ctx)
    try:
        first = _fp_a(ix)
        _fp_b(ix)
        return fresh, first, _fp_a(ix)
    finally:
        ix.close()
