"""A `reflo`-shaped command line on top of the HIP library (python -m flo_amd.cli ...).

Mirrors the reference CLI (reflo/src/main.rs:19-93, 218-420): the same sub-commands, options, quality names and
printed fields for the parts that sit on this repository's path -
    encode  <in.wav> <out.flo> [--level N] [--lossy | --transform] [--quality low|medium|high|veryhigh|transparent]
                               [--bitrate KBPS] [--target-kbps KBPS] [--rate HZ] [--lufs N [--ceiling D] [--limit]]
                               [--mono] [--trim-silence DB]
    edit    <in.wav> <out.wav> [--mono | --channels N --matrix a,b,...] [--start S] [--duration S]
                               [--trim-silence DB] [--pre-ms MS] [--post-ms MS] [--fade-in MS] [--fade-out MS]
                               [--pad-head S] [--pad-tail S]
    mix     <in1.wav> <in2.wav> ... --out <out.wav> [--gains g,g,...] [--at-ms a,a,...]
    concat  <in1.wav> <in2.wav> ... --out <out.wav> [--crossfade-ms MS]
    filter  <in.wav> <out.wav> (--lowpass HZ | --highpass HZ | --bandpass LO,HI | --bandstop LO,HI) [--taps N] [--beta B]
    convolve <in.wav> <ir.wav> <out.wav> [--tail] [--method direct|fft|auto]
    resample <in.wav> <out.wav> --rate HZ
    normalize <in.wav> <out.wav> --lufs N [--ceiling D] [--limit]
    curve   <in.wav> [--json]
    ladder  <in.wav> <outdir> --qualities Q0,Q1,... [--json]
    decode  <in.flo> <out.wav>
    info    <in.flo>
    validate <in.flo>
    metadata <in.flo> [--json]
    analysis <in.flo> [--waveform] [--spectrum] [--json]
    similar  <in.flo>... [-k N | --threshold T] [--json]
    compare  <source.wav> <in.flo> [--json] [--blocks]
Ingestion is WAV only (flo_amd/wav.py; the reference demuxes MP3/FLAC/OGG/AAC through symphonia, reflo/src/audio.rs:57-166).
`encode` writes the META chunk the reference CLI writes for an untagged file (reflo/src/lib.rs:202-283, flo_amd/meta.py):
length_ms, encoding_time, encoder_settings, flo_encoder_version, source_format (+ --title / --artist / --album) - the
reference-made Examples/*.flo are reproduced including META, the encoding time aside. Tags inside the source file
(RIFF INFO) are not carried over. `analysis` (reflo/src/main.rs:619-800) decodes the file and prints what flo_analyze
computes on the device: EBU R128 loudness, range, true peak and sample peak (core/ebu_r128.rs), and on request the
waveform peaks at 60 per second and the spectral fingerprint (core/analysis.rs).
`similar` (not in reflo) compares the spectrum fingerprints the files' META carry under spectral_similarity
(core/analysis.rs:395-437) on the device: each file's k nearest other files, or every pair at or above a threshold.
`compare` (not in reflo; the reference's TODO lists it as "compare original vs encoded") measures on the device how far
the file's decoded audio lies from the source WAV: SNR, segmental SNR, peak error, clipped samples and the energy of the
decoded tail past the source's end, per channel (flo_compare, include/flo_hip.h).
`encode --lossy --target-kbps N` and `curve` (not in reflo) measure instead of mapping: the size of the file at every quality
of a grid comes from one device pass over the audio (flo_batch_size_curve), and the encode takes the best quality whose whole
file, META included, stays within N kbps over the clip's duration.
`ladder` (not in reflo) writes the file at every quality of a list, <outdir>/<stem>.r<j>.flo for rung j, from one upload and
one transform pass on the device (flo_batch_encode_ladder): each file is what `encode --lossy --quality Qj` writes.
`resample` and `encode --rate N` (not in reflo) convert the audio to N Hz on the device first (flo_resample: a polyphase
Kaiser-windowed sinc, include/flo_hip.h); the encode then analyses and encodes the converted audio, and header and META carry N.
`normalize` and `encode --lufs N` (not in reflo) bring the audio to N LUFS under a true-peak ceiling of D dBTP (default -1) on
the device (flo_normalize): by a gain that the ceiling may lower, or with --limit by the full gain and a look-ahead limiter.
In `encode` this comes after --rate and before the analysis, so META describes the audio that is encoded.
`edit`, `encode --mono` and `encode --trim-silence DB` (not in reflo) cut, pad, fade and remix the audio on the device
(flo_batch_edit, flo_batch_active_range): --start / --duration pick a window in seconds, --trim-silence DB narrows it to the
clip's active range (samples above DB dBFS), widened by --pre-ms / --post-ms; the cut is faded over --fade-in / --fade-out
milliseconds and padded with --pad-head / --pad-tail seconds of silence; --mono averages the channels, --channels N with
--matrix (N rows of the source's channel count, row-major) mixes them. In `encode` the edits come first, before --rate and
--lufs, in that order.
`mix` and `concat` (not in reflo) sum or join several WAV files of one sample rate and channel count on the device
(flo_mix): `mix` lays file i at --at-ms a_i milliseconds (default 0) times --gains g_i (default 1), the output ending with
the file that ends last; `concat` plays the files end to end, neighbours overlapping in a linear crossfade of
--crossfade-ms milliseconds (default 0: gapless). Files of another rate or channel count go through `resample` or `edit` first.
`filter` and `convolve` (not in reflo) run a direct-form FIR over the audio on the device (flo_convolve): `filter` designs a
linear-phase Kaiser-windowed sinc of --taps coefficients (odd, default 255) and --beta (default 9) and takes its delay off, so
the output is as long as the input; `convolve` applies the response in ir.wav (mono, or with the input's channels: channel c
by channel c), cut to the input's length or with --tail in full; --method fft takes the partitioned FFT path for long
responses (flo_convolve_fft: up to 1048576 taps, an f32 approximation of the direct chain), auto takes it from the measured
crossover on, direct (the default) never. A response at another rate goes through `resample` first, a
stereo response on a mono input through `edit --mono` or `edit --channels`.
The quality names map as in the reference CLI (main.rs:236-242): low 0.2, medium 0.4, high 0.6, veryhigh 0.8,
transparent 1.0 - NOT the QualityPreset values the library API uses (lossy/mod.rs:39-47).
"""
import argparse
import math
import sys

import json
import struct

from . import api, meta
from .wav import WavError, read_wav_bytes, write_wav_bytes

QUALITY = {"low": 0.2, "medium": 0.4, "med": 0.4, "high": 0.6, "veryhigh": 0.8, "vh": 0.8, "transparent": 1.0, "trans": 1.0}
QUALITY_NAMES = ["Low", "Medium", "High", "VeryHigh", "Transparent"]


def _wav_source_format(audio_bytes: bytes) -> str:
    """reflo/src/audio.rs:106-119 (bytes input carries no extension): the codec decides - 16 / 24 / 32-bit integer PCM
    is "WAV", everything else "UNKNOWN" (float and 8-bit PCM are not in the reference's list)."""
    pos = 12
    while pos + 8 <= len(audio_bytes):
        cid, size = audio_bytes[pos:pos + 4], struct.unpack_from("<I", audio_bytes, pos + 4)[0]
        if cid == b"fmt " and size >= 16:
            tag, bits = struct.unpack_from("<H", audio_bytes, pos + 8)[0], struct.unpack_from("<H", audio_bytes, pos + 22)[0]
            if tag == 0xFFFE and size >= 26:
                tag = struct.unpack_from("<H", audio_bytes, pos + 32)[0]
            return "WAV" if tag == 1 and bits in (16, 24, 32) else "UNKNOWN"
        pos += 8 + size + (size & 1)
    return "UNKNOWN"


def edit_options(mono=False, channels=None, matrix=None, start=None, duration=None, trim_silence=None, pre_ms=0.0, post_ms=0.0,
                 fade_in=0.0, fade_out=0.0, pad_head=0.0, pad_tail=0.0):
    """apply_edit's options for the `edit` command's switches, or None when none of them is given"""
    if isinstance(matrix, str):
        matrix = [float(v) for v in matrix.split(",") if v.strip()]
    if mono and (channels is not None or matrix is not None):
        raise ValueError("--mono excludes --channels and --matrix")
    if (channels is None) != (matrix is None):
        raise ValueError("--channels and --matrix go together")
    o = dict(mono=bool(mono), channels=channels, matrix=matrix, start=start, duration=duration, trim_silence=trim_silence,
             pre_ms=float(pre_ms), post_ms=float(post_ms), fade_in=float(fade_in), fade_out=float(fade_out),
             pad_head=float(pad_head), pad_tail=float(pad_tail))
    idle = dict(mono=False, channels=None, matrix=None, start=None, duration=None, trim_silence=None, pre_ms=0.0, post_ms=0.0,
                fade_in=0.0, fade_out=0.0, pad_head=0.0, pad_tail=0.0)
    return None if o == idle else o


def apply_edit(samples, sr, ch, opts, ctx=None):
    """(samples, channels, info) of one cut of the clip on the device (edit_options): one upload, the active range when
    --trim-silence asks for it, one Batch.edit, one fetch"""
    c = ctx or api.default_context()
    p = api._f32(samples)
    n = p.size // ch
    secs = lambda v: int(round(float(v) * sr))   # noqa: E731
    b = api.Batch(c, api.MODE_LOSSLESS, [p.size], sr, ch, 0)
    try:
        b.upload(0, p)
        lo = min(secs(opts["start"]), n) if opts["start"] is not None else 0
        hi = min(lo + secs(opts["duration"]), n) if opts["duration"] is not None else n
        info = {}
        if opts["trim_silence"] is not None:
            first, end = (int(v) for v in b.active_ranges(opts["trim_silence"])[0])
            info["active"] = (first, end)
            seg = api.trim_segments([(first, end)], [n], sr, opts["pre_ms"], opts["post_ms"])[0]
            lo, hi = max(lo, seg["start"]), min(hi, seg["start"] + seg["frames"])
            hi = max(hi, lo)
        frames = hi - lo
        fade = lambda ms: min(api._ms_frames(ms, sr), frames, (1 << 24) - 1)   # noqa: E731
        seg = dict(clip=0, start=lo, frames=frames, pad_head=secs(opts["pad_head"]), pad_tail=secs(opts["pad_tail"]),
                   fade_in=fade(opts["fade_in"]), fade_out=fade(opts["fade_out"]))
        info["segment"] = seg
        if opts["mono"]:
            r = b.edit([seg], None, [[1.0 / ch] * ch])
        else:
            r = b.edit([seg], opts["channels"], opts["matrix"])
        try:
            return r.download_pcm(0), r.channels, info
        finally:
            r.close()
    finally:
        b.close()


def edit_wav(audio_bytes: bytes, opts, ctx=None):
    """(wav, info): the WAV cut, padded, faded and remixed on the device, as the 32-bit float WAV `decode` writes"""
    samples, sr, ch = read_wav_bytes(audio_bytes)
    out, ch, info = apply_edit(samples, sr, ch, opts or edit_options(start=0.0), ctx)
    return write_wav_bytes(out, sr, ch), info


def _read_at_rate(audio_bytes: bytes, rate, ctx=None, level=None, edit=None):
    """the WAV's samples, edited on the device when `edit` (edit_options) is given, converted to `rate` Hz on the device when
    one is given and differs, then normalised when `level` (a dict of Context.normalize's keywords) is given"""
    samples, sr, ch = read_wav_bytes(audio_bytes)
    if edit is not None:
        samples, ch, _ = apply_edit(samples, sr, ch, edit, ctx)
    if rate is not None and int(rate) != sr:
        samples, sr = (ctx or api.default_context()).resample(samples, sr, int(rate), ch), int(rate)
    if level is not None:
        samples, _ = (ctx or api.default_context()).normalize(samples, sr, ch, **level)
    return samples, sr, ch


def mix_options(n_inputs, gains=None, at_ms=None):
    """(gains, at_ms) of the `mix` command for n_inputs files: comma-separated lists or sequences, one entry per file;
    None: every gain 1, every file at 0 ms"""
    def numbers(v, default, what):
        if v is None:
            return [default] * n_inputs
        vals = [float(x) for x in v.split(",")] if isinstance(v, str) else [float(x) for x in v]
        if len(vals) != n_inputs:
            raise ValueError(f"{what} has {len(vals)} entries for {n_inputs} input files")
        return vals
    g, at = numbers(gains, 1.0, "--gains"), numbers(at_ms, 0.0, "--at-ms")
    if any(a < 0 for a in at):
        raise ValueError("--at-ms must not be negative")
    return g, at


def _same_format(wavs):
    """([samples], sample_rate, channels) of WAV files that share both"""
    if not wavs:
        raise ValueError("no input files")
    clips = [read_wav_bytes(w) for w in wavs]
    sr, ch = clips[0][1], clips[0][2]
    for i, (_, r, c) in enumerate(clips):
        if (r, c) != (sr, ch):
            raise ValueError(f"input {i + 1} is {r} Hz with {c} channels, input 1 is {sr} Hz with {ch}: "
                             "bring them to one format with `resample` and `edit --channels` first")
    return [c[0] for c in clips], sr, ch


def mix_wavs(wavs, gains=None, at_ms=None, ctx=None) -> bytes:
    """the sum of the WAV files (bytes each), file i at at_ms[i] milliseconds times gains[i] (mix_options), as the 32-bit
    float WAV `decode` writes: one upload, one device pass, one fetch (Context.mix)"""
    clips, sr, ch = _same_format(wavs)
    g, at = mix_options(len(clips), gains, at_ms)
    parts = [dict(out=0, clip=i, at=int(math.floor(at[i] * sr / 1000.0 + 0.5)), gain=g[i]) for i in range(len(clips))]
    return write_wav_bytes((ctx or api.default_context()).mix(clips, sr, ch, parts), sr, ch)


def concat_wavs(wavs, crossfade_ms=0.0, ctx=None) -> bytes:
    """the WAV files (bytes each) end to end, neighbours crossfaded over crossfade_ms (api.concat_parts), as the 32-bit float
    WAV `decode` writes"""
    clips, sr, ch = _same_format(wavs)
    parts, T = api.concat_parts([c.size // ch for c in clips], sr, crossfade_ms)
    return write_wav_bytes((ctx or api.default_context()).mix(clips, sr, ch, parts, T), sr, ch)


def filter_options(lowpass=None, highpass=None, bandpass=None, bandstop=None):
    """(kind, f_lo, f_hi) of the `filter` command: exactly one of the four; the band options are "LO,HI" or a pair"""
    given = [(k, v) for k, v in (("lowpass", lowpass), ("highpass", highpass), ("bandpass", bandpass), ("bandstop", bandstop)) if v is not None]
    if len(given) != 1:
        raise ValueError("exactly one of --lowpass, --highpass, --bandpass and --bandstop is required")
    kind, v = given[0]
    if kind == "lowpass":
        return kind, None, float(v)
    if kind == "highpass":
        return kind, float(v), None
    pair = [float(x) for x in (v.split(",") if isinstance(v, str) else v)]
    if len(pair) != 2:
        raise ValueError(f"--{kind} takes two frequencies, LO,HI")
    return kind, pair[0], pair[1]


def filter_wav(wav, kind, f_lo=None, f_hi=None, taps=255, beta=9.0, ctx=None) -> bytes:
    """the WAV file (bytes) through api.fir_design's filter, delay taken off, as the 32-bit float WAV `decode` writes"""
    samples, sr, ch = read_wav_bytes(wav)
    table = api.fir_design(kind, sr, f_lo, f_hi, taps, beta)
    return write_wav_bytes((ctx or api.default_context()).convolve(samples, table, sr, ch, 1, mode="centered"), sr, ch)


def convolve_wavs(wav, ir_wav, tail=False, ctx=None, method="direct") -> bytes:
    """the WAV file (bytes) filtered by the response in ir_wav (mono or of the same channels, at the same rate), cut to the
    input's length or (tail) in full, as the 32-bit float WAV `decode` writes"""
    samples, sr, ch = read_wav_bytes(wav)
    ir, ir_sr, ir_ch = read_wav_bytes(ir_wav)
    if ir_sr != sr:
        raise ValueError(f"the response is {ir_sr} Hz, the input {sr} Hz: bring the response to {sr} Hz with `resample` first")
    if ir_ch not in (1, ch):
        raise ValueError(f"the response has {ir_ch} channels, the input {ch}: a response is mono or has the input's channels; "
                         "bring either to the other's with `edit --mono` or `edit --channels` first")
    return write_wav_bytes((ctx or api.default_context()).convolve(samples, ir, sr, ch, ir_ch, mode="full" if tail else "head", method=method), sr, ch)


def level_options(lufs, ceiling=-1.0, limit=False):
    """Context.normalize's keywords for --lufs / --ceiling / --limit, or None without --lufs"""
    return None if lufs is None else dict(target_lufs=float(lufs), ceiling_dbtp=float(ceiling), limit=bool(limit))


def normalize_wav(audio_bytes: bytes, lufs, ceiling=-1.0, limit=False, ctx=None):
    """(wav, report): the WAV at `lufs` LUFS under `ceiling` dBTP, as the 32-bit float WAV `decode` writes"""
    samples, sr, ch = read_wav_bytes(audio_bytes)
    out, report = (ctx or api.default_context()).normalize(samples, sr, ch, **level_options(lufs, ceiling, limit))
    return write_wav_bytes(out, sr, ch), report


def resample_wav(audio_bytes: bytes, rate, ctx=None) -> bytes:
    """the WAV at `rate` Hz, as the 32-bit float WAV `decode` writes"""
    samples, sr, ch = _read_at_rate(audio_bytes, rate, ctx)
    return write_wav_bytes(samples, sr, ch)


def encode_from_audio(audio_bytes: bytes, level=5, lossy=False, quality=0.6, bitrate=None, ctx=None, title=None, artist=None,
                      album=None, encoding_time=None, rate=None, normalize=None, edit=None, pcm=None) -> bytes:
    """reflo::encode_from_audio (reflo/src/lib.rs:183-306) for WAV input; edit: cut and remix first (edit_options); rate:
    then convert to that sample rate; normalize: then bring to that level (level_options). pcm: (samples, rate, channels)
    that the caller has already read, edited, converted and levelled that way: they are encoded as they are."""
    c = ctx or api.default_context()
    samples, sr, ch = pcm if pcm is not None else _read_at_rate(audio_bytes, rate, c, normalize, edit)
    level = min(int(level), 9)
    is_lossy = bool(lossy or bitrate is not None)
    quality = min(max(float(quality), 0.0), 1.0)
    mb = meta.cli_metadata(samples.size, sr, ch, _wav_source_format(audio_bytes), is_lossy, quality, bitrate, level,
                           title, artist, album, encoding_time)
    if is_lossy:
        q = api.QualityPreset.from_bitrate(bitrate, sr, ch).as_f32() if bitrate is not None else quality
        return api.TransformEncoder(sr, ch, q, c).encode_to_flo(samples, mb)
    return api.Encoder(sr, ch, 16, c).with_compression(level).encode(samples, mb)


def encode_to_target(audio_bytes: bytes, target_kbps, title=None, artist=None, album=None, encoding_time=None, rate=None, normalize=None,
                     edit=None, pcm=None):
    """(file, info): the WAV encoded at the best quality of api.DEFAULT_RATE_GRID whose whole file fits target_kbps; pcm as
    in encode_from_audio"""
    samples, sr, ch = pcm if pcm is not None else _read_at_rate(audio_bytes, rate, level=normalize, edit=edit)
    shown = int(target_kbps) if float(target_kbps).is_integer() else target_kbps
    mb = meta.cli_metadata(samples.size, sr, ch, _wav_source_format(audio_bytes), True, 0.0, shown, 5, title, artist, album,
                           encoding_time)
    return api.encode_to_bitrate(samples, sr, ch, target_kbps, metadata=mb, with_info=True, _analysis=False)


def curve_report(audio_bytes: bytes, qualities=api.DEFAULT_RATE_GRID) -> list:
    """one row per candidate quality: the size of the file (empty META) and its bitrate over the clip's duration"""
    samples, sr, ch = read_wav_bytes(audio_bytes)
    sizes = api.size_curve(samples, sr, ch, qualities)
    secs = samples.size / ch / sr
    return [{"quality": float(q), "bytes": int(b), "kbps": (int(b) * 8 / 1000 / secs) if secs else 0.0} for q, b in zip(qualities, sizes)]


def parse_rungs(text: str) -> list:
    """"low,high,transparent" -> [0.2, 0.6, 1.0]: the names `encode --quality` takes"""
    out = []
    for t in (x.strip().lower() for x in text.split(",")):
        if t not in QUALITY:
            raise ValueError(f"Invalid quality level: {t}. Use: low, medium, high, veryhigh, transparent")
        out.append(QUALITY[t])
    return out


def ladder_from_audio(audio_bytes: bytes, qualities, ctx=None, title=None, artist=None, album=None, encoding_time=None) -> list:
    """the WAV at every quality of the list, one file per rung, each with the META `encode --lossy --quality` writes"""
    samples, sr, ch = read_wav_bytes(audio_bytes)
    c = ctx or api.default_context()
    fmt = _wav_source_format(audio_bytes)
    p = api._f32(samples)
    b = api.Batch(c, api.MODE_LOSSY, [p.size], sr, ch, 0.0)
    try:
        b.upload(0, p)
        with b.encode_ladder(qualities) as lad:
            return [lad.fetch(0, j, meta.cli_metadata(samples.size, sr, ch, fmt, True, min(max(float(q), 0.0), 1.0), None, 5, title,
                                                      artist, album, encoding_time)) for j, q in enumerate(qualities)]
    finally:
        b.close()


def get_metadata(flo_bytes: bytes):
    """reflo::get_metadata: the decoded META chunk (a dict), or None when the file has none."""
    return api.file_metadata(flo_bytes)


def decode_to_wav(flo_bytes: bytes, ctx=None) -> bytes:
    """reflo::decode_to_wav: libflo::decode, then a 32-bit float WAV (reflo/src/audio.rs:290-320)."""
    c = ctx or api.default_context()
    pcm, sr, ch = c.decode(flo_bytes, with_info=True)
    return write_wav_bytes(pcm, sr, ch)


def flo_info(flo_bytes: bytes) -> dict:
    """reflo::get_flo_info (reflo/src/lib.rs:40-93): header fields, duration, compression ratio, CRC check."""
    import zlib
    i = api.probe_container(flo_bytes)
    data = flo_bytes[i.data_start:i.data_start + i.data_size]
    duration = i.total_samples / i.sample_rate if i.sample_rate else 0.0
    raw = i.total_samples * i.channels * (i.bit_depth // 8)
    return dict(version=f"{i.version_major}.{i.version_minor}", sample_rate=i.sample_rate, channels=i.channels,
                bit_depth=i.bit_depth, total_samples=i.total_samples, duration_secs=duration, file_size=len(flo_bytes),
                compression_ratio=(raw / len(flo_bytes)) if len(flo_bytes) else 0.0,
                crc_valid=(zlib.crc32(data) & 0xFFFFFFFF) == i.data_crc32, is_lossy=bool(i.flags & 1),
                lossy_quality=(i.flags >> 8) & 0x0F, compression_level=i.compression_level)


def analysis_report(flo_bytes: bytes, waveform=False, spectrum=False, ctx=None) -> dict:
    """What reflo's `analysis` command gathers (reflo/src/main.rs:619-735): file info, compute_ebu_r128_loudness on the
    decoded samples, optionally extract_waveform_peaks at 60 peaks per second and extract_spectral_fingerprint."""
    import numpy as np
    c = ctx or api.default_context()
    info = flo_info(flo_bytes)
    pcm, sr, ch = c.decode(flo_bytes, with_info=True)
    a = c.analyze(pcm, info["sample_rate"], info["channels"], 60)
    out = {"file_info": {"sample_rate": info["sample_rate"], "channels": info["channels"], "bit_depth": info["bit_depth"],
                         "duration_secs": info["duration_secs"], "total_samples": info["total_samples"]},
           "loudness": {"integrated_lufs": a["integrated_lufs"], "loudness_range_lu": a["loudness_range_lu"],
                        "true_peak_dbtp": a["true_peak_dbtp"], "sample_peak_dbfs": a["sample_peak_dbfs"]},
           "waveform": None, "spectral": None}
    if waveform:
        pk = a["peaks"]
        stats = None
        if pk.size:
            # (the reference averages with a sequential f32 sum: main.rs:662)
            acc = np.float32(0.0)
            for v in pk:
                acc = np.float32(acc + v)
            stats = {"min": float(pk.min()), "max": float(pk.max()), "average": float(acc / np.float32(pk.size))}
        out["waveform"] = {"peaks_per_second": 60, "total_peaks": int(pk.size), "channels": info["channels"], "peak_statistics": stats}
    if spectrum:
        out["spectral"] = {"duration_ms": a["duration_ms"], "sample_rate": a["sample_rate"], "channels": a["channels"],
                           "peak_frequency_bands": list(a["frequency_peaks"]), "energy_profile": list(a["energy_profile"]),
                           "average_loudness": a["avg_loudness"], "spectral_hash_hex": a["hash"][:8].hex()}
    return out


def similar_report(paths, k=None, threshold=None, as_json=False, ctx=None) -> str:
    """The `similar` command's output: each file's nearest neighbours (k, default 5) among the others, or the pairs
    scoring at least `threshold`, from the fingerprints in the files' META."""
    fps = api.fingerprints_from_files(paths)
    ix = api.FingerprintIndex(fps, ctx)
    try:
        if threshold is not None:
            i, j, s = ix.pairs(threshold)
            pairs = [(paths[a], paths[b], float(c)) for a, b, c in zip(i.tolist(), j.tolist(), s)]
            if as_json:
                return json.dumps({"threshold": threshold, "pairs": [{"a": x, "b": y, "score": c} for x, y, c in pairs]}, indent=2)
            lines = [f"Pairs with similarity >= {threshold}: {len(pairs)}"]
            lines += [f"  {c:.6f}  {x}  {y}" for x, y, c in pairs]
            return "\n".join(lines)
        idx, score = ix.topk_self(5 if k is None else k)
        near = [(p, [(paths[j], float(c)) for j, c in zip(idx[n].tolist(), score[n]) if j != 0xFFFFFFFF])
                for n, p in enumerate(paths)]
        if as_json:
            return json.dumps([{"file": p, "neighbours": [{"file": f, "score": c} for f, c in v]} for p, v in near], indent=2)
        lines = []
        for p, v in near:
            lines.append(p)
            lines += [f"  {c:.6f}  {f}" for f, c in v] or ["  (no other files)"]
        return "\n".join(lines)
    finally:
        ix.close()


def _num(v: float):
    """a float for JSON: non-finite values as the strings "inf", "-inf", "nan" (float() reads them back)"""
    v = float(v)
    return v if v == v and v not in (float("inf"), float("-inf")) else str(v)


def _dbfs(v: float) -> float:
    import math
    return 20.0 * math.log10(v) if v > 0 else float("-inf")


def compare_report(audio_bytes: bytes, flo_bytes: bytes, blocks=False, ctx=None) -> dict:
    """The `compare` command's report: the WAV source against the file's decoded audio (Context.compare), per channel.
    A WAV whose sample rate or channel count differs from the file's header is refused (ValueError)."""
    samples, sr, ch = read_wav_bytes(audio_bytes)
    info = api.probe_container(flo_bytes)
    if sr != info.sample_rate or ch != info.channels:
        raise ValueError(f"the WAV is {sr} Hz / {ch} channels, the file {info.sample_rate} Hz / {info.channels} channels")
    c = ctx or api.default_context()
    r = c.compare(samples, flo_bytes, blocks)
    rep = {"sample_rate": sr, "channels": ch, "compared_frames": r["compared_frames"], "decoded_frames": r["decoded_frames"],
           "source_frames": r["source_frames"], "snr_db": _num(r["snr_db_all"]),
           "per_channel": [{"channel": k, "snr_db": _num(r["snr_db"][k]), "seg_snr_db": _num(r["seg_snr_db"][k]),
                            "seg_blocks": int(r["seg_blocks"][k]), "peak_error_dbfs": _num(_dbfs(float(r["peak_error"][k]))),
                            "peak_error": _num(r["peak_error"][k]), "clipped": int(r["clipped"][k]),
                            "tail_energy": _num(r["tail_energy"][k]), "signal": _num(r["signal"][k]), "error": _num(r["error"][k])}
                           for k in range(ch)]}
    if blocks:
        b = r["blocks"]
        rep["block_snr_db"] = [[_num(api.snr_db(float(b[i, k]["signal"]), float(b[i, k]["error"]))) for k in range(ch)]
                               for i in range(b.shape[0])]
    return rep


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="flo", description="flo audio format converter (MI355X-native encode / decode)")
    sub = ap.add_subparsers(dest="command", required=True)
    e = sub.add_parser("encode", help="Encode a WAV file to flo format")
    e.add_argument("input")
    e.add_argument("output")
    e.add_argument("-l", "--level", type=int, default=5, help="Compression level (0-9, default 5)")
    e.add_argument("--lossy", action="store_true", help="Enable lossy compression mode")
    e.add_argument("--transform", action="store_true", help="Use transform-based lossy")
    e.add_argument("--quality", default="high", help="Lossy quality level (low, medium, high, veryhigh, transparent)")
    e.add_argument("--bitrate", type=int, default=None, help="Target bitrate in kbps (alternative to quality)")
    e.add_argument("--target-kbps", type=float, default=None, help="Lossy: the best measured quality whose file stays within this bitrate")
    e.add_argument("--rate", type=int, default=None, help="Convert to this sample rate (Hz) on the device before encoding")
    e.add_argument("--title", default=None, help="Title metadata")
    e.add_argument("--artist", default=None, help="Artist metadata")
    e.add_argument("--album", default=None, help="Album metadata")
    ed = sub.add_parser("edit", help="Cut, pad, fade and remix a WAV file on the device")
    ed.add_argument("input")
    ed.add_argument("output")
    ed.add_argument("--channels", type=int, default=None, help="Output channels of --matrix")
    ed.add_argument("--matrix", default=None, help="Comma-separated mix matrix, one row per output channel")
    ed.add_argument("--start", type=float, default=None, help="Start of the cut in seconds")
    ed.add_argument("--duration", type=float, default=None, help="Length of the cut in seconds")
    ed.add_argument("--pre-ms", type=float, default=0.0, help="Keep this much in front of the active range")
    ed.add_argument("--post-ms", type=float, default=0.0, help="Keep this much behind the active range")
    ed.add_argument("--fade-in", type=float, default=0.0, help="Linear fade-in in milliseconds")
    ed.add_argument("--fade-out", type=float, default=0.0, help="Linear fade-out in milliseconds")
    ed.add_argument("--pad-head", type=float, default=0.0, help="Seconds of silence in front of the cut")
    ed.add_argument("--pad-tail", type=float, default=0.0, help="Seconds of silence behind the cut")
    for p_ in (e, ed):
        p_.add_argument("--mono", action="store_true", help="Average the channels into one on the device")
        p_.add_argument("--trim-silence", type=float, default=None, metavar="DB", help="Cut to the range of samples above DB dBFS")
    nm = sub.add_parser("normalize", help="Bring a WAV file to a loudness under a true-peak ceiling on the device")
    nm.add_argument("input")
    nm.add_argument("output")
    for p_, need in ((e, False), (nm, True)):
        p_.add_argument("--lufs", type=float, default=None, required=need, help="Target integrated loudness in LUFS")
        p_.add_argument("--ceiling", type=float, default=-1.0, help="True-peak ceiling in dBTP (default -1)")
        p_.add_argument("--limit", action="store_true", help="Apply the full gain and hold the ceiling with a look-ahead limiter")
    mx = sub.add_parser("mix", help="Sum several WAV files at chosen gains and offsets on the device")
    mx.add_argument("inputs", nargs="+")
    mx.add_argument("--out", required=True, help="Output WAV file")
    mx.add_argument("--gains", default=None, help="Comma-separated linear gains, one per input (default 1)")
    mx.add_argument("--at-ms", default=None, help="Comma-separated start offsets in milliseconds, one per input (default 0)")
    cc = sub.add_parser("concat", help="Join several WAV files end to end on the device")
    cc.add_argument("inputs", nargs="+")
    cc.add_argument("--out", required=True, help="Output WAV file")
    cc.add_argument("--crossfade-ms", type=float, default=0.0, help="Linear crossfade between neighbours in milliseconds (default 0)")
    fl = sub.add_parser("filter", help="Low-, high-, band-pass or band-stop a WAV file with a linear-phase FIR on the device")
    fl.add_argument("input")
    fl.add_argument("output")
    which = fl.add_mutually_exclusive_group(required=True)
    which.add_argument("--lowpass", type=float, default=None, metavar="HZ", help="Keep what lies below HZ")
    which.add_argument("--highpass", type=float, default=None, metavar="HZ", help="Keep what lies above HZ")
    which.add_argument("--bandpass", default=None, metavar="LO,HI", help="Keep what lies between LO and HI Hz")
    which.add_argument("--bandstop", default=None, metavar="LO,HI", help="Remove what lies between LO and HI Hz")
    fl.add_argument("--taps", type=int, default=255, help="Filter length, odd (default 255)")
    fl.add_argument("--beta", type=float, default=9.0, help="Kaiser window beta (default 9)")
    cv = sub.add_parser("convolve", help="Convolve a WAV file with an impulse response on the device")
    cv.add_argument("input")
    cv.add_argument("ir")
    cv.add_argument("output")
    cv.add_argument("--tail", action="store_true", help="Keep the response's tail: the output is input + response - 1 frames long")
    cv.add_argument("--method", choices=("direct", "fft", "auto"), default="direct",
                    help="direct: the FIR chain (default); fft: partitioned FFT convolution for long responses; auto: by the measured crossover")
    rs = sub.add_parser("resample", help="Convert a WAV file to another sample rate on the device")
    rs.add_argument("input")
    rs.add_argument("output")
    rs.add_argument("--rate", type=int, required=True, help="Output sample rate in Hz")
    d = sub.add_parser("decode", help="Decode a flo file to WAV")
    d.add_argument("input")
    d.add_argument("output")
    i = sub.add_parser("info", help="Show information about a flo file")
    i.add_argument("input")
    m = sub.add_parser("metadata", help="Display metadata from a flo file")
    m.add_argument("input")
    m.add_argument("--json", action="store_true", help="Output as JSON")
    v = sub.add_parser("validate", help="Validate a flo file")
    v.add_argument("input")
    an = sub.add_parser("analysis", help="Analyze audio with waveform peaks and spectral fingerprinting")
    an.add_argument("input")
    an.add_argument("-w", "--waveform", action="store_true", help="Show waveform peaks")
    an.add_argument("-s", "--spectrum", action="store_true", help="Show spectral fingerprint")
    an.add_argument("--json", action="store_true", help="Output as JSON")
    si = sub.add_parser("similar", help="Find similar files by their spectral fingerprints")
    si.add_argument("inputs", nargs="+", metavar="input")
    sg = si.add_mutually_exclusive_group()
    sg.add_argument("-k", type=int, default=None, help="Nearest neighbours per file (default 5, at most 64)")
    sg.add_argument("--threshold", type=float, default=None, help="List every pair scoring at least this")
    si.add_argument("--json", action="store_true", help="Output as JSON")
    cp = sub.add_parser("compare", help="Compare a flo file's decoded audio with its source WAV")
    cp.add_argument("source")
    cp.add_argument("input")
    cp.add_argument("--json", action="store_true", help="Output as JSON")
    cp.add_argument("--blocks", action="store_true", help="Also print the SNR of every 1024-frame block")
    cu = sub.add_parser("curve", help="File size at every quality of a grid, measured on the device")
    cu.add_argument("input")
    cu.add_argument("--json", action="store_true", help="Output as JSON")
    la = sub.add_parser("ladder", help="Encode a WAV file at every quality of a list, from one transform pass")
    la.add_argument("input")
    la.add_argument("outdir")
    la.add_argument("--qualities", required=True, help="Comma-separated rungs: low, medium, high, veryhigh, transparent")
    la.add_argument("--json", action="store_true", help="Output as JSON")
    la.add_argument("--title", default=None, help="Title metadata")
    la.add_argument("--artist", default=None, help="Artist metadata")
    la.add_argument("--album", default=None, help="Album metadata")
    a = ap.parse_args(argv)
    try:
        if a.command == "encode":
            print(f"Reading {a.input}...")
            audio = open(a.input, "rb").read()
            samples, sr, ch = read_wav_bytes(audio)
            print(f"  Sample rate: {sr} Hz")
            print(f"  Channels: {ch}")
            print(f"  Duration: {samples.size / ch / sr:.2f}s")
            edit = edit_options(mono=a.mono, trim_silence=a.trim_silence)
            level = level_options(a.lufs, a.ceiling, a.limit)
            pcm = None
            if edit is not None:
                print("Editing on the device...")
            if a.rate is not None and a.rate != sr:
                print(f"Converting to {a.rate} Hz...")
                if edit is None:
                    samples, sr, ch = _read_at_rate(audio, a.rate)
            if level is not None:
                print(f"Normalising to {a.lufs:g} LUFS under {a.ceiling:g} dBTP{' (limiter)' if a.limit else ''}...")
            if edit is not None:   # the edit runs once: what it makes is converted, levelled and handed to the encode
                pcm = samples, sr, ch = _read_at_rate(audio, a.rate, level=level, edit=edit)
                print(f"  Edited: {ch} channels, {samples.size / ch / sr:.2f}s")
            lossy = a.lossy or a.transform
            if a.target_kbps is not None:
                print(f"Encoding to flo (lossy, at most {a.target_kbps:g} kbps, measured)...")
                flo, info = encode_to_target(audio, a.target_kbps, a.title, a.artist, a.album, rate=a.rate, normalize=level, pcm=pcm)
                secs = samples.size / ch / sr
                print(f"  Quality: {info['quality']:.4f} (candidate {info['index']}){'' if info['fits'] else ' - the target is below the smallest file'}")
                print(f"  Achieved: {(len(flo) * 8 / 1000 / secs) if secs else 0.0:.1f} kbps ({len(flo)} of {info['target_bytes']} bytes)")
            elif lossy or a.bitrate is not None:
                if a.bitrate is not None:
                    print(f"Encoding to flo (lossy, ~{a.bitrate} kbps)...")
                    q = None
                else:
                    if a.quality.lower() not in QUALITY:
                        print(f"Invalid quality level: {a.quality}. Use: low, medium, high, veryhigh, transparent", file=sys.stderr)
                        return 1
                    q = QUALITY[a.quality.lower()]
                    print(f"Encoding to flo (lossy, {a.quality} quality)...")
                flo = encode_from_audio(audio, a.level, True, q if q is not None else 0.6, a.bitrate, None, a.title, a.artist, a.album, rate=a.rate, normalize=level, pcm=pcm)
            else:
                print("Encoding to flo (lossless)...")
                flo = encode_from_audio(audio, a.level, title=a.title, artist=a.artist, album=a.album, rate=a.rate, normalize=level, pcm=pcm)
            open(a.output, "wb").write(flo)
            original = int(samples.size * 4)
            print("Done!")
            print(f"  Output: {a.output}")
            print(f"  Size: {len(flo)} bytes ({original / max(len(flo), 1):.1f}x compression)")
        elif a.command == "edit":
            print(f"Reading {a.input}...")
            audio = open(a.input, "rb").read()
            samples, sr, ch = read_wav_bytes(audio)
            print(f"  Sample rate: {sr} Hz")
            print(f"  Channels: {ch}")
            print(f"  Duration: {samples.size / ch / sr:.2f}s")
            opts = edit_options(a.mono, a.channels, a.matrix, a.start, a.duration, a.trim_silence, a.pre_ms, a.post_ms, a.fade_in,
                                a.fade_out, a.pad_head, a.pad_tail)
            print("Editing on the device...")
            wav, info = edit_wav(audio, opts)
            open(a.output, "wb").write(wav)
            if "active" in info:
                print(f"  Active range: frames {info['active'][0]} .. {info['active'][1]}")
            g = info["segment"]
            print(f"  Cut: frames {g['start']} .. {g['start'] + g['frames']}, fades {g['fade_in']} / {g['fade_out']}, pads {g['pad_head']} / {g['pad_tail']}")
            print("Done!")
            print(f"  Output: {a.output}")
        elif a.command in ("mix", "concat"):
            print(f"Reading {len(a.inputs)} files...")
            wavs = [open(p, "rb").read() for p in a.inputs]
            if a.command == "mix":
                print("Mixing on the device...")
                wav = mix_wavs(wavs, a.gains, a.at_ms)
            else:
                print(f"Joining on the device (crossfade {a.crossfade_ms:g} ms)...")
                wav = concat_wavs(wavs, a.crossfade_ms)
            open(a.out, "wb").write(wav)
            samples, sr, ch = read_wav_bytes(wav)
            print(f"  Sample rate: {sr} Hz")
            print(f"  Channels: {ch}")
            print(f"  Duration: {samples.size / ch / sr:.2f}s")
            print("Done!")
            print(f"  Output: {a.out}")
        elif a.command in ("filter", "convolve"):
            print(f"Reading {a.input}...")
            audio = open(a.input, "rb").read()
            samples, sr, ch = read_wav_bytes(audio)
            print(f"  Sample rate: {sr} Hz")
            print(f"  Channels: {ch}")
            print(f"  Duration: {samples.size / ch / sr:.2f}s")
            if a.command == "filter":
                kind, f_lo, f_hi = filter_options(a.lowpass, a.highpass, a.bandpass, a.bandstop)
                print(f"Filtering on the device ({kind}, {a.taps} taps)...")
                wav = filter_wav(audio, kind, f_lo, f_hi, a.taps, a.beta)
            else:
                print(f"Convolving with {a.ir} on the device...")
                wav = convolve_wavs(audio, open(a.ir, "rb").read(), a.tail, method=a.method)
            open(a.output, "wb").write(wav)
            print("Done!")
            print(f"  Output: {a.output}")
        elif a.command == "resample":
            print(f"Reading {a.input}...")
            audio = open(a.input, "rb").read()
            samples, sr, ch = read_wav_bytes(audio)
            print(f"  Sample rate: {sr} Hz")
            print(f"  Channels: {ch}")
            print(f"  Duration: {samples.size / ch / sr:.2f}s")
            print(f"Converting to {a.rate} Hz...")
            wav = resample_wav(audio, a.rate)
            open(a.output, "wb").write(wav)
            print("Done!")
            print(f"  Output: {a.output}")
        elif a.command == "normalize":
            print(f"Reading {a.input}...")
            audio = open(a.input, "rb").read()
            samples, sr, ch = read_wav_bytes(audio)
            print(f"  Sample rate: {sr} Hz")
            print(f"  Channels: {ch}")
            print(f"  Duration: {samples.size / ch / sr:.2f}s")
            print(f"Normalising to {a.lufs:g} LUFS under {a.ceiling:g} dBTP{' (limiter)' if a.limit else ''}...")
            wav, r = normalize_wav(audio, a.lufs, a.ceiling, a.limit)
            open(a.output, "wb").write(wav)
            print(f"  Input: {r['input_lufs']:.2f} LUFS, true peak {r['input_true_peak_dbtp']:.2f} dBTP")
            if r["status"]:
                print(f"  Copied unchanged: {r['status']}")
            else:
                print(f"  Gain: {r['gain_db']:+.2f} dB" + (f" ({r['ceiling_reduction_db']:.2f} dB taken off by the ceiling)" if r["ceiling_reduction_db"] else ""))
                if a.limit:
                    print(f"  Limited frames: {r['limited_frames']} (deepest {r['min_gain_db']:.2f} dB)")
            print("Done!")
            print(f"  Output: {a.output}")
        elif a.command == "decode":
            print(f"Reading {a.input}...")
            flo = open(a.input, "rb").read()
            info = flo_info(flo)
            print(f"  Sample rate: {info['sample_rate']} Hz")
            print(f"  Channels: {info['channels']}")
            print(f"  Duration: {info['duration_secs']:.2f}s")
            print("Decoding...")
            wav = decode_to_wav(flo)
            print("Writing WAV...")
            open(a.output, "wb").write(wav)
            print("Done!")
            print(f"  Output: {a.output}")
        elif a.command == "info":
            info = flo_info(open(a.input, "rb").read())
            print("flo Audio File")
            print("-" * 31)
            print(f"  Version:     {info['version']}")
            print(f"  Sample rate: {info['sample_rate']} Hz")
            print(f"  Channels:    {info['channels']}")
            print(f"  Bit depth:   {info['bit_depth']}")
            print(f"  Duration:    {info['duration_secs']:.2f}s")
            print(f"  Total sample-frames: {info['total_samples']}")
            print(f"  File size:   {info['file_size']} bytes")
            print(f"  Compression: {info['compression_ratio']:.1f}x")
            print(f"  CRC valid:   {'yes' if info['crc_valid'] else 'no'}")
            if info["is_lossy"]:
                ql = info["lossy_quality"]
                print(f"  Encoding:    Lossy ({QUALITY_NAMES[ql] if ql < len(QUALITY_NAMES) else 'Unknown'})")
            else:
                print("  Encoding:    Lossless")
        elif a.command == "metadata":
            md = get_metadata(open(a.input, "rb").read())
            if md is None:
                print("null" if a.json else "No metadata present")
            elif a.json:
                print(json.dumps(md, indent=2, default=lambda b: f"<{len(b)} bytes>"))
            else:
                for k, v in md.items():
                    shown = f"<{len(v)} bytes>" if isinstance(v, (bytes, list)) and len(v) > 16 else v
                    print(f"  {k}: {shown}")
        elif a.command == "analysis":
            rep = analysis_report(open(a.input, "rb").read(), a.waveform, a.spectrum)
            if a.json:
                print(json.dumps(rep, indent=2))
            else:
                fi, lo = rep["file_info"], rep["loudness"]
                print(f"Analyzing {a.input}...")
                print()
                print("File Information")
                print("\u2500" * 16)
                print(f"  Sample rate: {fi['sample_rate']} Hz")
                print(f"  Channels:    {fi['channels']}")
                print(f"  Bit depth:   {fi['bit_depth']} bits")
                print(f"  Duration:    {fi['duration_secs']:.2f}s")
                print(f"  Total samples: {fi['total_samples']}")
                print()
                print("Loudness Metrics (EBU R128)")
                print("\u2500" * 28)
                print(f"  Integrated loudness: {lo['integrated_lufs']:.2f} LUFS")
                print(f"  Loudness range:      {lo['loudness_range_lu']:.2f} LU")
                print(f"  True peak:           {lo['true_peak_dbtp']:.2f} dBTP")
                print(f"  Sample peak:         {lo['sample_peak_dbfs']:.2f} dBFS")
                print()
                if rep["waveform"]:
                    wf = rep["waveform"]
                    print("Waveform Analysis")
                    print("\u2500" * 17)
                    print(f"  Peaks per second:    {wf['peaks_per_second']}")
                    print(f"  Total peaks:         {wf['total_peaks']}")
                    print(f"  Channels:            {wf['channels']}")
                    if wf["peak_statistics"]:
                        st = wf["peak_statistics"]
                        print("  Peak statistics:")
                        print(f"    Min:               {st['min']:.6f}")
                        print(f"    Max:               {st['max']:.6f}")
                        print(f"    Average:           {st['average']:.6f}")
                    print()
                if rep["spectral"]:
                    sp = rep["spectral"]
                    print("Spectral Analysis")
                    print("\u2500" * 17)
                    print(f"  Duration:            {sp['duration_ms']} ms")
                    print(f"  Sample rate:         {sp['sample_rate']} Hz")
                    print(f"  Channels:            {sp['channels']}")
                    print(f"  Peak frequency bands: {sp['peak_frequency_bands']}")
                    print(f"  Energy profile (16 bands): {sp['energy_profile']}")
                    print(f"  Average loudness:    {sp['average_loudness']}")
                    print(f"  Spectral hash (first 8 bytes):   {sp['spectral_hash_hex']}")
                    print()
        elif a.command == "curve":
            rows = curve_report(open(a.input, "rb").read())
            if a.json:
                print(json.dumps(rows, indent=2))
            else:
                print(f"{'quality':>8}  {'bytes':>12}  {'kbps':>9}")
                for r in rows:
                    print(f"{r['quality']:8.4f}  {r['bytes']:12d}  {r['kbps']:9.1f}")
        elif a.command == "ladder":
            import os
            try:
                rungs = parse_rungs(a.qualities)
            except ValueError as ex:
                print(ex, file=sys.stderr)
                return 1
            audio = open(a.input, "rb").read()
            samples, sr, ch = read_wav_bytes(audio)
            files = ladder_from_audio(audio, rungs, None, a.title, a.artist, a.album)
            os.makedirs(a.outdir, exist_ok=True)
            stem = os.path.splitext(os.path.basename(a.input))[0]
            secs = samples.size / ch / sr
            rows = []
            for j, (q, f) in enumerate(zip(rungs, files)):
                path = os.path.join(a.outdir, f"{stem}.r{j}.flo")
                open(path, "wb").write(f)
                rows.append({"rung": j, "quality": float(q), "bytes": len(f), "kbps": (len(f) * 8 / 1000 / secs) if secs else 0.0})
            if a.json:
                print(json.dumps(rows, indent=2))
            else:
                print(f"{'rung':>4}  {'quality':>8}  {'bytes':>12}  {'kbps':>9}")
                for r in rows:
                    print(f"{r['rung']:4d}  {r['quality']:8.4f}  {r['bytes']:12d}  {r['kbps']:9.1f}")
        elif a.command == "similar":
            print(similar_report(a.inputs, a.k, a.threshold, a.json))
        elif a.command == "compare":
            rep = compare_report(open(a.source, "rb").read(), open(a.input, "rb").read(), a.blocks)
            if a.json:
                print(json.dumps(rep, indent=2))
            else:
                print(f"Comparing {a.input} with {a.source}")
                print(f"  Sample rate: {rep['sample_rate']} Hz, channels: {rep['channels']}")
                print(f"  Frames: {rep['compared_frames']} compared, {rep['decoded_frames']} decoded, "
                      f"{rep['source_frames']} in the source")
                print(f"  SNR (all channels): {float(rep['snr_db']):.4f} dB")
                for p in rep["per_channel"]:
                    print(f"  Channel {p['channel']}: SNR {float(p['snr_db']):.4f} dB, segmental SNR {float(p['seg_snr_db']):.4f} dB "
                          f"({p['seg_blocks']} blocks), peak error {float(p['peak_error_dbfs']):.4f} dBFS, "
                          f"clipped {p['clipped']}, tail energy {float(p['tail_energy']):.6e}")
                if a.blocks:
                    print("  Block SNR (dB), one column per channel:")
                    for i, row in enumerate(rep["block_snr_db"]):
                        print(f"    {i:6d}  " + "  ".join(f"{float(v):9.4f}" for v in row))
        elif a.command == "validate":
            try:
                ok = flo_info(open(a.input, "rb").read())["crc_valid"]
            except api.FloError:
                ok = False
            print("Valid flo file" if ok else "Invalid flo file")
            return 0 if ok else 1
    except (OSError, WavError, ValueError, api.FloError) as ex:
        print(f"Error: {ex}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
