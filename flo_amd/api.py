"""Host-side mirror of libflo's encoder interface, bound to the HIP library through its C ABI.

Same names, argument meaning and error behaviour as the reference (all paths under /root/reference):
  Encoder(sample_rate, channels, bit_depth).with_compression(level).encode(samples, metadata)
        -> libflo/src/lossless/encoder.rs:17-45
  LossyEncoder / TransformEncoder(sample_rate, channels, quality).encode_to_flo(samples, metadata)
        -> libflo/src/lossy/encoder.rs:36-53,167-239 (re-export lib.rs:21-24)
  QualityPreset                      -> libflo/src/lossy/mod.rs:19-128
  encode / encode_lossy / encode_with_bitrate (free functions: analysis metadata first, as the reference)
        -> libflo/src/lib.rs:97-206, 219-283
Errors surface as FloError(message), the analogue of FloResult<T> = Result<T, String> (core/types.rs:281).
"""
import ctypes as C
import enum
import math
import threading
import weakref
from typing import NamedTuple

import numpy as np

from . import _native
from ._native import FloError, MODE_LOSSLESS, MODE_LOSSY


class QualityPreset(enum.IntEnum):
    """lossy/mod.rs:19-128"""
    Low = 0
    Medium = 1
    High = 2
    VeryHigh = 3
    Transparent = 4

    def as_f32(self) -> float:
        return [0.0, 0.35, 0.55, 0.75, 1.0][int(self)]

    @staticmethod
    def from_f32(q: float) -> "QualityPreset":
        if q < 0.2:
            return QualityPreset.Low
        if q < 0.45:
            return QualityPreset.Medium
        if q < 0.65:
            return QualityPreset.High
        if q < 0.85:
            return QualityPreset.VeryHigh
        return QualityPreset.Transparent

    @staticmethod
    def from_bitrate(bitrate_kbps: int, sample_rate: int, channels: int) -> "QualityPreset":
        raw_kbps = (sample_rate * channels * 16) // 1000
        ratio = np.float32(raw_kbps) / np.float32(bitrate_kbps)
        if ratio > 20.0:
            return QualityPreset.Low
        if ratio > 10.0:
            return QualityPreset.Medium
        if ratio > 6.0:
            return QualityPreset.High
        if ratio > 4.0:
            return QualityPreset.VeryHigh
        return QualityPreset.Transparent

    def expected_ratio(self) -> float:
        return [30.0, 10.0, 6.0, 4.0, 3.0][int(self)]

    def equivalent_bitrate(self) -> int:
        return [48, 128, 192, 256, 320][int(self)]


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1)


class _CBuffer:
    """keeps a buffer the library handed out (flo_free) alive for as long as an array looks at it"""

    def __init__(self, lib, ptr):
        self._lib, self._ptr = lib, C.c_void_p(ptr.value)

    def __del__(self):
        if self._ptr.value:
            self._lib.flo_free(self._ptr)
            self._ptr = C.c_void_p()


def _analysis_dict(a, peaks):
    return dict(peaks=peaks, hash=bytes(a.hash), duration_ms=a.duration_ms, sample_rate=a.sample_rate,
                channels=a.channels, frequency_peaks=list(a.frequency_peaks), energy_profile=list(a.energy_profile),
                avg_loudness=a.avg_loudness, integrated_lufs=a.integrated_lufs, length_ms=a.length_ms,
                loudness_range_lu=a.loudness_range_lu, true_peak_dbtp=a.true_peak_dbtp, sample_peak_dbfs=a.sample_peak_dbfs,
                sum_squares=np.float32(a.sum_squares))


class Context:
    """One per host thread / GPU (flo_ctx). A context, and every object built on it (Batch, Ladder, Corpus, the streaming
    encoders and decoders, FingerprintIndex, Encoder, Decoder, ...), is used by one thread at a time: it carries no lock. The
    contexts of a process are independent, so a pool of threads gives each worker its own. An object built without ctx=
    keeps default_context() of the thread that built it and belongs to that thread. Encoder, LossyEncoder and
    TransformEncoder hold no device state and keep no context when built without one: each call of theirs runs on the
    calling thread's default_context()."""

    def __init__(self, device: int = 0):
        self._L = _native.lib()
        h = C.c_void_p()
        rc = self._L.flo_ctx_create(device, C.byref(h))
        if rc != 0:
            raise FloError(self._L.flo_last_create_error().decode())
        self._h = h
        self.device = device
        self._batches = weakref.WeakSet()   # batches hold device memory of this context: they go first

    def close(self):
        if getattr(self, "_h", None):
            for g in list(getattr(self, "_dists", ())):   # communicators made on this context go first (flo_dist_destroy uses it)
                g.close()
            for b in list(self._batches):
                b.close()
            self._L.flo_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise FloError(self._L.flo_last_error(self._h).decode())

    def _take(self, ptr, n):
        data = C.string_at(ptr.value, n.value) if ptr.value else b""
        self._L.flo_free(ptr)
        return data

    def device_info(self):
        name = C.create_string_buffer(256)
        cus, hbm = C.c_int(), C.c_uint64()
        self._chk(self._L.flo_ctx_device_info(self._h, name, 256, C.byref(cus), C.byref(hbm)))
        return name.value.decode(), cus.value, hbm.value

    def force_path(self, which: int):
        self._chk(self._L.flo_ctx_force_path(self._h, which))

    def reserve_cus(self, n: int):
        """compute units the persistent encode kernels leave free (for RCCL's kernels when ranks exchange files)"""
        self._chk(self._L.flo_ctx_reserve_cus(self._h, n))

    def reserved_cus(self) -> int:
        """compute units the persistent encode kernels currently leave free"""
        return int(self._L.flo_ctx_reserved_cus(self._h))

    def resample(self, samples, in_rate, out_rate, channels):
        """flo_resample: the interleaved f32 clip at out_rate (one upload, the batch kernel, one fetch)"""
        p = _f32(samples)
        out, n = C.c_void_p(), C.c_size_t()
        self._chk(self._L.flo_resample(self._h, p.ctypes.data, p.size, in_rate, out_rate, channels, C.byref(out), C.byref(n)))
        res = np.frombuffer(C.string_at(out.value, n.value * 4), np.float32).copy() if n.value else np.zeros(0, np.float32)
        self._L.flo_free(out)
        return res

    def normalize(self, samples, sample_rate, channels, target_lufs=-14.0, ceiling_dbtp=-1.0, limit=False, lookahead_ms=1.5,
                  max_gain_db=30.0):
        """flo_normalize: (the interleaved f32 clip at target_lufs under ceiling_dbtp, its report): one upload, the batch's
        measurements and kernel, one fetch. Whole sample-frames come back"""
        p = _f32(samples)
        opts = _normalize_opts(sample_rate, target_lufs, ceiling_dbtp, limit, lookahead_ms, max_gain_db)
        out, rep = C.c_void_p(), _native.NormalizeReport()
        self._chk(self._L.flo_normalize(self._h, p.ctypes.data, p.size, sample_rate, channels, C.byref(opts), C.byref(out), C.byref(rep)))
        n = p.size // channels * channels
        res = np.frombuffer(C.string_at(out.value, n * 4), np.float32).copy() if n else np.zeros(0, np.float32)
        self._L.flo_free(out)
        return res, _normalize_report(rep)

    def true_peak(self, samples, sample_rate, channels) -> float:
        """the clip's 4x oversampled peak in dBTP (Batch.true_peaks of a batch of this clip)"""
        p = _f32(samples)
        b = Batch(self, MODE_LOSSLESS, [p.size], sample_rate, channels, 0)
        try:
            self._chk(self._L.flo_batch_upload(b._h, 0, p.ctypes.data))
            return float(b.true_peaks()[0])
        finally:
            b.close()

    def edit(self, samples, sample_rate, channels, segment=None, out_channels=None, matrix=None):
        """flo_edit: one cut of the interleaved f32 clip, padded, faded and mixed to out_channels (one upload, the batch
        kernel, one fetch). segment: a dict as Batch.edit takes (clip is 0); None: the whole clip"""
        p = _f32(samples)
        segs = _edit_segments([dict(segment or {}, clip=0)], [p.size // channels])
        cout, m = _edit_matrix(channels, out_channels, matrix)
        out, n = C.c_void_p(), C.c_size_t()
        self._chk(self._L.flo_edit(self._h, p.ctypes.data, p.size, sample_rate, channels, segs, cout, m.ctypes.data if m is not None else None,
                                   C.byref(out), C.byref(n)))
        res = np.frombuffer(C.string_at(out.value, n.value * 4), np.float32).copy() if n.value else np.zeros(0, np.float32)
        self._L.flo_free(out)
        return res

    def mix(self, clips, sample_rate, channels, parts, out_frames=None):
        """flo_mix: one output clip summed from parts of the interleaved f32 clips (one upload, the batch kernel, one fetch).
        parts: dicts as Batch.mix takes (batch and out are 0); out_frames None: the end of the furthest part"""
        ps = [_f32(x) for x in clips]
        arr = _mix_parts(parts, [[p.size // channels for p in ps]])
        if out_frames is None:
            out_frames = max([int(g.at) + int(g.frames) for g in arr], default=0)
        ptrs = (C.c_void_p * max(len(ps), 1))(*[p.ctypes.data for p in ps])
        lens = (C.c_size_t * max(len(ps), 1))(*[p.size for p in ps])
        out, n = C.c_void_p(), C.c_size_t()
        self._chk(self._L.flo_mix(self._h, len(ps), ptrs, lens, sample_rate, channels, len(arr), arr, int(out_frames), C.byref(out), C.byref(n)))
        res = np.frombuffer(C.string_at(out.value, n.value * 4), np.float32).copy() if n.value else np.zeros(0, np.float32)
        self._L.flo_free(out)
        return res

    def convolve(self, samples, ir, sample_rate, channels, ir_channels=1, job=None, *, mode="head", taps=None, method="direct"):
        """flo_convolve: the interleaved f32 clip filtered by the interleaved f32 response `ir` of ir_channels (1 or channels)
        channels (one upload each, the batch kernel, one fetch). job: a dict as Batch.convolve takes (clip and ir are 0) or a
        _native.ConvJob; None: the whole response in `mode` (Batch.convolve), at most `taps` taps. method: as Batch.convolve
        ("fft", or "auto" from crossover_taps on: flo_convolve_fft)"""
        p, h = _f32(samples), _f32(ir)
        jobs = _conv_jobs(None if job is None else [job if isinstance(job, _native.ConvJob) else dict(job, clip=0, ir=0)],
                          [p.size // channels], [h.size // ir_channels], 0, mode, taps)
        out, n = C.c_void_p(), C.c_size_t()
        fn = self._L.flo_convolve_fft if _conv_takes_fft(method, jobs, [h.size // ir_channels], channels, ir_channels) else self._L.flo_convolve
        self._chk(fn(self._h, p.ctypes.data, p.size, h.ctypes.data, h.size, sample_rate, channels, ir_channels, jobs, C.byref(out), C.byref(n)))
        res = np.frombuffer(C.string_at(out.value, n.value * 4), np.float32).copy() if n.value else np.zeros(0, np.float32)
        self._L.flo_free(out)
        return res

    def upload_path(self):
        """(path large host uploads take on this host, GB/s the probe measured for pageable-direct, for the pinned ring)"""
        name, a, b = C.create_string_buffer(64), C.c_double(), C.c_double()
        self._chk(self._L.flo_ctx_upload_path(self._h, name, 64, C.byref(a), C.byref(b)))
        return name.value.decode(), a.value, b.value

    # -- one clip ---------------------------------------------------------------------------------------

    def encode_lossy(self, samples, sample_rate, channels, quality, metadata=b"") -> bytes:
        p = _f32(samples)
        out, n = C.c_void_p(), C.c_size_t()
        self._chk(self._L.flo_encode_lossy(self._h, p.ctypes.data, p.size, sample_rate, channels, quality,
                                           metadata, len(metadata), C.byref(out), C.byref(n)))
        return self._take(out, n)

    def encode_lossless(self, samples, sample_rate, channels, bit_depth=16, level=5, metadata=b"") -> bytes:
        p = _f32(samples)
        out, n = C.c_void_p(), C.c_size_t()
        self._chk(self._L.flo_encode_lossless(self._h, p.ctypes.data, p.size, sample_rate, channels, bit_depth, level,
                                              metadata, len(metadata), C.byref(out), C.byref(n)))
        return self._take(out, n)

    def encode_batch(self, mode, clips, sample_rate, channels, quality_or_level):
        arrs = [_f32(c) for c in clips]
        k = len(arrs)
        ptrs = (C.c_void_p * k)(*[a.ctypes.data for a in arrs])
        lens = (C.c_size_t * k)(*[a.size for a in arrs])
        outs, olens = (C.c_void_p * k)(), (C.c_size_t * k)()
        self._chk(self._L.flo_encode_batch(self._h, mode, k, ptrs, lens, sample_rate, channels, quality_or_level, outs, olens))
        res = []
        for i in range(k):
            res.append(C.string_at(outs[i], olens[i]) if outs[i] else b"")
            self._L.flo_free(outs[i])
        return res

    def encode_batch_to_size(self, clips, sample_rate, channels, qualities, target_bytes, metadata=None):
        """flo_encode_batch_to_size: (files, chosen, fits) - every clip at the best candidate quality whose whole file,
        META included, fits target_bytes[i]; one upload, one size curve, one encode per clip"""
        arrs = [_f32(c) for c in clips]
        k = len(arrs)
        q = np.ascontiguousarray(qualities, dtype=np.float32).reshape(-1)
        tb = np.ascontiguousarray(target_bytes, dtype=np.uint64).reshape(-1)
        if tb.size != k:
            raise ValueError(f"{tb.size} targets for {k} clips")
        ptrs = (C.c_void_p * k)(*[a.ctypes.data for a in arrs])
        lens = (C.c_size_t * k)(*[a.size for a in arrs])
        mp = ml = None
        if metadata is not None:
            metas = [bytes(m or b"") for m in metadata]
            if len(metas) != k:
                raise ValueError(f"metadata has {len(metas)} entries for {k} clips")
            keep = [C.create_string_buffer(m, len(m)) if m else None for m in metas]
            mp = (C.c_void_p * k)(*[C.addressof(x) if x is not None else None for x in keep])
            ml = (C.c_size_t * k)(*[len(m) for m in metas])
        outs, olens = (C.c_void_p * k)(), (C.c_size_t * k)()
        chosen, fits = np.zeros(max(k, 1), np.uint32), np.zeros(max(k, 1), np.int32)
        self._chk(self._L.flo_encode_batch_to_size(self._h, k, ptrs, lens, sample_rate, channels, q.size, q.ctypes.data, tb.ctypes.data,
                                                   mp, ml, outs, olens, chosen.ctypes.data, fits.ctypes.data))
        res = []
        for i in range(k):
            res.append(C.string_at(outs[i], olens[i]) if outs[i] else b"")
            self._L.flo_free(outs[i])
        return res, [int(x) for x in chosen[:k]], [bool(x) for x in fits[:k]]

    def decode(self, flo: bytes, with_info=False):
        """libflo::decode (lib.rs:296-315): interleaved f32 PCM of a .flo file, decoded on the device."""
        return self._decode(self._L.flo_decode, np.float32, flo, with_info)

    def decode_lossless_i32(self, flo: bytes, with_info=False):
        """the integers a lossless file decodes to, before the 1/32767 scaling (bit-exact parity checks)"""
        return self._decode(self._L.flo_decode_lossless_i32, np.int32, flo, with_info)

    def _decode(self, fn, dtype, flo, with_info):
        flo = bytes(flo)
        out, n = C.c_void_p(), C.c_size_t()
        sr, ch = C.c_uint32(), C.c_uint8()
        self._chk(fn(self._h, flo, len(flo), C.byref(out), C.byref(n), C.byref(sr), C.byref(ch)))
        if n.value:
            # the array IS the library's buffer (freed with it): two more copies of a 3-minute file's 63 MB, each into fresh
            # pages, cost four times what the decode itself does
            buf = (C.c_char * (n.value * 4)).from_address(out.value)
            buf._flo_owner = _CBuffer(self._L, out)
            a = np.frombuffer(buf, dtype=dtype)
        else:
            self._L.flo_free(out)
            a = np.zeros(0, dtype)
        return (a, sr.value, ch.value) if with_info else a

    def decode_frame_at(self, flo: bytes, frame_index: int):
        """seeking::decode_frame_at (seeking.rs:43-63): the interleaved f32 samples of one frame, decoded on the device"""
        flo = bytes(flo)
        out, n = C.c_void_p(), C.c_size_t()
        self._chk(self._L.flo_decode_frame_at(self._h, flo, len(flo), int(frame_index), C.byref(out), C.byref(n)))
        a = np.ctypeslib.as_array((C.c_float * n.value).from_address(out.value)).copy() if n.value else np.zeros(0, np.float32)
        self._L.flo_free(out)
        return a

    def compare(self, samples, flo: bytes, blocks=False):
        """How far a .flo file's decoded audio lies from `samples` (its source, interleaved f32 with the file's channel
        count), measured on the device (flo_compare, include/flo_hip.h): a dict as fidelity_dict returns it."""
        p = _f32(samples)
        flo = bytes(flo)
        ch = max(int(probe_container(flo).channels), 1)
        out = np.zeros(ch, FIDELITY_DTYPE)
        cap = ((p.size // ch + 1023) // 1024) * ch   # n_blocks <= ceil(source frames / 1024)
        blk = np.zeros(max(cap, 1), FIDELITY_BLOCK_DTYPE) if blocks else None
        nb = C.c_size_t()
        self._chk(self._L.flo_compare(self._h, p.ctypes.data, p.size, flo, len(flo), out.ctypes.data,
                                      blk.ctypes.data if blocks else None, cap if blocks else 0, C.byref(nb)))
        return fidelity_dict(out, blk[:nb.value * ch].reshape(-1, ch) if blocks else None)

    def get_toc(self, flo: bytes):
        return get_toc(flo)

    def seek_to_time(self, flo: bytes, target_ms: int):
        return seek_to_time(flo, target_ms)

    # -- analysis metadata of libflo::encode* (lib.rs:219-283) ---------------------------------------------------
    def analyze(self, samples, sample_rate, channels, peaks_per_second=50):
        """waveform peaks, spectral fingerprint and EBU R128 integrated loudness, computed on the device"""
        p = _f32(samples)
        peaks = np.zeros(int(np.ceil(p.size // max(channels, 1) * peaks_per_second / max(sample_rate, 1))) + 16, np.float32)
        a = _native.Analysis()
        self._chk(self._L.flo_analyze(self._h, p.ctypes.data, p.size, sample_rate, channels, peaks_per_second,
                                      peaks.ctypes.data, peaks.size, C.byref(a)))
        return _analysis_dict(a, peaks[: a.n_peaks].copy())

    def analysis_metadata(self, samples, sample_rate, channels, peaks_per_second=50) -> bytes:
        """add_analysis_data_if_missing(&[], ...): the MessagePack META libflo::encode* build for an empty input META"""
        p = _f32(samples)
        out, n = C.c_void_p(), C.c_size_t()
        self._chk(self._L.flo_analysis_metadata(self._h, p.ctypes.data, p.size, sample_rate, channels, peaks_per_second,
                                                C.byref(out), C.byref(n)))
        return self._take(out, n)

    # -- stage-level entry points (parity tests) -----------------------------------------------------------
    def mdct_forward(self, frames):
        f = _f32(frames)
        n = f.size // 2048
        out = np.zeros(n * 1024, np.float32)
        self._chk(self._L.flo_mdct_forward(self._h, f.ctypes.data, n, out.ctypes.data))
        return out.reshape(n, 1024)

    def lossy_analyze(self, samples, sample_rate, channels, quality):
        p = _f32(samples)
        hops = ((p.size // channels) + 1024 + 1023) // 1024
        coeffs = np.zeros((hops, channels, 1024), np.float32)
        q = np.zeros((hops, channels, 1024), np.int16)
        sfw = np.zeros((hops, channels, 25), np.uint16)
        nh = C.c_size_t()
        self._chk(self._L.flo_lossy_analyze(self._h, p.ctypes.data, p.size, sample_rate, channels, quality,
                                            coeffs.ctypes.data, q.ctypes.data, sfw.ctypes.data, C.byref(nh)))
        assert nh.value == hops
        return dict(coeffs=coeffs, q=q, sf_words=sfw)

    def lossy_quantize(self, coeffs, sample_rate, quality, exact=False):
        """Device psychoacoustics + quantiser on caller-supplied spectra. exact=False is the quantiser every encode
        runs; exact=True adds the reference's dB-domain re-check next to the threshold (test yardstick)."""
        c = np.ascontiguousarray(coeffs, np.float32)
        hops, channels = c.shape[0], c.shape[1]
        q = np.zeros((hops, channels, 1024), np.int16)
        sfw = np.zeros((hops, channels, 25), np.uint16)
        self._chk(self._L.flo_lossy_quantize(self._h, c.ctypes.data, hops, sample_rate, channels, quality, 1 if exact else 0,
                                             q.ctypes.data, sfw.ctypes.data))
        return dict(q=q, sf_words=sfw)

    def lossy_pack_frames(self, coeffs, sample_rate, quality):
        """lossy_quantize that keeps the frames: the clip's DATA bytes and frame sizes beside the integers and scale words,
        in the form force_path names (5, 2, else 1)."""
        c = np.ascontiguousarray(coeffs, np.float32)
        hops, channels = c.shape[0], c.shape[1]
        q = np.zeros((hops, channels, 1024), np.int16)
        sfw = np.zeros((hops, channels, 25), np.uint16)
        data = np.zeros(hops * (12 + channels * (50 + 4 + 2064)) + 16, np.uint8)
        sizes = np.zeros(max(hops, 1), np.uint32)
        n = C.c_size_t()
        self._chk(self._L.flo_lossy_pack_frames(self._h, c.ctypes.data, hops, sample_rate, channels, quality, q.ctypes.data,
                                                sfw.ctypes.data, data.ctypes.data, data.size, C.byref(n), sizes.ctypes.data))
        return dict(q=q, sf_words=sfw, data=data[:n.value].tobytes(), frame_sizes=sizes[:hops].astype(np.int64))

    def lossy_quantize_smr(self, coeffs, smr, sample_rate, quality):
        """TransformEncoder::quantize_coefficients on the device (encoder.rs:109-154): vectors of 1024 coefficients and the
        caller's signal-to-mask ratios -> (i16 [n][1024], f32 scale factors [n][25]); smr=None: scale factors only."""
        c = np.ascontiguousarray(coeffs, np.float32).reshape(-1, 1024)
        n = c.shape[0]
        sf = np.zeros((n, 25), np.float32)
        if smr is None:
            self._chk(self._L.flo_lossy_quantize_smr(self._h, c.ctypes.data, None, n, sample_rate, quality, None, sf.ctypes.data))
            return None, sf
        m = np.ascontiguousarray(smr, np.float32).reshape(-1, 1024)
        assert m.shape == c.shape
        q = np.zeros((n, 1024), np.int16)
        self._chk(self._L.flo_lossy_quantize_smr(self._h, c.ctypes.data, m.ctypes.data, n, sample_rate, quality, q.ctypes.data, sf.ctypes.data))
        return q, sf

    def sparse_pack(self, q, form=0):
        """serialize_sparse on the device. form 0: as the encoder packs (item form, behind it the block form, behind that the
        general form for dense vectors); form 1: the general form for every vector; form 2: block form, then general."""
        q = np.ascontiguousarray(q, np.int16).reshape(-1, 1024)
        n = q.shape[0]
        out = np.zeros(n * 2080, np.uint8)
        off = np.zeros(n + 1, np.uint32)
        self._chk(self._L.flo_sparse_pack(self._h, q.ctypes.data, n, form, out.ctypes.data, out.size, off.ctypes.data))
        return [out[off[i]:off[i + 1]].tobytes() for i in range(n)]

    # -- profiling hooks --------------------------------------------------------------------------------------
    def profile_enable(self, on=True):
        self._chk(self._L.flo_ctx_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        self._chk(self._L.flo_ctx_profile_reset(self._h))

    def profile_query(self, kernel: str):
        ms, n = C.c_double(), C.c_uint64()
        self._chk(self._L.flo_ctx_profile_query(self._h, kernel.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def stream(self):
        return self._L.flo_ctx_stream(self._h)


class Batch:
    """Device-resident batch of clips (flo_batch): PCM stays in HBM, bitstreams are left in HBM."""

    def __init__(self, ctx: Context, mode, n_interleaved, sample_rate, channels, quality_or_level, _handle=None):
        self.ctx, self._L = ctx, ctx._L
        self.channels = int(channels)
        self.sample_rate = int(sample_rate)
        self.n_clips = len(n_interleaved)
        self.n_interleaved = list(int(x) for x in n_interleaved)
        self._made = (mode, quality_or_level)
        h = C.c_void_p()
        if _handle is None:
            lens = (C.c_size_t * self.n_clips)(*self.n_interleaved)
            ctx._chk(self._L.flo_batch_create(ctx._h, mode, self.n_clips, lens, sample_rate, channels, quality_or_level, C.byref(h)))
        else:
            h = _handle   # (made by the library: Batch.resample)
        self._h = h
        ctx._batches.add(self)

    def resample(self, out_rate) -> "Batch":
        """flo_batch_resample: a new batch of the same mode, channels, quality / level and bit depth at out_rate, every clip
        converted on the device in one launch (enqueued; sync() of either batch orders it). Whole sample-frames are
        converted; this batch stays valid and unchanged"""
        h = C.c_void_p()
        self.ctx._chk(self._L.flo_batch_resample(self._h, out_rate, C.byref(h)))
        lens = [resample_out_frames(self.sample_rate, out_rate, n // self.channels) * self.channels for n in self.n_interleaved]
        return Batch(self.ctx, self._made[0], lens, out_rate, self.channels, self._made[1], _handle=h)

    def true_peaks(self, linear=False) -> np.ndarray:
        """flo_batch_true_peak: every clip's 4x oversampled peak (the 1 -> 4 interpolator of the sample-rate conversion, the
        samples themselves included), in one launch: dBTP as f64 (20 log10, -150 at or below 1e-9), or the f32 values"""
        lin = np.zeros(max(self.n_clips, 1), np.float32)
        self.ctx._chk(self._L.flo_batch_true_peak(self._h, lin.ctypes.data))
        lin = lin[:self.n_clips]
        return lin if linear else np.array([_dbtp(v) for v in lin], np.float64)

    def normalize(self, target_lufs=-14.0, ceiling_dbtp=-1.0, limit=False, lookahead_ms=1.5, max_gain_db=30.0):
        """flo_batch_normalize: (a new batch of the same mode, rate, channels, quality / level and bit depth, one report per
        clip). Every clip is brought to target_lufs by its own gain; without `limit` the gain is lowered where the clip's
        true peak would pass ceiling_dbtp, with it the full gain is applied and a limiter that looks lookahead_ms ahead
        holds the ceiling. Whole sample-frames are processed; this batch stays valid and unchanged"""
        opts = _normalize_opts(self.sample_rate, target_lufs, ceiling_dbtp, limit, lookahead_ms, max_gain_db)
        h = C.c_void_p()
        reps = (_native.NormalizeReport * max(self.n_clips, 1))()
        self.ctx._chk(self._L.flo_batch_normalize(self._h, C.byref(opts), C.byref(h), reps))
        lens = [n // self.channels * self.channels for n in self.n_interleaved]
        out = Batch(self.ctx, self._made[0], lens, self.sample_rate, self.channels, self._made[1], _handle=h)
        return out, [_normalize_report(reps[i]) for i in range(self.n_clips)]

    def edit(self, segments, channels=None, matrix=None) -> "Batch":
        """flo_batch_edit: a new batch of the same mode, rate, quality / level and bit depth whose clip k is segment k: a
        cut of one clip of this batch, padded, faded and mixed to `channels` by `matrix` ([channels][self.channels] f32; None:
        a copy), every clip in one launch (enqueued; sync() of either batch orders it). A segment is a dict with clip and
        optionally start (0), frames (to the clip's end), pad_head, pad_tail, fade_in, fade_out (0), all in frames, or a
        _native.EditSegment. This batch stays valid and unchanged"""
        frames = [n // self.channels for n in self.n_interleaved]
        segs = _edit_segments(segments, frames)
        cout, m = _edit_matrix(self.channels, channels, matrix)
        h = C.c_void_p()
        self.ctx._chk(self._L.flo_batch_edit(self._h, len(segs), segs, cout, m.ctypes.data if m is not None else None, C.byref(h)))
        lens = [(int(g.pad_head) + int(g.frames) + int(g.pad_tail)) * cout for g in segs]
        return Batch(self.ctx, self._made[0], lens, self.sample_rate, cout, self._made[1], _handle=h)

    def remix(self, matrix) -> "Batch":
        """every clip whole, mixed to len(matrix) channels by matrix [Cout][self.channels] (Batch.edit)"""
        return self.edit([dict(clip=i) for i in range(self.n_clips)], None, matrix)

    def to_mono(self) -> "Batch":
        """every clip whole as one channel: the matrix [[1 / channels] * channels] in f32 (Batch.remix)"""
        return self.remix(np.array([[1.0 / self.channels] * self.channels], np.float32))

    def active_ranges(self, threshold_db=-60.0) -> np.ndarray:
        """flo_batch_active_range: (n_clips, 2) uint64, per clip the first frame with a sample above the threshold in magnitude
        (or NaN) and the last such frame plus one; 0, 0 for a clip without one. The threshold is f32(10^(threshold_db / 20))"""
        r = np.zeros((2, max(self.n_clips, 1)), np.uint64)
        thr = np.float32(10.0 ** (float(threshold_db) / 20.0))
        self.ctx._chk(self._L.flo_batch_active_range(self._h, float(thr), r[0].ctypes.data, r[1].ctypes.data))
        return np.ascontiguousarray(r[:, :self.n_clips].T)

    def trim_silence(self, threshold_db=-60.0, pre_ms=0.0, post_ms=0.0, fade_ms=0.0):
        """(a new batch, the active ranges): every clip cut to its active range, widened by pre_ms in front and post_ms behind
        (inside the clip) and faded in and out over fade_ms (at most the cut). A clip without an active frame becomes a clip
        of 0 frames. Batch.active_ranges, then Batch.edit"""
        ranges = self.active_ranges(threshold_db)
        frames = [n // self.channels for n in self.n_interleaved]
        segs = trim_segments(ranges, frames, self.sample_rate, pre_ms, post_ms, fade_ms)
        return self.edit(segs), ranges

    def mix(self, parts, out_frames=None, others=()) -> "Batch":
        """flo_batch_mix: a new batch of this batch's mode, rate, channels, quality / level and bit depth whose clip k is the
        sum of the parts with out == k, in list order, every clip in one launch (enqueued; sync() of any of the batches
        orders it). The sources are (self, *others): batches of this context, rate and channel count. A part is a dict with
        out and clip and optionally batch (0: this batch), start (0), frames (to the clip's end), at (0), gain (1.0),
        fade_in, fade_out (0), all in frames, or a _native.MixPart; parts are listed with `out` non-decreasing. Source
        frames [start, start + frames) land on output frames [at, at + frames), times gain and the linear fades of
        Batch.edit; a part is cut at its source's end and at the output's end. A frame no part covers is +0.0.
        out_frames: the frames of every output clip; None: every output ends with its furthest part, and there are
        1 + max(out) of them. The sources stay valid and unchanged"""
        srcs = (self,) + tuple(others)
        arr = _mix_parts(parts, [[n // b.channels for n in b.n_interleaved] for b in srcs])
        if out_frames is None:
            out_frames = _mix_out_frames(arr)
        frames = [int(t) for t in out_frames]
        T = (C.c_uint64 * max(len(frames), 1))(*frames)
        hs = (C.c_void_p * len(srcs))(*[b._h.value for b in srcs])
        h = C.c_void_p()
        self.ctx._chk(self._L.flo_batch_mix(hs, len(srcs), len(frames), T, len(arr), arr, C.byref(h)))
        return Batch(self.ctx, self._made[0], [t * self.channels for t in frames], self.sample_rate, self.channels, self._made[1], _handle=h)

    def concat(self, groups, crossfade_ms=0.0) -> "Batch":
        """a new batch whose clip k plays the clips groups[k] (a list of clip indices of this batch) end to end, neighbours
        overlapping by crossfade_ms (concat_parts has the rule and what a linear crossfade sums to). Batch.mix"""
        frames = [n // self.channels for n in self.n_interleaved]
        parts, T = [], []
        for k, g in enumerate(groups):
            p, t = concat_parts(frames, self.sample_rate, crossfade_ms, out=k, clips=list(g))
            parts += p
            T.append(t)
        return self.mix(parts, T)

    def convolve(self, irs, jobs=None, *, ir=0, mode="head", taps=None, method="direct") -> "Batch":
        """flo_batch_convolve: a new batch of this batch's mode, rate, channels, quality / level and bit depth whose clip k is
        job k: a clip of this batch filtered by a clip of `irs` (a batch of this context and rate with 1 or self.channels
        channels; it may be this batch), every clip in one launch (enqueued; sync() of any of the three batches orders it).
        Output sample (t, c) is the FMA chain over taps k = 0 .. K - 1 of h[k, c] * x[t + skip - k, c], +0.0 outside the clip.
        A job is a dict with clip and optionally ir (0), frames (the source clip's frames), skip (0), ir_start (0), taps (to
        the response's end), or a _native.ConvJob. Without jobs every clip gets one job against response `ir` (an index, or a
        list with one index per clip), at most `taps` taps, in `mode`: "head": skip 0, frames N (causal, the tail is cut);
        "full": frames N + K - 1 (0 when either is empty); "centered": skip (K - 1) // 2, frames N (for linear-phase
        filters). Both batches stay valid and unchanged.
        method: "direct" (the default: that chain, to the bit); "fft": flo_batch_convolve_fft, the partitioned FFT path for
        long responses, which approximates the chain in f32 and takes up to FLO_CONV_FFT_MAX_TAPS taps; "auto": the FFT path
        when the largest K of the call is at least conv_fft_geometry()["crossover_taps"]. The FFT path is not merely
        enqueued: its scratch goes back to the pool before the call returns, so the call returns when its launches have run"""
        ir_frames = [n // irs.channels for n in irs.n_interleaved]
        arr = _conv_jobs(jobs, [n // self.channels for n in self.n_interleaved], ir_frames, ir, mode, taps)
        h = C.c_void_p()
        fn = self._L.flo_batch_convolve_fft if _conv_takes_fft(method, arr, ir_frames, self.channels, irs.channels) else self._L.flo_batch_convolve
        self.ctx._chk(fn(self._h, irs._h, len(arr), arr, C.byref(h)))
        return Batch(self.ctx, self._made[0], [int(g.frames) * self.channels for g in arr], self.sample_rate, self.channels, self._made[1], _handle=h)

    def filter(self, kind, f_lo=None, f_hi=None, taps=255, beta=9.0) -> "Batch":
        """every clip through the linear-phase FIR fir_design(kind, self.sample_rate, f_lo, f_hi, taps, beta), delay taken
        off: the table as a one-clip mono batch of this context, then convolve(..., mode="centered")"""
        table = fir_design(kind, self.sample_rate, f_lo, f_hi, taps, beta)
        irs = Batch(self.ctx, MODE_LOSSLESS, [table.size], self.sample_rate, 1, 0)
        try:
            irs.upload(0, table)
            return self.convolve(irs, mode="centered")
        finally:
            irs.close()   # (waits for the stream: the launch has read the response before it goes)

    def close(self):
        if getattr(self, "_h", None):
            self._L.flo_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clip_device_ptr(self, clip):
        return self._L.flo_batch_clip_device_ptr(self._h, clip)

    def upload(self, clip, samples):
        p = _f32(samples)
        assert p.size == self.n_interleaved[clip]
        self.ctx._chk(self._L.flo_batch_upload(self._h, clip, p.ctypes.data))
        self.ctx._chk(self._L.flo_batch_sync(self._h))   # p may be released by the caller

    def fill_synthetic(self, seed=0xF10A0D10, clip_id0=0):
        self.ctx._chk(self._L.flo_batch_fill_synthetic(self._h, seed, clip_id0))

    def download_pcm(self, clip):
        """the clip's interleaved f32 PCM as it sits in the batch (after upload or fill_synthetic), as a numpy array"""
        import numpy as np
        self.sync()
        n = int(self.n_interleaved[clip])
        out = np.empty(n, np.float32)
        if n:
            hip = C.CDLL("libamdhip64.so")
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            rc = hip.hipMemcpy(out.ctypes.data, self._L.flo_batch_clip_device_data(self._h, clip), n * 4, 2)
            if rc != 0:
                raise FloError(f"hipMemcpy (device to host) failed with {rc}")
        return out

    def encode(self, which=0):
        self.ctx._chk(self._L.flo_batch_encode(self._h, which))

    def sync(self):
        self.ctx._chk(self._L.flo_batch_sync(self._h))

    def data_bytes(self):
        t = C.c_uint64()
        self.ctx._chk(self._L.flo_batch_data_bytes(self._h, C.byref(t)))
        return t.value

    def analysis_metadata(self, clip, peaks_per_second=50) -> bytes:
        """the analysis META of a clip already uploaded into this batch (no second trip over PCIe)"""
        out, n = C.c_void_p(), C.c_size_t()
        self.ctx._chk(self._L.flo_batch_analysis_metadata(self._h, clip, peaks_per_second, C.byref(out), C.byref(n)))
        return self.ctx._take(out, n)

    def analyze_all(self, peaks_per_second=50):
        """the analysis of every clip (one device pass over the whole batch): a list of dicts shaped like Context.analyze"""
        off = (C.c_uint64 * (self.n_clips + 1))()
        self.ctx._chk(self._L.flo_batch_analyze_all(self._h, peaks_per_second, None, None, 0, off))
        peaks = np.zeros(max(off[self.n_clips], 1), np.float32)
        an = (_native.Analysis * max(self.n_clips, 1))()
        self.ctx._chk(self._L.flo_batch_analyze_all(self._h, peaks_per_second, an, peaks.ctypes.data, peaks.size, off))
        return [_analysis_dict(an[i], peaks[off[i]:off[i + 1]].copy()) for i in range(self.n_clips)]

    def analysis_metadata_all(self, peaks_per_second=50):
        """the analysis META of every clip (one device pass over the whole batch), as a list of bytes"""
        out, off = C.c_void_p(), (C.c_uint64 * (self.n_clips + 1))()
        self.ctx._chk(self._L.flo_batch_analysis_metadata_all(self._h, peaks_per_second, C.byref(out), off))
        blob = self.ctx._take(out, C.c_size_t(off[self.n_clips]))
        return [blob[off[i]:off[i + 1]] for i in range(self.n_clips)]

    def set_bit_depth(self, bit_depth: int):
        self.ctx._chk(self._L.flo_batch_set_bit_depth(self._h, bit_depth))

    def size_curve(self, qualities) -> np.ndarray:
        """flo_batch_size_curve: [n_clips, K] uint64, the exact length of the file (empty META) an encode of this lossy batch
        at qualities[j] produces, from one device pass over the PCM the batch holds; the batch's results are untouched"""
        q = np.ascontiguousarray(qualities, dtype=np.float32).reshape(-1)
        out = np.zeros((self.n_clips, q.size), np.uint64)
        self.ctx._chk(self._L.flo_batch_size_curve(self._h, q.size, q.ctypes.data, out.ctypes.data))
        return out

    def set_quality(self, quality: float):
        """re-point a lossy batch at another quality; results of an earlier encode are dropped"""
        self.ctx._chk(self._L.flo_batch_set_quality(self._h, quality))

    def encode_ladder(self, qualities) -> "Ladder":
        """flo_batch_encode_ladder: every clip of this lossy batch as a finished file at each of the K qualities, from one
        transform pass over the PCM the batch holds (rung j of clip i is encode_lossy's file at qualities[j]); complete on
        return. The batch's own quality plays no part and its results are untouched; the Ladder may outlive the batch"""
        q = np.ascontiguousarray(qualities, dtype=np.float32).reshape(-1)
        h = C.c_void_p()
        self.ctx._chk(self._L.flo_batch_encode_ladder(self._h, q.size, q.ctypes.data, C.byref(h)))
        return Ladder(self.ctx, h, [float(x) for x in q])

    def fetch(self, clip, metadata=b"") -> bytes:
        out, n = C.c_void_p(), C.c_size_t()
        self.ctx._chk(self._L.flo_batch_fetch(self._h, clip, metadata, len(metadata), C.byref(out), C.byref(n)))
        return self.ctx._take(out, n)

    def pack_streams(self, dst_ptr: int, dst_cap: int):
        """Pack all DATA chunks into caller-owned device memory; returns the n_clips + 1 offsets."""
        offs = (C.c_uint64 * (self.n_clips + 1))()
        self.ctx._chk(self._L.flo_batch_pack_streams(self._h, dst_ptr, dst_cap, offs))
        return list(offs)

    def pack_files(self, dst_ptr: int, dst_cap: int):
        """Pack all finished .flo files (empty META) into caller-owned device memory; returns the n_clips + 1 offsets."""
        offs = (C.c_uint64 * (self.n_clips + 1))()
        self.ctx._chk(self._L.flo_batch_pack_files(self._h, dst_ptr, dst_cap, offs))
        return list(offs)

    def decode_to(self, dst_ptr: int, dst_cap_floats: int):
        """Decode every clip of an encoded lossy batch into device memory; returns the per-clip float offsets."""
        offs = (C.c_uint64 * max(self.n_clips, 1))()
        self.ctx._chk(self._L.flo_batch_decode(self._h, dst_ptr, dst_cap_floats, offs))
        return list(offs[: self.n_clips])

    def fidelity(self, blocks=False):
        """How far each clip's decoded audio lies from its source (flo_batch_fidelity, include/flo_hip.h), measured on the
        device after encode + sync: one dict per clip (see fidelity_dict); blocks=True adds the block records."""
        ch = self.channels
        off = np.zeros(self.n_clips + 1, np.uint64)
        self.ctx._chk(self._L.flo_batch_fidelity(self._h, None, None, 0, off.ctypes.data))
        out = np.zeros(max(self.n_clips * ch, 1), FIDELITY_DTYPE)
        nrec = int(off[-1]) * ch
        blk = np.zeros(max(nrec, 1), FIDELITY_BLOCK_DTYPE) if blocks else None
        self.ctx._chk(self._L.flo_batch_fidelity(self._h, out.ctypes.data, blk.ctypes.data if blocks else None,
                                                 nrec if blocks else 0, off.ctypes.data))
        return [fidelity_dict(out[i * ch:(i + 1) * ch],
                              blk[int(off[i]) * ch:int(off[i + 1]) * ch].reshape(-1, ch) if blocks else None)
                for i in range(self.n_clips)]

    def device_streams(self):
        base = C.c_void_p()
        offs, sizes = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        self.ctx._chk(self._L.flo_batch_device_streams(self._h, C.byref(base), C.byref(offs), C.byref(sizes)))
        return base.value, [offs[i] for i in range(self.n_clips)], [sizes[i] for i in range(self.n_clips)]


class Ladder:
    """flo_ladder: the files of a quality ladder (Batch.encode_ladder), resident on the device. Closed before its context."""

    def __init__(self, ctx: Context, handle, qualities):
        self.ctx, self._L, self._h = ctx, ctx._L, handle
        self.qualities = list(qualities)
        nc, nq = C.c_size_t(), C.c_size_t()
        ctx._chk(self._L.flo_ladder_shape(handle, C.byref(nc), C.byref(nq)))
        self.n_clips, self.n_rungs = nc.value, nq.value
        self.file_bytes = np.zeros((self.n_clips, self.n_rungs), np.uint64)   # without META
        ctx._chk(self._L.flo_ladder_file_bytes(handle, self.file_bytes.ctypes.data))
        ctx._batches.add(self)

    def fetch(self, clip, rung, metadata=b"") -> bytes:
        out, n = C.c_void_p(), C.c_size_t()
        self.ctx._chk(self._L.flo_ladder_fetch(self._h, clip, rung, metadata, len(metadata), C.byref(out), C.byref(n)))
        return self.ctx._take(out, n)

    def device_files(self, rung):
        """(base, offsets, sizes) of one rung's files as they sit in device memory (no META); offsets are multiples of 16"""
        base = C.c_void_p()
        offs, sizes = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        self.ctx._chk(self._L.flo_ladder_device_files(self._h, rung, C.byref(base), C.byref(offs), C.byref(sizes)))
        return base.value, [offs[i] for i in range(self.n_clips)], [sizes[i] for i in range(self.n_clips)]

    def close(self):
        if getattr(self, "_h", None):
            self._L.flo_ladder_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def debug_pool_fill(byte):
    """Test hook (flo_debug_pool_fill): fill every pool block and pinned download buffer with `byte` (0 .. 255) as it is handed
    out; None turns the fill off. Process-wide. Returns the previous setting (None: off)."""
    if byte is not None and not 0 <= int(byte) <= 255:
        raise ValueError("byte must be None or 0 .. 255")
    prev = _native.lib().flo_debug_pool_fill(-1 if byte is None else int(byte))
    return None if prev < 0 else prev


def debug_stream_delay(us):
    """Test hook (flo_debug_stream_delay): queue a delay of about `us` microseconds (0 .. 5000) in front of every launch of
    the library's and behind every wait for an event on its own streams; None turns it off. Process-wide. Returns the
    previous setting (None: off)."""
    if us is not None and not 0 <= int(us) <= 5000:
        raise ValueError("us must be None or 0 .. 5000")
    prev = _native.lib().flo_debug_stream_delay(-1 if us is None else int(us))
    return None if prev < 0 else prev


def debug_stream_delays():
    """The number of delays queued so far in this process (flo_debug_stream_delays)."""
    return int(_native.lib().flo_debug_stream_delays())


def debug_delay_enqueue(stream, us):
    """Queue one delay of about `us` microseconds (0 .. 5000) on `stream` (a hipStream_t as an integer, or an object with
    .cuda_stream such as a torch stream), whatever the switch says (flo_debug_delay_enqueue)."""
    if not 0 <= int(us) <= 5000:
        raise ValueError("us must be 0 .. 5000")
    handle = getattr(stream, "cuda_stream", stream)
    rc = _native.lib().flo_debug_delay_enqueue(int(handle) if handle else None, int(us))
    if rc != 0:
        raise RuntimeError("flo_debug_delay_enqueue failed (%d)" % rc)


_default = threading.local()   # .ctx: the calling thread's default context


def default_context() -> Context:
    """The calling thread's own context on device 0, made on the thread's first call. The free functions (encode, decode,
    resample, normalize, ...) and every object built without ctx= use it, so each of them works on the context of the thread
    that called or built it: the header's rule, one flo_ctx per host thread, holds without the caller doing anything. The
    same object is returned for as long as the thread lives. Nothing but the thread (and the objects the caller built on it)
    refers to it, so it is destroyed when the thread has finished and those objects are gone."""
    ctx = getattr(_default, "ctx", None)
    if ctx is None:
        ctx = _default.ctx = Context(0)
    return ctx


class Encoder:
    """lossless::Encoder — lossless/encoder.rs:9-45"""

    def __init__(self, sample_rate: int, channels: int, bit_depth: int, ctx: Context = None):
        self.sample_rate, self.channels, self.bit_depth = sample_rate, channels, bit_depth
        self.compression_level = 5
        self._ctx = ctx

    def with_compression(self, level: int) -> "Encoder":
        self.compression_level = min(int(level), 9)
        return self

    def encode(self, samples, metadata: bytes = b"") -> bytes:
        ctx = self._ctx or default_context()
        return ctx.encode_lossless(samples, self.sample_rate, self.channels, self.bit_depth, self.compression_level, metadata)


class Decoder:
    """lossless::Decoder (lossless/decoder.rs:6-18); like libflo::decode it also accepts transform files."""

    def __init__(self, ctx: Context = None):
        self._ctx = ctx or default_context()

    def decode(self, data: bytes):
        return self._ctx.decode(data)


class TransformFrame:
    """lossy::TransformFrame (lossy/mod.rs): what encode_frame returns - per channel the 1024 quantised coefficients and the
    25 band scale factors; `scale_words` are the u16 words the container stores for them (encoder.rs:262-266)."""

    def __init__(self, coefficients, scale_factors, scale_words):
        self.coefficients, self.scale_factors, self.scale_words = coefficients, scale_factors, scale_words
        self.block_size, self.num_samples = 2048, 1024


class TransformEncoder:
    """lossy::TransformEncoder — lossy/encoder.rs:6-53,63-164,167-239. One fresh encoder per clip is the contract."""

    _HISTORY = 65   # frames whose masking levels can still reach the newest one: the temporal step is max(a_t, 0.7 s_{t-1}),
                    # and the frame-parallel kernels resolve it exactly from a 64-frame warm-up (tests compare them to the chain);
                    # a level of +inf is the exception, kept by _pin

    def __init__(self, sample_rate: int, channels: int, quality: float, ctx: Context = None):
        self.sample_rate, self.channels = sample_rate, channels
        self.quality = float(min(max(quality, 0.0), 1.0))
        self._ctx = ctx
        self._spectra = []   # the last _HISTORY frames' coefficients [ch][1024]: the psychoacoustic model's temporal state
        self._pinned = []    # in front of them: the spectra whose level may never decay (see _pin)
        self._pinned_n = {}

    def set_quality(self, quality: float):
        self.quality = float(min(max(quality, 0.0), 1.0))

    def reset(self):
        """encoder.rs:157-164: forget the temporal masking state (and the transform's, which keeps none here)"""
        self._spectra = []
        self._pinned = []
        self._pinned_n = {}

    _PIN_CAP = 32   # pinned spectra per channel

    def _pin(self, old):
        """A spectrum that leaves the history takes its masking levels with it, which is right for every finite level (0.7^65
        of it is nothing) and wrong for +inf, the level of a band whose f32 energy overflowed: the reference keeps that one
        for good. Such a spectrum therefore stays in front of the history, the other channels zeroed. Whether a band's f32
        sum overflows depends on the kernel's summation order, so the test here is deliberately wide: every channel whose sum
        of squares (f64) is not below a quarter of the f32 maximum - NaN included - is kept, and keeping one whose level was
        finite after all changes nothing (in front of 65 frames it has decayed). Each kept spectrum is judged by the device
        again in every pass, so no decision is taken here. Up to _PIN_CAP per channel, the earliest: not covered is a clip
        with more than that many such frames of which none of the first _PIN_CAP overflowed on the device."""
        for c in range(self.channels):
            if self._pinned_n.get(c, 0) >= self._PIN_CAP:
                continue
            with np.errstate(all="ignore"):
                e = float((old[c].astype(np.float64) ** 2).sum())
            if not e < 0.25 * float(np.finfo(np.float32).max):
                keep = np.zeros_like(old)
                keep[c] = old[c]
                self._pinned.append(keep)
                self._pinned_n[c] = self._pinned_n.get(c, 0) + 1

    def encode_frame(self, samples) -> TransformFrame:
        """encoder.rs:63-106: one block of 2048 sample-frames (interleaved; shorter blocks are zero-padded) -> its quantised
        spectrum. Stateful like the reference: the masking thresholds of a frame depend on the frames encoded before it
        (psychoacoustic.rs:196-203), so the device pass runs over the kept spectra and the newest frame's result is returned."""
        ctx = self._ctx or default_context()
        x = _f32(samples)
        ch = self.channels
        per = x.size // ch + (1 if x.size % ch else 0)
        block = np.zeros((ch, 2048), np.float32)
        for c in range(ch):
            d = x[c::ch][:2048]
            block[c, :d.size] = d
        assert per <= 2048, "encode_frame takes one block (2048 sample-frames)"
        spec = ctx.mdct_forward(block.reshape(-1))            # [ch][1024], device
        self._spectra.append(spec)
        if len(self._spectra) > self._HISTORY:
            self._pin(self._spectra.pop(0))
        g = ctx.lossy_quantize(np.stack(self._pinned + self._spectra), self.sample_rate, self.quality)
        _, sf = ctx.lossy_quantize_smr(spec, None, self.sample_rate, self.quality)
        return TransformFrame([g["q"][-1, c].copy() for c in range(ch)], [sf[c].copy() for c in range(ch)],
                              [g["sf_words"][-1, c].copy() for c in range(ch)])

    def quantize_coefficients(self, coeffs, smr):
        """encoder.rs:109-154: (quantised i16 [1024], scale factors f32 [25]) of one channel's coefficients under the
        caller's signal-to-mask ratios, on the device"""
        ctx = self._ctx or default_context()
        q, sf = ctx.lossy_quantize_smr(coeffs, smr, self.sample_rate, self.quality)
        return q[0], sf[0]

    def encode_to_flo(self, samples, metadata: bytes = b"") -> bytes:
        ctx = self._ctx or default_context()
        return ctx.encode_lossy(samples, self.sample_rate, self.channels, self.quality, metadata)


LossyEncoder = TransformEncoder


class EncodedFrame:
    """streaming/encoder.rs:18-29"""

    def __init__(self, index, timestamp_ms, data, samples):
        self.index, self.timestamp_ms, self.data, self.samples = index, timestamp_ms, data, samples

    def __repr__(self):
        return f"EncodedFrame(index={self.index}, timestamp_ms={self.timestamp_ms}, samples={self.samples}, {len(self.data)} bytes)"


class StreamingEncoder:
    """streaming::StreamingEncoder - libflo/src/streaming/encoder.rs:6-257, over flo_stream_* of the C ABI."""

    def __init__(self, sample_rate: int, channels: int, bit_depth: int, ctx: Context = None):
        self.sample_rate, self.channels, self.bit_depth = sample_rate, channels, bit_depth
        self.compression_level = 5
        self._ctx = ctx or default_context()
        self._L = self._ctx._L
        self._h = None
        self._open()

    def _open(self):
        if self._h:
            self._L.flo_stream_destroy(self._h)
        h = C.c_void_p()
        self._ctx._chk(self._L.flo_stream_create(self._ctx._h, self.sample_rate, self.channels, self.bit_depth, self.compression_level, C.byref(h)))
        self._h = h

    def with_compression(self, level: int) -> "StreamingEncoder":
        self.compression_level = min(int(level), 9)
        self._open()      # like the reference, meant to be called right after construction
        return self

    def pending_samples(self) -> int:
        return self._L.flo_stream_pending_samples(self._h)

    def pending_frames(self) -> int:
        return self._L.flo_stream_pending_frames(self._h)

    def push_samples(self, samples):
        p = _f32(samples)
        self._ctx._chk(self._L.flo_stream_push(self._h, p.ctypes.data, p.size))

    def append_samples(self, samples):
        """buffer samples without encoding anything: encode_streams encodes what is complete"""
        p = _f32(samples)
        self._ctx._chk(self._L.flo_stream_append(self._h, p.ctypes.data, p.size))

    def _pull(self, fn):
        idx, ts, ns = C.c_uint32(), C.c_uint32(), C.c_uint32()
        data, n = C.c_void_p(), C.c_size_t()
        r = fn(self._h, C.byref(idx), C.byref(ts), C.byref(ns), C.byref(data), C.byref(n))
        if r < 0:
            raise FloError(self._L.flo_last_error(self._ctx._h).decode())
        if r == 0:
            return None
        return EncodedFrame(idx.value, ts.value, self._ctx._take(data, n), ns.value)

    def next_frame(self):
        return self._pull(self._L.flo_stream_next_frame)

    def flush(self):
        return self._pull(self._L.flo_stream_flush)

    def finalize(self, metadata: bytes = b"") -> bytes:
        out, n = C.c_void_p(), C.c_size_t()
        self._ctx._chk(self._L.flo_stream_finalize(self._h, metadata, len(metadata), C.byref(out), C.byref(n)))
        return self._ctx._take(out, n)

    def close(self):
        if getattr(self, "_h", None):
            self._L.flo_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LossyStreamingEncoder(StreamingEncoder):
    """The lossy encoder (TransformEncoder::encode_to_flo, lossy/encoder.rs:167-239) frame by frame, over
    flo_stream_create_lossy: frame h comes out once (h + 1) * 1024 sample-frames have been pushed, byte for byte the
    offline file's frame h; finalize() after pulling nothing is encode_lossy's file. flush() ends the input (the trailing
    frames join the queue) and returns the queue's front."""

    def __init__(self, sample_rate: int, channels: int, quality, ctx: Context = None):
        if isinstance(quality, QualityPreset):
            quality = quality.as_f32()
        self.sample_rate, self.channels, self.quality = sample_rate, channels, float(quality)
        self._ctx = ctx or default_context()
        self._L = self._ctx._L
        self._h = None
        h = C.c_void_p()
        self._ctx._chk(self._L.flo_stream_create_lossy(self._ctx._h, self.sample_rate, self.channels, self.quality, C.byref(h)))
        self._h = h

    def with_compression(self, level: int):
        raise FloError("a lossy stream has no compression level")


class EncodeStreamsResult(NamedTuple):
    status: np.ndarray   # [n] int32: 0, or the stream's FLO_ERR_* code
    errors: list         # [n] messages ("" where status is 0)


def encode_streams(encoders, ctx: Context = None) -> EncodeStreamsResult:
    """flo_stream_encode_ready: every complete frame of every encoder (LossyStreamingEncoder or StreamingEncoder) is
    encoded and queued - per (sample rate, channels, quality) of the lossy ones one upload, one set of launches and one
    read-back, the call synchronising once. The frames land in each encoder's queue (next_frame / finalize)."""
    encoders = list(encoders)
    if any(getattr(e, "_h", None) is None for e in encoders):
        raise FloError("encode_streams: an encoder is closed")
    if ctx is None:
        ctx = encoders[0]._ctx if encoders else default_context()
    n = len(encoders)
    hs = (C.c_void_p * max(n, 1))(*[e._h.value for e in encoders])
    st = np.zeros(max(n, 1), np.int32)
    rc = ctx._L.flo_stream_encode_ready(ctx._h, n, C.cast(hs, C.c_void_p), st.ctypes.data)
    st = st[:n].copy()
    if rc != 0 and not st.any():   # the call itself was refused (a null or repeated encoder)
        raise FloError(ctx._L.flo_last_error(ctx._h).decode())
    msg = ctx._L.flo_last_error(ctx._h).decode() if st.any() else ""
    errors = [("belongs to another context" if encoders[i]._ctx is not ctx else msg) if st[i] else "" for i in range(n)]
    return EncodeStreamsResult(st, errors)


def probe_container(data: bytes):
    """Header and frame census of a .flo file as the container reader sees it (reader.rs:16-256); no device needed.
    Raises FloError with the reader's message for files the reference reader rejects."""
    L = _native.lib()
    info = _native.ContainerInfo()
    err = C.create_string_buffer(256)
    data = bytes(data)
    if L.flo_probe_container(data, len(data), C.byref(info), err, len(err)) != 0:
        raise FloError(err.value.decode() or "not a .flo file")
    return info


def decode(data: bytes):
    """libflo::decode (lib.rs:296-315)"""
    return default_context().decode(data)


# -- seeking (libflo/src/seeking.rs) -------------------------------------------------------------------------------
class TocEntry(NamedTuple):
    """core/types.rs:174-179"""
    frame_index: int
    byte_offset: int
    frame_size: int
    timestamp_ms: int


class SeekResult(NamedTuple):
    """seeking.rs:7-19"""
    frame_index: int
    byte_offset: int
    timestamp_ms: int
    sample_offset: int
    next_timestamp_ms: int


def get_toc(data: bytes):
    """seeking::get_toc (seeking.rs:28-32): the TOC as the reader returns it; no device needed"""
    L = _native.lib()
    data = bytes(data)
    p, n = C.POINTER(_native.TocEntryC)(), C.c_size_t()
    err = C.create_string_buffer(256)
    if L.flo_get_toc(data, len(data), C.byref(p), C.byref(n), err, len(err)) != 0:
        raise FloError(err.value.decode() or "not a .flo file")
    res = [TocEntry(p[i].frame_index, p[i].byte_offset, p[i].frame_size, p[i].timestamp_ms) for i in range(n.value)]
    L.flo_free(C.cast(p, C.c_void_p))
    return res


def seek_to_time(data: bytes, target_ms: int):
    """seeking::seek_to_time (seeking.rs:75-132); no device needed"""
    L = _native.lib()
    data = bytes(data)
    r = _native.SeekResultC()
    err = C.create_string_buffer(256)
    if L.flo_seek_to_time(data, len(data), int(target_ms), C.byref(r), err, len(err)) != 0:
        raise FloError(err.value.decode() or "not a .flo file")
    return SeekResult(r.frame_index, r.byte_offset, r.timestamp_ms, r.sample_offset, r.next_timestamp_ms)


def decode_frame_at(data: bytes, frame_index: int):
    """seeking::decode_frame_at (seeking.rs:43-63)"""
    return default_context().decode_frame_at(data, frame_index)


# -- fidelity reports (flo_batch_fidelity, flo_compare; definitions in include/flo_hip.h) ---------------------------------
FIDELITY_DTYPE = np.dtype([("signal", "<f8"), ("error", "<f8"), ("tail_energy", "<f8"), ("snr_db", "<f8"), ("seg_snr_db", "<f8"),
                           ("peak_error", "<f4"), ("peak_out", "<f4"), ("clipped", "<u8"), ("compared_frames", "<u8"),
                           ("source_frames", "<u8"), ("decoded_frames", "<u8"), ("n_blocks", "<u4"), ("seg_blocks", "<u4")])
FIDELITY_BLOCK_DTYPE = np.dtype([("signal", "<f8"), ("error", "<f8"), ("peak_error", "<f4"), ("peak_out", "<f4"),
                                 ("clipped", "<u4"), ("n", "<u4")])
assert FIDELITY_DTYPE.itemsize == C.sizeof(_native.Fidelity)
assert FIDELITY_BLOCK_DTYPE.itemsize == C.sizeof(_native.FidelityBlock)


def snr_db(signal: float, error: float) -> float:
    """10 log10(signal / error): +inf when error = 0, -inf when signal = 0 < error"""
    if error == 0.0:
        return float("inf")
    if signal == 0.0:
        return float("-inf")
    return 10.0 * float(np.log10(signal / error))


def fidelity_dict(rec, blocks=None) -> dict:
    """One clip's report from its FIDELITY_DTYPE records [channels]: per-channel arrays signal, error, tail_energy, snr_db,
    seg_snr_db, peak_error, peak_out, clipped, seg_blocks; the counts compared_frames, source_frames, decoded_frames,
    n_blocks; snr_db_all over all channels (the channels' sums added in channel order); `blocks`: the FIDELITY_BLOCK_DTYPE
    records [n_blocks, channels] when asked for."""
    d = {k: rec[k].copy() for k in ("signal", "error", "tail_energy", "snr_db", "seg_snr_db", "peak_error", "peak_out",
                                      "clipped", "seg_blocks")}
    for k in ("compared_frames", "source_frames", "decoded_frames", "n_blocks"):
        d[k] = int(rec[k][0]) if rec.size else 0
    s = e = 0.0
    for c in range(rec.size):   # (sequential: Python's sum() of floats is compensated)
        s += float(rec["signal"][c])
        e += float(rec["error"][c])
    d["snr_db_all"] = snr_db(s, e)
    if blocks is not None:
        d["blocks"] = np.ascontiguousarray(blocks)
    return d


def compare(samples, flo: bytes, blocks=False) -> dict:
    """Context.compare on the default context: how far a .flo file's decoded audio lies from its source"""
    return default_context().compare(samples, flo, blocks)


class Corpus:
    """Many .flo files resident in HBM (flo_corpus); short windows of their decoded signals decoded in batches.

    decode_windows(file_idx, starts, length) returns a float32 tensor [n, length, channels] on the context's device that
    equals torch.from_numpy(decode(files[f]).reshape(-1, channels))[start:start + length] bit for bit, zero-padded past the
    end of the file. The decode is enqueued behind torch's current stream and the result is ordered before whatever is
    queued on that stream afterwards: no explicit synchronisation is needed."""

    def __init__(self, files, ctx=None):
        self._ctx = ctx or default_context()
        self._L = self._ctx._L
        blobs = [bytes(f) for f in files]
        arr = (C.c_char_p * len(blobs))(*blobs)
        lens = (C.c_size_t * len(blobs))(*[len(b) for b in blobs])
        h = C.c_void_p()
        self._ctx._chk(self._L.flo_corpus_create(self._ctx._h, len(blobs), arr, lens, C.byref(h)))
        self._h = h
        self._ctx._batches.add(self)   # closed before its context
        sr, ch = C.c_uint32(), C.c_uint8()
        self._L.flo_corpus_format(h, C.byref(sr), C.byref(ch))
        self.sample_rate, self.channels = sr.value, ch.value
        n = C.c_uint64()
        lengths = []
        for i in range(len(blobs)):
            self._L.flo_corpus_file_frames(h, i, C.byref(n))
            lengths.append(n.value)
        self.lengths = np.array(lengths, np.uint64)

    def decode_windows(self, file_idx, starts, length: int, out=None):
        import torch
        fi = np.ascontiguousarray(np.asarray(file_idx).reshape(-1), dtype=np.uint32)
        st = np.ascontiguousarray(np.asarray(starts).reshape(-1), dtype=np.uint64)
        if fi.size != st.size:
            raise FloError("file_idx and starts differ in length")
        if fi.size and int(fi.max()) >= len(self.lengths):
            raise FloError("window file index out of range")
        dev = torch.device("cuda", self._device_index())
        shape = (fi.size, int(length), self.channels)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=dev)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
            raise FloError(f"out must be a contiguous float32 tensor of shape {shape} on {dev}")
        stream = torch.cuda.current_stream(dev).cuda_stream
        self._ctx._chk(self._L.flo_corpus_decode_windows(self._h, fi.size, fi.ctypes.data, st.ctypes.data, int(length),
                                                         out.data_ptr(), out.numel(), C.c_void_p(stream)))
        return out

    def _device_index(self):
        return self._ctx.device

    def sync(self):
        self._ctx._chk(self._L.flo_corpus_sync(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._L.flo_corpus_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# -- streaming decoder (libflo/src/streaming/decoder.rs, types.rs) ---------------------------------------------------
class DecoderState(enum.IntEnum):
    """streaming/types.rs DecoderState"""
    WaitingForHeader = 0
    WaitingForToc = 1
    Ready = 2
    Finished = 3
    Error = 4


class StreamingAudioInfo(NamedTuple):
    """streaming/types.rs StreamingAudioInfo"""
    sample_rate: int
    channels: int
    bit_depth: int
    total_samples: int
    is_lossy: bool

    def duration_secs(self) -> float:
        return self.total_samples / self.sample_rate if self.sample_rate else float("inf") if self.total_samples else float("nan")

    def total_samples_per_channel(self) -> int:
        return self.total_samples


class StreamingDecoder:
    """StreamingDecoder (streaming/decoder.rs) on flo_sdec: feed bytes as they arrive, take each frame once it is complete.
    With ctx=None the default context is taken at the first decode only: feeding and the counters need no device."""

    def __init__(self, ctx: Context = None):
        self._L = _native.lib()
        self._ctx = ctx
        h = C.c_void_p()
        if self._L.flo_sdec_create(ctx._h if ctx else None, C.byref(h)) != 0:
            raise FloError("flo_sdec_create failed")
        self._h = h
        if ctx:
            ctx._batches.add(self)   # its device state goes before its context

    def _err(self):
        return self._L.flo_sdec_last_error(self._h).decode()

    def _attach(self) -> Context:
        if self._ctx is None:
            self._ctx = default_context()
            if self._L.flo_sdec_attach(self._h, self._ctx._h) != 0:
                raise FloError("the decoder belongs to another context")
            self._ctx._batches.add(self)
        return self._ctx

    def feed(self, data) -> bool:
        """feed (:70-78): True if new frames are available; FloError on bad magic (the state is then Error)"""
        data = bytes(data)
        nf = C.c_int()
        if self._L.flo_sdec_feed(self._h, data, len(data), C.byref(nf)) != 0:
            raise FloError(self._err())
        return bool(nf.value)

    def state(self) -> DecoderState:
        return DecoderState(self._L.flo_sdec_state(self._h))

    def info(self):
        """StreamingAudioInfo once the header is parsed, else None"""
        i = _native.SdecInfoC()
        if self._L.flo_sdec_info(self._h, C.byref(i)) != 0:
            return None
        return StreamingAudioInfo(i.sample_rate, i.channels, i.bit_depth, i.total_samples, bool(i.is_lossy))

    def frames_available(self) -> int:
        return int(self._L.flo_sdec_frames_available(self._h))

    def available_frames(self) -> int:
        return int(self._L.flo_sdec_available_frames(self._h))

    def current_frame_index(self) -> int:
        return int(self._L.flo_sdec_current_frame_index(self._h))

    def buffered_bytes(self) -> int:
        return int(self._L.flo_sdec_buffered_bytes(self._h))

    def next_frame(self):
        """next_frame (:81-112): one frame's interleaved f32 samples (possibly empty), or None when no frame is ready"""
        if self.state() != DecoderState.Ready:
            return None
        self._attach()
        p, n = C.c_void_p(), C.c_size_t()
        rc = self._L.flo_sdec_next_frame(self._h, C.byref(p), C.byref(n))
        if rc < 0:
            raise FloError(self._err())
        if rc == 0:
            return None
        if not n.value:
            return np.zeros(0, np.float32)
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n.value,)).copy()
        self._L.flo_free(p)
        return arr

    def decode_available(self):
        """decode_available (:114-122): the whole buffer decoded from frame 0; the state becomes Finished"""
        if self.state() != DecoderState.Ready:
            return np.zeros(0, np.float32)
        self._attach()
        p, n = C.c_void_p(), C.c_size_t()
        if self._L.flo_sdec_decode_available(self._h, C.byref(p), C.byref(n)) != 0:
            raise FloError(self._err())
        if not n.value:
            if p.value:
                self._L.flo_free(p)
            return np.zeros(0, np.float32)
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n.value,)).copy()
        self._L.flo_free(p)
        return arr

    def reset(self):
        self._L.flo_sdec_reset(self._h)

    def close(self):
        if getattr(self, "_h", None):
            self._L.flo_sdec_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StreamsResult(NamedTuple):
    out: object          # float32 torch tensor on the context's device
    offsets: np.ndarray  # [n + 1] uint64: decoder i's samples are out[offsets[i]:offsets[i + 1]]
    status: np.ndarray   # [n] int32: 0, or the FLO_ERR_* code decoder i's next next_frame reports
    errors: list         # [n] that error's message ("" for status 0)


def decode_streams(decoders, max_frames: int = 0, out=None, ctx: Context = None) -> StreamsResult:
    """flo_sdec_decode_ready: every complete frame not yet returned of every decoder (at most max_frames each, 0: all),
    decoded in one set of launches. Decoder i's part equals the concatenation of as many next_frame() results, and its
    counters advance to match. The decode is enqueued behind torch's current stream and ordered before what is queued on
    it afterwards. `out`: an optional contiguous float32 tensor on the device, large enough."""
    import torch
    decoders = list(decoders)
    if any(getattr(d, "_h", None) is None for d in decoders):
        raise FloError("decode_streams: a decoder is closed")
    if ctx is None:
        ctx = next((d._ctx for d in decoders if d._ctx is not None), None) or default_context()
    for d in decoders:
        if d._ctx is None:
            d._ctx = ctx
            if d._L.flo_sdec_attach(d._h, ctx._h) != 0:
                raise FloError("a decoder belongs to another context")
            ctx._batches.add(d)
    L = ctx._L
    n = len(decoders)
    hs = C.cast((C.c_void_p * max(n, 1))(*[d._h.value for d in decoders]), C.c_void_p)
    offs = np.zeros(n + 1, np.uint64)
    st = np.zeros(max(n, 1), np.int32)
    dev = torch.device("cuda", ctx.device)
    stream = torch.cuda.current_stream(dev).cuda_stream
    # sizing first (no destination: offsets only, nothing decoded), then the decode into a buffer of that size
    ctx._chk(L.flo_sdec_decode_ready(ctx._h, n, hs, int(max_frames), None, 0, offs.ctypes.data, st.ctypes.data, None))
    need = int(offs[-1])
    if out is None:
        out = torch.empty(max(need, 1), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev or out.numel() < need:
        raise FloError(f"out must be a contiguous float32 tensor of at least {need} elements on {dev}")
    ctx._chk(L.flo_sdec_decode_ready(ctx._h, n, hs, int(max_frames), C.c_void_p(out.data_ptr()), out.numel(), offs.ctypes.data,
                                     st.ctypes.data, C.c_void_p(stream)))
    st = st[:n].copy()
    errors = [decoders[i]._err() if st[i] else "" for i in range(n)]
    return StreamsResult(out[:int(offs[-1])], offs, st, errors)


def resample_out_frames(in_rate, out_rate, in_frames) -> int:
    """flo_resample_out_frames: ceil(in_frames * L / M), the sample-frames a clip of in_frames has after conversion"""
    n = C.c_uint64()
    if _native.lib().flo_resample_out_frames(in_rate, out_rate, in_frames, C.byref(n)) != 0:
        raise FloError(f"unsupported sample-rate conversion {in_rate} -> {out_rate}")
    return int(n.value)


def resample_filter(in_rate, out_rate):
    """flo_resample_filter: (info, table): info a dict with L, M, taps and tile_outputs, table the f32 array [L, taps] of
    the conversion's polyphase filter. Host only: needs no device"""
    L = _native.lib()
    info, tab, err = _native.ResampleInfo(), C.c_void_p(), C.create_string_buffer(256)
    if L.flo_resample_filter(in_rate, out_rate, C.byref(info), C.byref(tab), err, 256) != 0:
        raise FloError(err.value.decode())
    n = info.L * info.taps
    table = np.frombuffer(C.string_at(tab.value, n * 4), np.float32).reshape(info.L, info.taps).copy()
    L.flo_free(tab)
    return dict(L=info.L, M=info.M, taps=info.taps, tile_outputs=info.tile_outputs), table


def resample(samples, in_rate, out_rate, channels) -> np.ndarray:
    """the interleaved f32 clip converted to out_rate on the device (Context.resample on the default context)"""
    return default_context().resample(samples, in_rate, out_rate, channels)


def resample_many(clips, in_rate, out_rate, channels, ctx: Context = None):
    """every clip converted to out_rate: one batch, one launch; a list of f32 arrays (whole sample-frames are converted)"""
    c = ctx or default_context()
    ps = [_f32(x) for x in clips]
    b = Batch(c, MODE_LOSSLESS, [p.size for p in ps], in_rate, channels, 0)
    try:
        for i, p in enumerate(ps):
            c._chk(c._L.flo_batch_upload(b._h, i, p.ctypes.data))
        r = b.resample(out_rate)
        try:
            return [r.download_pcm(i) for i in range(r.n_clips)]
        finally:
            r.close()
    finally:
        b.close()


def _dbtp(linear) -> float:
    v = float(linear)
    return 20.0 * math.log10(v) if v > 1e-9 else (v if v != v else -150.0)


def normalize_lookahead(sample_rate, lookahead_frames=0) -> int:
    """flo_normalize_lookahead: the limiter's look-ahead in frames at sample_rate: lookahead_frames (at most 1024), or for 0
    max(1, round(0.0015 * sample_rate)). Host only: needs no device"""
    opts = _native.NormalizeOpts(-14.0, -1.0, 30.0, _native.NORM_GAIN, int(lookahead_frames))
    n, err = C.c_uint32(), C.create_string_buffer(256)
    if _native.lib().flo_normalize_lookahead(sample_rate, C.byref(opts), C.byref(n), err, 256) != 0:
        raise FloError(err.value.decode())
    return int(n.value)


def _normalize_opts(sample_rate, target_lufs, ceiling_dbtp, limit, lookahead_ms, max_gain_db):
    """flo_normalize_opts of the keyword arguments: 1.5 ms is the library's own default (lookahead_frames 0), any other
    look-ahead is rounded to frames here"""
    frames = 0 if float(lookahead_ms) == 1.5 else max(1, int(math.floor(float(lookahead_ms) * sample_rate / 1000.0 + 0.5)))
    return _native.NormalizeOpts(float(target_lufs), float(ceiling_dbtp), float(max_gain_db),
                                 _native.NORM_LIMIT if limit else _native.NORM_GAIN, frames)


def _normalize_report(r) -> dict:
    status = "non-finite" if r.status & _native.NORM_STATUS_NONFINITE else "silent" if r.status & _native.NORM_STATUS_SILENT else ""
    return dict(input_lufs=r.input_lufs, input_true_peak=float(r.input_true_peak), input_true_peak_dbtp=r.input_true_peak_dbtp,
                gain=float(r.gain), gain_db=r.gain_db, ceiling_reduction_db=r.ceiling_reduction_db, status=status, status_bits=int(r.status),
                limited_frames=int(r.limited_frames), min_gain_q24=int(r.min_gain_q24),
                min_gain_db=20.0 * math.log10(r.min_gain_q24 / 16777216.0) if r.min_gain_q24 else -150.0)


def normalize_gain(integrated_lufs, sample_peak_dbfs, true_peak_linear, target_lufs=-14.0, ceiling_dbtp=-1.0, limit=False,
                   max_gain_db=30.0, lookahead_frames=0) -> dict:
    """flo_normalize_gain: the report of one clip from its measurements alone (limited_frames and min_gain_q24 are the
    kernel's and stay at their start values). Host only: needs no device"""
    opts = _native.NormalizeOpts(float(target_lufs), float(ceiling_dbtp), float(max_gain_db),
                                 _native.NORM_LIMIT if limit else _native.NORM_GAIN, int(lookahead_frames))
    rep, err = _native.NormalizeReport(), C.create_string_buffer(256)
    if _native.lib().flo_normalize_gain(integrated_lufs, sample_peak_dbfs, true_peak_linear, C.byref(opts), C.byref(rep), err, 256) != 0:
        raise FloError(err.value.decode())
    return _normalize_report(rep)


def true_peak(samples, sample_rate, channels) -> float:
    """the interleaved f32 clip's 4x oversampled peak in dBTP, measured on the device (Context.true_peak on the default context)"""
    return default_context().true_peak(samples, sample_rate, channels)


def normalize(samples, sample_rate, channels, **kw):
    """(the interleaved f32 clip at the target level, its report): Context.normalize on the default context"""
    return default_context().normalize(samples, sample_rate, channels, **kw)


def normalize_many(clips, sample_rate, channels, ctx: Context = None, **kw):
    """every clip brought to the target level: one batch, one pass; (a list of f32 arrays, the reports). Keywords as
    Batch.normalize"""
    c = ctx or default_context()
    ps = [_f32(x) for x in clips]
    b = Batch(c, MODE_LOSSLESS, [p.size for p in ps], sample_rate, channels, 0)
    try:
        for i, p in enumerate(ps):
            c._chk(c._L.flo_batch_upload(b._h, i, p.ctypes.data))
        r, reports = b.normalize(**kw)
        try:
            return [r.download_pcm(i) for i in range(r.n_clips)], reports
        finally:
            r.close()
    finally:
        b.close()


def edit_tile_frames(in_channels, out_channels) -> int:
    """flo_edit_tile_frames: the output frames one workgroup of the edit kernel makes. Host only: needs no device"""
    n = C.c_uint32()
    if _native.lib().flo_edit_tile_frames(in_channels, out_channels, C.byref(n)) != 0:
        raise FloError(f"unsupported channel counts {in_channels} -> {out_channels}")
    return int(n.value)


def _ms_frames(ms, sample_rate) -> int:
    return int(math.floor(float(ms) * sample_rate / 1000.0 + 0.5))


def trim_segments(ranges, frames, sample_rate, pre_ms=0.0, post_ms=0.0, fade_ms=0.0) -> list:
    """Batch.trim_silence's segments from the active ranges (first, end) of clips of `frames` frames: start = max(first - pre,
    0), stop = min(end + post, N), nothing for a clip without an active frame; fades of min(round(fade_ms), the cut)"""
    pre, post, fade = _ms_frames(pre_ms, sample_rate), _ms_frames(post_ms, sample_rate), _ms_frames(fade_ms, sample_rate)
    segs = []
    for i, (first, end) in enumerate(np.asarray(ranges, np.uint64).reshape(-1, 2).tolist()):
        start, stop = (max(first - pre, 0), min(end + post, int(frames[i]))) if end else (0, 0)
        f = min(fade, stop - start, (1 << 24) - 1)
        segs.append(dict(clip=i, start=start, frames=stop - start, fade_in=f, fade_out=f))
    return segs


def _edit_segments(segments, clip_frames):
    """the flo_edit_segment array of a list of dicts / EditSegment; `frames` missing or None: to the clip's end"""
    segments = list(segments)
    out = (_native.EditSegment * max(len(segments), 1))()
    for k, g in enumerate(segments):
        if isinstance(g, _native.EditSegment):
            out[k] = g
            continue
        unknown = set(g) - {"clip", "start", "frames", "pad_head", "pad_tail", "fade_in", "fade_out", "reserved"}
        if unknown:
            raise FloError(f"segment {k}: unknown keys {sorted(unknown)}")
        clip, start = int(g.get("clip", 0)), int(g.get("start", 0))
        frames = g.get("frames")
        if frames is None:
            frames = max(int(clip_frames[clip]) - start, 0) if 0 <= clip < len(clip_frames) else 0
        out[k] = _native.EditSegment(start, int(frames), clip, int(g.get("pad_head", 0)), int(g.get("pad_tail", 0)),
                                     int(g.get("fade_in", 0)), int(g.get("fade_out", 0)), int(g.get("reserved", 0)))
    return (_native.EditSegment * len(segments)).from_buffer(out) if segments else (_native.EditSegment * 0)()


def _mix_parts(parts, clip_frames):
    """the flo_mix_part array of a list of dicts / MixPart; clip_frames[b][i]: the frames of clip i of source b. `frames`
    missing or None: to the clip's end"""
    parts = list(parts)
    out = (_native.MixPart * max(len(parts), 1))()
    for k, g in enumerate(parts):
        if isinstance(g, _native.MixPart):
            out[k] = g
            continue
        unknown = set(g) - {"out", "batch", "clip", "start", "frames", "at", "gain", "fade_in", "fade_out"}
        if unknown:
            raise FloError(f"part {k}: unknown keys {sorted(unknown)}")
        if "out" not in g or "clip" not in g:
            raise FloError(f"part {k}: out and clip are required")
        batch, clip, start = int(g.get("batch", 0)), int(g["clip"]), int(g.get("start", 0))
        frames = g.get("frames")
        if frames is None:
            known = 0 <= batch < len(clip_frames) and 0 <= clip < len(clip_frames[batch])
            frames = max(int(clip_frames[batch][clip]) - start, 0) if known else 0
        out[k] = _native.MixPart(start, int(frames), int(g.get("at", 0)), int(g["out"]), batch, clip, int(g.get("fade_in", 0)),
                                 int(g.get("fade_out", 0)), float(g.get("gain", 1.0)))
    return (_native.MixPart * len(parts)).from_buffer(out) if parts else (_native.MixPart * 0)()


def _mix_out_frames(parts) -> list:
    """out_frames=None of Batch.mix: 1 + max(out) outputs, each ending with its furthest part (at + frames)"""
    T = [0] * (1 + max([int(g.out) for g in parts], default=-1))
    for g in parts:
        T[g.out] = max(T[g.out], int(g.at) + int(g.frames))
    return T


def concat_parts(frames, sample_rate, crossfade_ms=0.0, out=0, clips=None, batch=0):
    """(parts, T) of one output that plays clips (indices into `frames`, the frames of every clip of source `batch`; None:
    all of them in order) end to end: Batch.mix's parts of output `out` and its length. Neighbours j, j + 1 overlap by
    xf_j = min(round(crossfade_ms * sample_rate / 1000), N_j, N_j+1) frames (at most 2^24 - 1, the longest fade):
    at_j = at_j-1 + N_j-1 - xf_j-1, fade_in = xf_j-1 (0 for the first), fade_out = xf_j (0 for the last). Pure Python, no device.
    The fades are Batch.edit's linear ones, kept as they are: over a crossfade of xf frames the weights of the clip that
    leaves and of the clip that enters are (xf - 1 - u) / xf and u / xf, which sum to (xf - 1) / xf, not 1. Other curves are
    out of scope."""
    idx = list(range(len(frames))) if clips is None else [int(i) for i in clips]
    want = _ms_frames(crossfade_ms, sample_rate)
    n = [int(frames[i]) for i in idx]
    xf = [min(want, n[j], n[j + 1], (1 << 24) - 1) for j in range(len(n) - 1)]
    parts, at = [], 0
    for j, i in enumerate(idx):
        if j:
            at += n[j - 1] - xf[j - 1]
        parts.append(dict(out=int(out), batch=int(batch), clip=i, start=0, frames=n[j], at=at, gain=1.0,
                          fade_in=xf[j - 1] if j else 0, fade_out=xf[j] if j < len(xf) else 0))
    return parts, (at + n[-1] if n else 0)


def mix(clips, sample_rate, channels, parts, out_frames=None) -> np.ndarray:
    """one clip summed from parts of the interleaved f32 clips, on the device (Context.mix on the default context)"""
    return default_context().mix(clips, sample_rate, channels, parts, out_frames)


def concat(clips, sample_rate, channels, crossfade_ms=0.0) -> np.ndarray:
    """the interleaved f32 clips end to end, neighbours crossfaded over crossfade_ms (concat_parts), on the device"""
    parts, T = concat_parts([_f32(x).size // channels for x in clips], sample_rate, crossfade_ms)
    return mix(clips, sample_rate, channels, parts, T)


def conv_geometry(channels, ir_channels=1) -> dict:
    """flo_conv_geometry: tile_frames, tap_chunk and lane_outputs of the FIR kernel variant these channel counts select. Host
    only: needs no device"""
    info = _native.ConvInfo()
    if _native.lib().flo_conv_geometry(channels, ir_channels, C.byref(info)) != 0:
        raise FloError(f"unsupported channel counts {channels} with a response of {ir_channels}")
    return dict(tile_frames=int(info.tile_frames), tap_chunk=int(info.tap_chunk), lane_outputs=int(info.lane_outputs))


def conv_fft_geometry(channels=2, ir_channels=1) -> dict:
    """flo_conv_fft_geometry: block_frames, lane_blocks, max_taps and crossover_taps of the partitioned FFT convolution. Host
    only: needs no device"""
    info = _native.ConvFftInfo()
    if _native.lib().flo_conv_fft_geometry(channels, ir_channels, C.byref(info)) != 0:
        raise FloError(f"unsupported channel counts {channels} with a response of {ir_channels}")
    return dict(block_frames=int(info.block_frames), lane_blocks=int(info.lane_blocks), max_taps=int(info.max_taps),
                crossover_taps=int(info.crossover_taps))


def _conv_takes_fft(method, jobs, ir_frames, channels=2, ir_channels=1):
    """whether `method` sends this flo_conv_job array down the FFT path; "auto" goes by the call's largest K"""
    if method == "direct":
        return False
    if method == "fft":
        return True
    if method != "auto":
        raise FloError(f"unknown method {method!r}: one of 'direct', 'fft', 'auto'")
    most = 0
    for g in jobs:
        p = int(ir_frames[g.ir]) if g.ir < len(ir_frames) else 0
        most = max(most, min(int(g.taps), p - min(int(g.ir_start), p)))
    # (channel counts the library refuses: the direct call carries the message)
    info = _native.ConvFftInfo()
    return _native.lib().flo_conv_fft_geometry(channels, ir_channels, C.byref(info)) == 0 and most >= info.crossover_taps


_FIR_KINDS = {"lowpass": _native.FIR_LOWPASS, "highpass": _native.FIR_HIGHPASS, "bandpass": _native.FIR_BANDPASS, "bandstop": _native.FIR_BANDSTOP}


def fir_design(kind, rate, f_lo=None, f_hi=None, taps=255, beta=9.0) -> np.ndarray:
    """flo_fir_design: the f32 table of a Kaiser-windowed sinc FIR of `taps` (odd) coefficients at `rate`. kind: "lowpass"
    (below f_hi), "highpass" (above f_lo), "bandpass" (f_lo .. f_hi), "bandstop", or the FLO_FIR_* number. A low-pass given
    only f_lo, or a high-pass given only f_hi, takes that as its one frequency. Host only: needs no device"""
    k = _FIR_KINDS.get(kind, kind) if isinstance(kind, str) else int(kind)
    if not isinstance(k, int):
        raise FloError(f"unknown filter kind {kind!r}: one of {sorted(_FIR_KINDS)}")
    if k == _native.FIR_LOWPASS and f_hi is None:
        f_hi = f_lo
    if k == _native.FIR_HIGHPASS and f_lo is None:
        f_lo = f_hi
    L = _native.lib()
    tab, err = C.c_void_p(), C.create_string_buffer(256)
    if L.flo_fir_design(k, int(rate), float(f_lo or 0.0), float(f_hi or 0.0), int(taps), float(beta), C.byref(tab), err, 256) != 0:
        raise FloError("flo_fir_design: " + err.value.decode())
    table = np.frombuffer(C.string_at(tab.value, int(taps) * 4), np.float32).copy()
    L.flo_free(tab)
    return table


def conv_mode(mode, n, k):
    """(skip, frames) of Batch.convolve's `mode` for a clip of n frames and a response of k taps"""
    if mode == "head":
        return 0, n
    if mode == "full":
        return 0, (n + k - 1 if n and k else 0)
    if mode == "centered":
        return (k - 1) // 2 if k else 0, n
    raise FloError(f"unknown mode {mode!r}: one of 'head', 'full', 'centered'")


def _conv_jobs(jobs, clip_frames, ir_frames, ir=0, mode="head", taps=None):
    """the flo_conv_job array of a list of dicts / ConvJob, or (jobs None) of one job per clip against response `ir` in `mode`"""
    cap = 0xFFFFFFFF if taps is None else int(taps)

    def k_of(j, start, most):
        p = int(ir_frames[j]) if 0 <= j < len(ir_frames) else 0
        return min(most, p - min(start, p))

    if jobs is None:
        irs = [int(x) for x in ir] if isinstance(ir, (list, tuple)) else [int(ir)] * len(clip_frames)
        if len(irs) != len(clip_frames):
            raise FloError(f"ir has {len(irs)} entries, the batch {len(clip_frames)} clips")
        conv_mode(mode, 0, 0)
        jobs = [dict(clip=i, ir=j, taps=cap, **dict(zip(("skip", "frames"), conv_mode(mode, int(n), k_of(j, 0, cap)))))
                for i, (n, j) in enumerate(zip(clip_frames, irs))]
    jobs = list(jobs)
    out = (_native.ConvJob * max(len(jobs), 1))()
    for k, g in enumerate(jobs):
        if isinstance(g, _native.ConvJob):
            out[k] = g
            continue
        unknown = set(g) - {"clip", "ir", "frames", "skip", "ir_start", "taps", "reserved"}
        if unknown:
            raise FloError(f"job {k}: unknown keys {sorted(unknown)}")
        if "clip" not in g:
            raise FloError(f"job {k}: clip is required")
        clip = int(g["clip"])
        frames = g.get("frames")
        if frames is None:
            frames = int(clip_frames[clip]) if 0 <= clip < len(clip_frames) else 0
        t = g.get("taps")
        out[k] = _native.ConvJob(int(frames), int(g.get("skip", 0)), int(g.get("ir_start", 0)), clip, int(g.get("ir", 0)),
                                 0xFFFFFFFF if t is None else int(t), int(g.get("reserved", 0)))
    return (_native.ConvJob * len(jobs)).from_buffer(out) if jobs else (_native.ConvJob * 0)()


def convolve(samples, ir, sample_rate, channels, ir_channels=1, job=None, *, mode="head", taps=None, method="direct") -> np.ndarray:
    """the interleaved f32 clip filtered by the response `ir` on the device (Context.convolve on the default context)"""
    return default_context().convolve(samples, ir, sample_rate, channels, ir_channels, job, mode=mode, taps=taps, method=method)


def fir_filter(samples, sample_rate, channels, kind, f_lo=None, f_hi=None, taps=255, beta=9.0) -> np.ndarray:
    """the interleaved f32 clip through fir_design's linear-phase filter, delay taken off (convolve, mode "centered")"""
    return convolve(samples, fir_design(kind, sample_rate, f_lo, f_hi, taps, beta), sample_rate, channels, 1, mode="centered")


def _edit_matrix(in_channels, out_channels, matrix):
    """(out_channels, the matrix as a contiguous f32 array [Cout * Cin] or None)"""
    if matrix is None:
        return int(in_channels if out_channels is None else out_channels), None
    m = np.ascontiguousarray(matrix, np.float32)
    if m.ndim == 2:
        if m.shape[1] != in_channels or (out_channels is not None and m.shape[0] != out_channels):
            raise FloError(f"matrix is {m.shape[0]} x {m.shape[1]}, the mix {out_channels if out_channels is not None else '?'} x {in_channels}")
        return int(m.shape[0]), m.reshape(-1)
    cout = int(m.size // in_channels if out_channels is None else out_channels)
    if m.ndim != 1 or m.size != cout * in_channels or not cout:
        raise FloError(f"matrix has {m.size} entries, the mix {cout} x {in_channels}")
    return cout, m


def _uploaded(c, clips, sample_rate, channels):
    ps = [_f32(x) for x in clips]
    b = Batch(c, MODE_LOSSLESS, [p.size for p in ps], sample_rate, channels, 0)
    try:
        for i, p in enumerate(ps):
            c._chk(c._L.flo_batch_upload(b._h, i, p.ctypes.data))
        b.sync()
    except Exception:
        b.close()
        raise
    return b


def _fetched(r):
    try:
        return [r.download_pcm(i) for i in range(r.n_clips)]
    finally:
        r.close()


def edit(samples, sample_rate, channels, segment=None, out_channels=None, matrix=None) -> np.ndarray:
    """one cut of the interleaved f32 clip, made on the device (Context.edit on the default context)"""
    return default_context().edit(samples, sample_rate, channels, segment, out_channels, matrix)


def edit_many(clips, sample_rate, channels, segments, out_channels=None, matrix=None, ctx: Context = None):
    """segments (Batch.edit) cut from the clips: one upload, one device pass, one fetch; a list of f32 arrays"""
    b = _uploaded(ctx or default_context(), clips, sample_rate, channels)
    try:
        return _fetched(b.edit(segments, out_channels, matrix))
    finally:
        b.close()


def remix_many(clips, sample_rate, channels, matrix, ctx: Context = None):
    """every clip mixed to len(matrix) channels by matrix [Cout][channels]: one batch, one launch; a list of f32 arrays"""
    b = _uploaded(ctx or default_context(), clips, sample_rate, channels)
    try:
        return _fetched(b.remix(matrix))
    finally:
        b.close()


def remix(samples, sample_rate, channels, matrix) -> np.ndarray:
    """the interleaved f32 clip mixed to len(matrix) channels on the device"""
    return remix_many([samples], sample_rate, channels, matrix)[0]


def active_range_many(clips, sample_rate, channels, threshold_db=-60.0, ctx: Context = None) -> np.ndarray:
    """(n, 2) uint64: every clip's first active frame and last active frame plus one (Batch.active_ranges)"""
    b = _uploaded(ctx or default_context(), clips, sample_rate, channels)
    try:
        return b.active_ranges(threshold_db)
    finally:
        b.close()


def active_range(samples, sample_rate, channels, threshold_db=-60.0):
    """(first, end) of the interleaved f32 clip, measured on the device"""
    r = active_range_many([samples], sample_rate, channels, threshold_db)
    return int(r[0, 0]), int(r[0, 1])


def trim_silence_many(clips, sample_rate, channels, ctx: Context = None, **kw):
    """every clip cut to its active range: one upload, two device passes, one fetch; (a list of f32 arrays, the ranges).
    Keywords as Batch.trim_silence"""
    b = _uploaded(ctx or default_context(), clips, sample_rate, channels)
    try:
        r, ranges = b.trim_silence(**kw)
        return _fetched(r), ranges
    finally:
        b.close()


def trim_silence(samples, sample_rate, channels, **kw):
    """(the interleaved f32 clip cut to its active range, (first, end)): trim_silence_many of one clip"""
    outs, ranges = trim_silence_many([samples], sample_rate, channels, **kw)
    return outs[0], (int(ranges[0, 0]), int(ranges[0, 1]))


def _encode_analysed(mode, samples, sample_rate, channels, quality_or_level, bit_depth, metadata) -> bytes:
    """what the three free functions share (lib.rs:97-206): `add_analysis_data_if_missing(&metadata.unwrap_or_default(), samples,
    sr, ch, 50)`, then the encoder - on ONE copy of the samples: uploaded once, analysed on the device, encoded from there"""
    from . import meta as _meta
    ctx = default_context()
    p = _f32(samples)
    b = Batch(ctx, mode, [p.size], sample_rate, channels, quality_or_level)
    try:
        b.upload(0, p)
        m = _meta.merge_analysis(metadata or b"", b.analysis_metadata(0, 50))
        if mode == MODE_LOSSLESS:
            b.set_bit_depth(bit_depth)
        b.encode(0)
        b.sync()
        return b.fetch(0, m)
    finally:
        b.close()


def encode(samples, sample_rate, channels, bit_depth, metadata=None) -> bytes:
    """libflo::encode (lib.rs:97-117): analysis metadata first (waveform peaks, spectral fingerprint, EBU R128 loudness,
    length), then the lossless encoder at level 5"""
    return _encode_analysed(MODE_LOSSLESS, samples, sample_rate, channels, 5, bit_depth, metadata)


def _lossy_quality(quality: int) -> float:
    """libflo::encode_lossy's quality level 0-4 -> 0.0/0.35/0.55/0.75/1.0 (lib.rs:135-166)"""
    return {0: 0.0, 1: 0.35, 2: 0.55, 3: 0.75}.get(int(quality), 1.0)


def encode_lossy(samples, sample_rate, channels, _bit_depth, quality: int, metadata=None) -> bytes:
    """libflo::encode_lossy (lib.rs:135-166): quality level 0-4 -> 0.0/0.35/0.55/0.75/1.0"""
    q = _lossy_quality(quality)
    return _encode_analysed(MODE_LOSSY, samples, sample_rate, channels, q, 16, metadata)


def encode_with_bitrate(samples, sample_rate, channels, _bit_depth, target_bitrate_kbps, metadata=None) -> bytes:
    """libflo::encode_with_bitrate (lib.rs:181-206)"""
    q = QualityPreset.from_bitrate(target_bitrate_kbps, sample_rate, channels).as_f32()
    return _encode_analysed(MODE_LOSSY, samples, sample_rate, channels, q, 16, metadata)


def _encode_analysed_many(mode, clips, sample_rate, channels, quality_or_level, bit_depth, metadata):
    """_encode_analysed for many clips: every clip uploaded into one batch (one flo_batch_upload each, one sync), ONE
    batched analysis (Batch.analysis_metadata_all), one encode, then each file with its META. metadata: None, one bytes
    for every clip, or one entry per clip"""
    from . import meta as _meta
    ps = [_f32(x) for x in clips]
    if metadata is None or isinstance(metadata, (bytes, bytearray)):
        user = [bytes(metadata or b"")] * len(ps)
    else:
        user = [bytes(m or b"") for m in metadata]
        if len(user) != len(ps):
            raise ValueError(f"metadata has {len(user)} entries for {len(ps)} clips")
    if not ps:
        return []
    ctx = default_context()
    b = Batch(ctx, mode, [p.size for p in ps], sample_rate, channels, quality_or_level)
    try:
        for i, p in enumerate(ps):
            ctx._chk(b._L.flo_batch_upload(b._h, i, p.ctypes.data))
        b.sync()   # (the copies have read ps)
        metas = b.analysis_metadata_all(50)
        if mode == MODE_LOSSLESS:
            b.set_bit_depth(bit_depth)
        b.encode(0)
        b.sync()
        return [b.fetch(i, _meta.merge_analysis(user[i], metas[i])) for i in range(len(ps))]
    finally:
        b.close()


def encode_many(clips, sample_rate, channels, bit_depth, metadata=None):
    """encode (libflo::encode) of every clip, the analysis of all of them in one device pass: a list of files"""
    return _encode_analysed_many(MODE_LOSSLESS, clips, sample_rate, channels, 5, bit_depth, metadata)


def encode_lossy_many(clips, sample_rate, channels, _bit_depth, quality: int, metadata=None):
    """encode_lossy (libflo::encode_lossy) of every clip, the analysis of all of them in one device pass. A clip whose
    length is not a whole number of sample-frames is analysed over all of its samples, as the reference does"""
    q = _lossy_quality(quality)
    return _encode_analysed_many(MODE_LOSSY, clips, sample_rate, channels, q, 16, metadata)


def encode_with_bitrate_many(clips, sample_rate, channels, _bit_depth, target_bitrate_kbps, metadata=None):
    """encode_with_bitrate (libflo::encode_with_bitrate) of every clip, the analysis of all of them in one device pass"""
    q = QualityPreset.from_bitrate(target_bitrate_kbps, sample_rate, channels).as_f32()
    return _encode_analysed_many(MODE_LOSSY, clips, sample_rate, channels, q, 16, metadata)


# -- size curves and the rate-targeted encode ---------------------------------------------------------------------------
DEFAULT_RATE_GRID = tuple(i / 16 for i in range(17))   # 0, 1/16, ..., 15/16, 1.0


def rate_pick(qualities, sizes, budget):
    """flo_rate_pick: (index, fits) of the candidate of the largest quality value whose size is <= budget (every candidate
    is looked at; equal qualities: the lower index); when none fits, the candidate of the smallest quality, fits False"""
    q = np.ascontiguousarray(qualities, dtype=np.float32).reshape(-1)
    z = np.ascontiguousarray(sizes, dtype=np.uint64).reshape(-1)
    if q.size != z.size:
        raise ValueError(f"{q.size} qualities for {z.size} sizes")
    idx, fits = C.c_uint32(), C.c_int()
    rc = _native.lib().flo_rate_pick(q.size, q.ctypes.data, z.ctypes.data, int(budget), C.byref(idx), C.byref(fits))
    if rc != _native.OK:
        raise FloError("flo_rate_pick: 1 to 32 candidates")
    return idx.value, bool(fits.value)


def size_curve(samples, sample_rate, channels, qualities=DEFAULT_RATE_GRID) -> np.ndarray:
    """the K file sizes (bytes, empty META) of one clip encoded at each candidate quality, measured on the device"""
    p = _f32(samples)
    b = Batch(default_context(), MODE_LOSSY, [p.size], sample_rate, channels, 0.0)
    try:
        b.upload(0, p)
        return b.size_curve(qualities)[0]
    finally:
        b.close()


def encode_ladder(samples, sample_rate, channels, qualities, metadata=None):
    """The clip at every quality of the ladder, from one upload, one analysis and one transform pass: a list of files, rung
    j being what encode_lossy's route (_encode_analysed) returns at qualities[j], analysis META merged (a trailing partial
    sample-frame is analysed as encode_lossy_many analyses it: over all of the caller's samples)"""
    return encode_ladder_many([samples], sample_rate, channels, qualities, [metadata] if metadata is not None else None)[0]


def encode_ladder_many(clips, sample_rate, channels, qualities, metadata=None):
    """encode_ladder of every clip: one upload, ONE batched analysis, one ladder. metadata: None, one bytes for every clip, or
    one entry per clip. Returns files[clip][rung]"""
    from . import meta as _meta
    ps = [_f32(x) for x in clips]
    n = len(ps)
    if metadata is None or isinstance(metadata, (bytes, bytearray)):
        user = [bytes(metadata or b"")] * n
    else:
        user = [bytes(m or b"") for m in metadata]
        if len(user) != n:
            raise ValueError(f"metadata has {len(user)} entries for {n} clips")
    q = np.ascontiguousarray(qualities, dtype=np.float32).reshape(-1)
    if not ps:
        return []
    ctx = default_context()
    b = Batch(ctx, MODE_LOSSY, [p.size for p in ps], sample_rate, channels, float(q[0]) if q.size else 0.0)
    try:
        for i, p in enumerate(ps):
            ctx._chk(b._L.flo_batch_upload(b._h, i, p.ctypes.data))
        b.sync()   # (the copies have read ps)
        metas = [_meta.merge_analysis(user[i], m) for i, m in enumerate(b.analysis_metadata_all(50))]
        with b.encode_ladder(q) as lad:
            return [[lad.fetch(i, j, metas[i]) for j in range(lad.n_rungs)] for i in range(n)]
    finally:
        b.close()


def _target_bytes(target_kbps, sample_frames, sample_rate) -> int:
    """kbps over the clip's duration, for the whole file: floor(kbps * 125 * sample_frames / sample_rate)"""
    from fractions import Fraction
    return int(Fraction(target_kbps) * 125 * sample_frames / sample_rate)


def _rate_info(q, idx, fits, size, target):
    return {"quality": float(q[idx]), "index": int(idx), "fits": bool(fits), "file_bytes": int(size), "target_bytes": int(target)}


def encode_to_bitrate(samples, sample_rate, channels, target_kbps, qualities=DEFAULT_RATE_GRID, metadata=None, with_info=False,
                      _analysis=True):
    """Like encode_with_bitrate (analysis META merged), but the quality is MEASURED: the best candidate quality whose whole
    file, META included, is at most floor(target_kbps * 125 * sample_frames / sample_rate) bytes. One batch: upload,
    analysis, size curve, set_quality, encode. with_info adds {"quality", "index", "fits", "file_bytes", "target_bytes"}"""
    from . import meta as _meta
    p = _f32(samples)
    q = np.ascontiguousarray(qualities, dtype=np.float32).reshape(-1)
    b = Batch(default_context(), MODE_LOSSY, [p.size], sample_rate, channels, float(q[0]))
    try:
        b.upload(0, p)
        m = _meta.merge_analysis(metadata or b"", b.analysis_metadata(0, 50)) if _analysis else bytes(metadata or b"")
        sizes = b.size_curve(q)[0]
        target = _target_bytes(target_kbps, p.size // channels, sample_rate)
        idx, fits = rate_pick(q, sizes, max(target - len(m), 0))
        b.set_quality(float(q[idx]))
        b.encode(0)
        b.sync()
        f = b.fetch(0, m)
        return (f, _rate_info(q, idx, fits, len(f), target)) if with_info else f
    finally:
        b.close()


def encode_to_bitrate_many(clips, sample_rate, channels, target_kbps, qualities=DEFAULT_RATE_GRID, metadata=None, with_info=False):
    """encode_to_bitrate of every clip: one upload, ONE batched analysis, one size curve, then every clip encoded once at
    its own chosen quality (a batch per chosen candidate, filled on the device). target_kbps: one number or one per clip;
    metadata: None, one bytes for every clip, or one entry per clip. Returns the files, with_info: (files, infos)"""
    from . import meta as _meta
    ps = [_f32(x) for x in clips]
    n = len(ps)
    if metadata is None or isinstance(metadata, (bytes, bytearray)):
        user = [bytes(metadata or b"")] * n
    else:
        user = [bytes(m or b"") for m in metadata]
        if len(user) != n:
            raise ValueError(f"metadata has {len(user)} entries for {n} clips")
    kbps = list(target_kbps) if np.ndim(target_kbps) else [target_kbps] * n
    if len(kbps) != n:
        raise ValueError(f"target_kbps has {len(kbps)} entries for {n} clips")
    if not ps:
        return ([], []) if with_info else []
    q = np.ascontiguousarray(qualities, dtype=np.float32).reshape(-1)
    ctx = default_context()
    b = Batch(ctx, MODE_LOSSY, [p.size for p in ps], sample_rate, channels, float(q[0]))
    kids = []
    try:
        for i, p in enumerate(ps):
            ctx._chk(b._L.flo_batch_upload(b._h, i, p.ctypes.data))
        b.sync()   # (the copies have read ps)
        metas = [_meta.merge_analysis(user[i], m) for i, m in enumerate(b.analysis_metadata_all(50))]
        sizes = b.size_curve(q)
        targets = [_target_bytes(kbps[i], ps[i].size // channels, sample_rate) for i in range(n)]
        picks = [rate_pick(q, sizes[i], max(targets[i] - len(metas[i]), 0)) for i in range(n)]
        files = [None] * n
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        for j in sorted(set(idx for idx, _ in picks)):
            members = [i for i in range(n) if picks[i][0] == j]
            if len(members) == n:
                e = b
                e.set_quality(float(q[j]))
            else:   # the chosen candidate's clips, copied device to device, nothing re-uploaded
                e = Batch(ctx, MODE_LOSSY, [ps[i].size for i in members], sample_rate, channels, float(q[j]))
                kids.append(e)
                e.sync()   # (the new batch's zero padding is written on the context's stream; the copies are not)
                for k, i in enumerate(members):
                    nb = (ps[i].size // channels) * channels * 4
                    if nb and hip.hipMemcpy(e.clip_device_ptr(k), b._L.flo_batch_clip_device_data(b._h, i), nb, 3) != 0:
                        raise FloError("hipMemcpy (device to device) failed")
                if hip.hipDeviceSynchronize() != 0:   # (the encode runs on the context's stream: behind the copies)
                    raise FloError("hipDeviceSynchronize failed")
            e.encode(0)
            e.sync()
            for k, i in enumerate(members):
                files[i] = e.fetch(i if e is b else k, metas[i])
            if e is not b:
                e.close()
        if with_info:
            return files, [_rate_info(q, picks[i][0], picks[i][1], len(files[i]), targets[i]) for i in range(n)]
        return files
    finally:
        for e in kids:
            e.close()
        b.close()


# -- spectral similarity (core/analysis.rs:359-437) -----------------------------------------------------------------------
FINGERPRINT_DTYPE = np.dtype([("hash", "u1", 32), ("duration_ms", "<u4"), ("sample_rate", "<u4"), ("channels", "u1"),
                              ("avg_loudness", "u1"), ("pad0", "u1"), ("pad1", "u1"), ("frequency_peaks", "u1", 8),
                              ("energy_profile", "u1", 16)])   # flo_fingerprint of include/flo_hip.h
assert FINGERPRINT_DTYPE.itemsize == C.sizeof(_native.Fingerprint)


def fingerprint_array(fps) -> np.ndarray:
    """Fingerprints as a contiguous FINGERPRINT_DTYPE array. Takes such an array, one fingerprint dict or a sequence of
    them: the dicts Context.analyze / Batch.analyze_all return, or SpectralFingerprint fields as the META holds them."""
    if isinstance(fps, np.void):   # one record of such an array
        fps = np.array(fps, fps.dtype)
    if isinstance(fps, np.ndarray) and fps.dtype.names:
        if fps.dtype != FINGERPRINT_DTYPE:
            raise FloError(f"fingerprint array must have dtype {FINGERPRINT_DTYPE}")
        return np.ascontiguousarray(fps.reshape(-1))
    if isinstance(fps, dict):
        fps = [fps]
    fps = list(fps)
    out = np.zeros(len(fps), FINGERPRINT_DTYPE)
    for i, f in enumerate(fps):
        h = bytes(bytearray(f["hash"]))
        if len(h) != 32 or len(f["frequency_peaks"]) != 8 or len(f["energy_profile"]) != 16:
            raise FloError(f"fingerprint {i}: hash, frequency_peaks and energy_profile must hold 32, 8 and 16 bytes")
        out[i]["hash"] = np.frombuffer(h, np.uint8)
        out[i]["duration_ms"] = int(f.get("duration_ms", 0))
        out[i]["sample_rate"] = int(f["sample_rate"])
        out[i]["channels"] = int(f["channels"])
        out[i]["avg_loudness"] = int(f["avg_loudness"])
        out[i]["frequency_peaks"] = np.asarray(f["frequency_peaks"], np.uint8)
        out[i]["energy_profile"] = np.asarray(f["energy_profile"], np.uint8)
    return out


def spectral_similarity(fp_a, fp_b) -> np.float32:
    """spectral_similarity (analysis.rs:395-437; spectral_similarity_score, lib.rs:1357), bit for bit; on the host"""
    a, b = fingerprint_array(fp_a), fingerprint_array(fp_b)
    if a.size != 1 or b.size != 1:
        raise FloError("spectral_similarity compares two single fingerprints")
    fpp = C.POINTER(_native.Fingerprint)
    return np.float32(_native.lib().flo_spectral_similarity(C.cast(a.ctypes.data, fpp), C.cast(b.ctypes.data, fpp)))


def extract_dominant_frequencies(fp, num_frequencies: int):
    """extract_dominant_frequencies (analysis.rs:367-387): one frame of at most 8 frequencies in Hz (f64), the peak bands
    mapped back from 0..255 to 0 .. Nyquist"""
    f = fingerprint_array(fp)[0]
    n = min(int(num_frequencies), 8)
    return [[float(f["frequency_peaks"][i]) / 255.0 * (float(f["sample_rate"]) / 2.0) for i in range(n)]]


def file_metadata(flo_bytes: bytes):
    """the decoded META chunk of a .flo file (a dict), or None when it has none (reflo::get_metadata)"""
    from . import meta as _meta
    i = probe_container(flo_bytes)
    meta_size = int.from_bytes(flo_bytes[62:70], "little")
    start = i.data_start + i.data_size + int.from_bytes(flo_bytes[54:62], "little")
    if meta_size == 0 or start + meta_size > len(flo_bytes):
        return None
    return _meta.unpack(flo_bytes[start:start + meta_size])


def fingerprints_from_files(files) -> np.ndarray:
    """The `spectrum_fingerprint` each file's META carries (what libflo::encode* store: rmp_serde::to_vec_named of the
    SpectralFingerprint, lib.rs:244-258), as a FINGERPRINT_DTYPE array. Files are paths or file bytes; a file without a
    fingerprint raises FloError naming it."""
    from . import meta as _meta
    out = []
    for n, f in enumerate(files):
        if isinstance(f, (bytes, bytearray, memoryview)):
            name, data = f"file {n}", bytes(f)
        else:
            name = str(f)
            with open(f, "rb") as fh:
                data = fh.read()
        try:
            md = file_metadata(data)
        except FloError as ex:
            raise FloError(f"{name}: {ex}") from None
        raw = md.get("spectrum_fingerprint") if isinstance(md, dict) else None
        if not isinstance(raw, (bytes, bytearray)) or not raw:
            raise FloError(f"{name}: no spectrum_fingerprint in the file's metadata")
        try:
            out.append(fingerprint_array(_meta.unpack(bytes(raw)))[0])
        except (KeyError, TypeError, ValueError, FloError) as ex:
            raise FloError(f"{name}: unreadable spectrum_fingerprint ({ex})") from None
    return np.array(out, FINGERPRINT_DTYPE)


class FingerprintIndex:
    """Fingerprints resident on the device (flo_fpindex), compared under spectral_similarity at collection scale.

    topk(queries, k) / topk_self(k) -> (idx [n, k] uint32, score [n, k] float32): the k best members per query, score
    descending then member index ascending; topk_self never lists a member as its own neighbour. Slots beyond the
    candidates hold 0xFFFFFFFF and -1.0. pairs(threshold) -> (i, j, score): every pair i < j scoring >= threshold,
    ordered by (i, j). Every score is the reference's, bit for bit; k is at most 64."""

    def __init__(self, fps, ctx=None):
        self._ctx = ctx or default_context()
        self._L = self._ctx._L
        arr = fingerprint_array(fps)
        h = C.c_void_p()
        self._ctx._chk(self._L.flo_fpindex_create(self._ctx._h, arr.ctypes.data, arr.size, C.byref(h)))
        self._h = h
        self.n = arr.size
        self._pair_cap = 1 << 16
        self._ctx._batches.add(self)   # closed before its context

    def __len__(self):
        return self.n

    @staticmethod
    def _k(k):
        k = int(k)
        if k < 0:
            raise FloError("k must not be negative")
        return k

    def topk(self, queries, k: int):
        q, k = fingerprint_array(queries), self._k(k)
        idx, score = np.empty((q.size, k), np.uint32), np.empty((q.size, k), np.float32)
        self._ctx._chk(self._L.flo_fpindex_topk(self._h, q.ctypes.data, q.size, k, idx.ctypes.data, score.ctypes.data))
        return idx, score

    def topk_self(self, k: int):
        k = self._k(k)
        idx, score = np.empty((self.n, k), np.uint32), np.empty((self.n, k), np.float32)
        self._ctx._chk(self._L.flo_fpindex_topk_self(self._h, k, idx.ctypes.data, score.ctypes.data))
        return idx, score

    def pairs(self, threshold: float):
        n = C.c_uint64()
        while True:
            cap = self._pair_cap
            i, j, s = np.empty(cap, np.uint32), np.empty(cap, np.uint32), np.empty(cap, np.float32)
            rc = self._L.flo_fpindex_pairs(self._h, float(threshold), cap, i.ctypes.data, j.ctypes.data, s.ctypes.data,
                                           C.byref(n))
            if rc == 3 and n.value > cap:   # FLO_ERR_NOMEM: room for the exact count, then again
                self._pair_cap = int(n.value)
                continue
            self._ctx._chk(rc)
            m = int(n.value)
            return i[:m].copy(), j[:m].copy(), s[:m].copy()

    def close(self):
        if getattr(self, "_h", None):
            self._L.flo_fpindex_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
