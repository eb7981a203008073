"""ctypes loader of the product library flo_amd/libflo_hip.so (C ABI in include/flo_hip.h).

There is no CPU path behind this module: if the shared library is missing, or no gfx950 device can be opened,
every entry point raises. torch is imported first on purpose — its bundled HIP runtime carries the same SONAME
as /opt/rocm's, so loading in this order gives the process ONE HIP runtime and lets torch tensors / RCCL and
this library's kernels share device pointers and streams.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("FLO_HIP_LIB") or os.path.join(_HERE, "libflo_hip.so")   # FLO_HIP_LIB: diagnostic builds
_LIB = None

OK = 0
MODE_LOSSLESS, MODE_LOSSY = 0, 1

EXPORTS = [
    "flo_ctx_create", "flo_ctx_destroy", "flo_last_error", "flo_last_create_error", "flo_free", "flo_ctx_device_info",
    "flo_encode_lossy", "flo_encode_lossless", "flo_encode_batch", "flo_decode", "flo_decode_lossless_i32", "flo_probe_container",
    "flo_batch_create", "flo_batch_destroy", "flo_batch_clip_device_ptr", "flo_batch_upload",
    "flo_batch_fill_synthetic", "flo_batch_encode", "flo_batch_sync", "flo_batch_data_bytes", "flo_batch_fetch",
    "flo_batch_device_streams", "flo_batch_pack_streams", "flo_batch_decode",
    "flo_batch_device_files", "flo_batch_pack_files",
    "flo_ctx_profile_enable", "flo_ctx_profile_query", "flo_ctx_profile_reset", "flo_ctx_force_path", "flo_ctx_stream",
    "flo_debug_pool_fill", "flo_debug_stream_delay", "flo_debug_stream_delays", "flo_debug_delay_enqueue",
    "flo_mdct_forward", "flo_lossy_analyze", "flo_lossy_quantize", "flo_lossy_quantize_smr", "flo_sparse_pack",
    "flo_lossy_pack_frames",
    "flo_dist_unique_id", "flo_dist_create", "flo_dist_destroy", "flo_dist_gather_submit", "flo_dist_gather_flush",
    "flo_dist_gather_result", "flo_dist_stream", "flo_ctx_reserve_cus", "flo_ctx_reserved_cus", "flo_ctx_upload_path",
    "flo_dist_table_submit", "flo_dist_table_flush", "flo_dist_table_result",
    "flo_stream_create", "flo_stream_destroy", "flo_stream_push", "flo_stream_pending_samples", "flo_stream_pending_frames",
    "flo_stream_next_frame", "flo_stream_flush", "flo_stream_finalize",
    "flo_stream_create_lossy", "flo_stream_append", "flo_stream_encode_ready",
    "flo_analyze", "flo_analysis_metadata", "flo_batch_analysis_metadata", "flo_batch_set_bit_depth",
    "flo_batch_analyze_all", "flo_batch_analysis_metadata_all", "flo_batch_clip_device_data",
    "flo_get_toc", "flo_seek_to_time", "flo_decode_frame_at",
    "flo_corpus_create", "flo_corpus_destroy", "flo_corpus_format", "flo_corpus_file_frames", "flo_corpus_decode_windows",
    "flo_corpus_sync",
    "flo_sdec_create", "flo_sdec_destroy", "flo_sdec_attach", "flo_sdec_last_error", "flo_sdec_feed", "flo_sdec_state",
    "flo_sdec_info", "flo_sdec_frames_available", "flo_sdec_available_frames", "flo_sdec_current_frame_index",
    "flo_sdec_buffered_bytes", "flo_sdec_next_frame", "flo_sdec_decode_available", "flo_sdec_reset", "flo_sdec_decode_ready",
    "flo_spectral_similarity", "flo_fpindex_create", "flo_fpindex_destroy", "flo_fpindex_topk", "flo_fpindex_topk_self",
    "flo_fpindex_pairs", "flo_batch_fidelity", "flo_compare",
    "flo_batch_size_curve", "flo_batch_set_quality", "flo_rate_pick", "flo_encode_batch_to_size",
    "flo_batch_encode_ladder", "flo_ladder_shape", "flo_ladder_file_bytes", "flo_ladder_fetch", "flo_ladder_device_files",
    "flo_ladder_destroy", "flo_encode_batch_ladder",
    "flo_resample_filter", "flo_resample_out_frames", "flo_batch_resample", "flo_resample",
    "flo_batch_true_peak", "flo_normalize_gain", "flo_normalize_lookahead", "flo_batch_normalize", "flo_normalize",
    "flo_batch_edit", "flo_batch_active_range", "flo_edit", "flo_edit_tile_frames",
    "flo_batch_mix", "flo_mix",
    "flo_batch_convolve", "flo_convolve", "flo_conv_geometry", "flo_fir_design",
    "flo_batch_convolve_fft", "flo_convolve_fft", "flo_conv_fft_geometry",
]


class Analysis(C.Structure):
    _fields_ = [("n_peaks", C.c_uint32), ("duration_ms", C.c_uint32), ("sample_rate", C.c_uint32), ("channels", C.c_uint8),
                ("avg_loudness", C.c_uint8), ("pad0", C.c_uint8), ("pad1", C.c_uint8), ("hash", C.c_uint8 * 32),
                ("frequency_peaks", C.c_uint8 * 8), ("energy_profile", C.c_uint8 * 16), ("integrated_lufs", C.c_double),
                ("length_ms", C.c_uint64), ("loudness_range_lu", C.c_double), ("true_peak_dbtp", C.c_double),
                ("sample_peak_dbfs", C.c_double), ("sum_squares", C.c_float), ("pad2", C.c_uint32)]


class ContainerInfo(C.Structure):
    _fields_ = [("version_major", C.c_uint8), ("version_minor", C.c_uint8), ("channels", C.c_uint8), ("bit_depth", C.c_uint8),
                ("compression_level", C.c_uint8), ("is_transform", C.c_uint8), ("pad0", C.c_uint8), ("pad1", C.c_uint8),
                ("flags", C.c_uint16), ("pad2", C.c_uint16), ("sample_rate", C.c_uint32), ("data_crc32", C.c_uint32),
                ("n_frames", C.c_uint32), ("total_samples", C.c_uint64), ("data_start", C.c_uint64), ("data_size", C.c_uint64),
                ("frame_samples_sum", C.c_uint64)]


class TocEntryC(C.Structure):
    _fields_ = [("frame_index", C.c_uint32), ("frame_size", C.c_uint32), ("byte_offset", C.c_uint64), ("timestamp_ms", C.c_uint32),
                ("pad", C.c_uint32)]


class SeekResultC(C.Structure):
    _fields_ = [("frame_index", C.c_uint32), ("timestamp_ms", C.c_uint32), ("byte_offset", C.c_uint64), ("sample_offset", C.c_uint32),
                ("next_timestamp_ms", C.c_uint32)]


class SdecInfoC(C.Structure):
    _fields_ = [("sample_rate", C.c_uint32), ("channels", C.c_uint8), ("bit_depth", C.c_uint8), ("is_lossy", C.c_uint8),
                ("pad", C.c_uint8), ("total_samples", C.c_uint64)]


class Fingerprint(C.Structure):   # flo_fingerprint (SpectralFingerprint, core/analysis.rs:10-26)
    _fields_ = [("hash", C.c_uint8 * 32), ("duration_ms", C.c_uint32), ("sample_rate", C.c_uint32), ("channels", C.c_uint8),
                ("avg_loudness", C.c_uint8), ("pad0", C.c_uint8), ("pad1", C.c_uint8), ("frequency_peaks", C.c_uint8 * 8),
                ("energy_profile", C.c_uint8 * 16)]


class FidelityBlock(C.Structure):   # flo_fidelity_block
    _fields_ = [("signal", C.c_double), ("error", C.c_double), ("peak_error", C.c_float), ("peak_out", C.c_float),
                ("clipped", C.c_uint32), ("n", C.c_uint32)]


class Fidelity(C.Structure):   # flo_fidelity: one channel of one clip
    _fields_ = [("signal", C.c_double), ("error", C.c_double), ("tail_energy", C.c_double), ("snr_db", C.c_double),
                ("seg_snr_db", C.c_double), ("peak_error", C.c_float), ("peak_out", C.c_float), ("clipped", C.c_uint64),
                ("compared_frames", C.c_uint64), ("source_frames", C.c_uint64), ("decoded_frames", C.c_uint64),
                ("n_blocks", C.c_uint32), ("seg_blocks", C.c_uint32)]


class ResampleInfo(C.Structure):   # flo_resample_info
    _fields_ = [("L", C.c_uint32), ("M", C.c_uint32), ("taps", C.c_uint32), ("tile_outputs", C.c_uint32)]


NORM_GAIN, NORM_LIMIT = 0, 1
NORM_STATUS_SILENT, NORM_STATUS_NONFINITE = 1, 2


class NormalizeOpts(C.Structure):   # flo_normalize_opts
    _fields_ = [("target_lufs", C.c_double), ("ceiling_dbtp", C.c_double), ("max_gain_db", C.c_double), ("mode", C.c_uint32),
                ("lookahead_frames", C.c_uint32)]


class NormalizeReport(C.Structure):   # flo_normalize_report
    _fields_ = [("input_lufs", C.c_double), ("input_true_peak_dbtp", C.c_double), ("gain_db", C.c_double),
                ("ceiling_reduction_db", C.c_double), ("input_true_peak", C.c_float), ("gain", C.c_float), ("status", C.c_uint32),
                ("min_gain_q24", C.c_uint32), ("limited_frames", C.c_uint64)]


class EditSegment(C.Structure):   # flo_edit_segment
    _fields_ = [("start", C.c_uint64), ("frames", C.c_uint64), ("clip", C.c_uint32), ("pad_head", C.c_uint32), ("pad_tail", C.c_uint32),
                ("fade_in", C.c_uint32), ("fade_out", C.c_uint32), ("reserved", C.c_uint32)]


class MixPart(C.Structure):   # flo_mix_part
    _fields_ = [("start", C.c_uint64), ("frames", C.c_uint64), ("at", C.c_uint64), ("out", C.c_uint32), ("batch", C.c_uint32), ("clip", C.c_uint32),
                ("fade_in", C.c_uint32), ("fade_out", C.c_uint32), ("gain", C.c_float)]


class ConvJob(C.Structure):   # flo_conv_job
    _fields_ = [("frames", C.c_uint64), ("skip", C.c_uint64), ("ir_start", C.c_uint64), ("clip", C.c_uint32), ("ir", C.c_uint32),
                ("taps", C.c_uint32), ("reserved", C.c_uint32)]


class ConvInfo(C.Structure):   # flo_conv_info
    _fields_ = [("tile_frames", C.c_uint32), ("tap_chunk", C.c_uint32), ("lane_outputs", C.c_uint32)]


class ConvFftInfo(C.Structure):   # flo_conv_fft_info
    _fields_ = [("block_frames", C.c_uint32), ("lane_blocks", C.c_uint32), ("max_taps", C.c_uint32), ("crossover_taps", C.c_uint32)]


CONV_MAX_TAPS = 65536
CONV_FFT_MAX_TAPS = 1048576
FIR_LOWPASS, FIR_HIGHPASS, FIR_BANDPASS, FIR_BANDSTOP = 0, 1, 2, 3


class FloError(RuntimeError):
    pass


def lib_path():
    return _SO


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_SO):
        raise FloError(f"{_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950). flo_amd has no CPU fallback.")
    try:
        import torch  # noqa: F401  (one HIP runtime per process, see module docstring)
    except Exception:
        pass
    L = C.CDLL(_SO)
    vp, sz, u8p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint8)
    L.flo_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.flo_ctx_destroy.argtypes = [vp]
    L.flo_ctx_destroy.restype = None
    L.flo_last_error.argtypes = [vp]
    L.flo_last_error.restype = C.c_char_p
    L.flo_last_create_error.restype = C.c_char_p
    L.flo_free.argtypes = [vp]
    L.flo_free.restype = None
    L.flo_ctx_device_info.argtypes = [vp, C.c_char_p, sz, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
    L.flo_encode_lossy.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint8, C.c_float, C.c_char_p, sz, C.POINTER(vp), C.POINTER(sz)]
    L.flo_encode_lossless.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint8, C.c_uint8, C.c_uint8, C.c_char_p, sz,
                                      C.POINTER(vp), C.POINTER(sz)]
    L.flo_encode_batch.argtypes = [vp, C.c_int, sz, C.POINTER(vp), C.POINTER(sz), C.c_uint32, C.c_uint8, C.c_float,
                                   C.POINTER(vp), C.POINTER(sz)]
    L.flo_batch_create.argtypes = [vp, C.c_int, sz, C.POINTER(sz), C.c_uint32, C.c_uint8, C.c_float, C.POINTER(vp)]
    L.flo_batch_destroy.argtypes = [vp]
    L.flo_batch_destroy.restype = None
    L.flo_batch_clip_device_ptr.argtypes = [vp, sz]
    L.flo_batch_clip_device_ptr.restype = vp
    L.flo_batch_upload.argtypes = [vp, sz, vp]
    L.flo_batch_fill_synthetic.argtypes = [vp, C.c_uint32, C.c_uint64]
    L.flo_batch_encode.argtypes = [vp, C.c_int]
    L.flo_batch_sync.argtypes = [vp]
    L.flo_batch_data_bytes.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.flo_batch_fetch.argtypes = [vp, sz, C.c_char_p, sz, C.POINTER(vp), C.POINTER(sz)]
    L.flo_batch_device_streams.argtypes = [vp, C.POINTER(vp), C.POINTER(C.POINTER(C.c_uint64)),
                                           C.POINTER(C.POINTER(C.c_uint64))]
    L.flo_batch_pack_streams.argtypes = [vp, vp, sz, C.POINTER(C.c_uint64)]
    L.flo_batch_pack_files.argtypes = [vp, vp, sz, C.POINTER(C.c_uint64)]
    L.flo_batch_device_files.argtypes = L.flo_batch_device_streams.argtypes
    L.flo_batch_decode.argtypes = [vp, vp, sz, C.POINTER(C.c_uint64)]
    L.flo_ctx_profile_enable.argtypes = [vp, C.c_int]
    L.flo_ctx_profile_query.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.flo_ctx_profile_reset.argtypes = [vp]
    L.flo_ctx_force_path.argtypes = [vp, C.c_int]
    L.flo_debug_pool_fill.argtypes = [C.c_int]
    L.flo_debug_stream_delay.argtypes = [C.c_int]
    L.flo_debug_stream_delays.argtypes = []
    L.flo_debug_stream_delays.restype = C.c_uint64
    L.flo_debug_delay_enqueue.argtypes = [vp, C.c_int]
    L.flo_ctx_stream.argtypes = [vp]
    L.flo_ctx_stream.restype = vp
    L.flo_mdct_forward.argtypes = [vp, vp, sz, vp]
    L.flo_lossy_analyze.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint8, C.c_float, vp, vp, vp, C.POINTER(sz)]
    L.flo_lossy_quantize.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint8, C.c_float, C.c_int, vp, vp]
    L.flo_lossy_pack_frames.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint8, C.c_float, vp, vp, vp, sz, vp, vp]
    L.flo_lossy_quantize_smr.argtypes = [vp, vp, vp, sz, C.c_uint32, C.c_float, vp, vp]
    L.flo_sparse_pack.argtypes = [vp, vp, sz, C.c_int, vp, sz, vp]
    L.flo_dist_unique_id.argtypes = [vp]
    L.flo_dist_create.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.flo_dist_destroy.argtypes = [vp]
    L.flo_dist_destroy.restype = None
    L.flo_dist_gather_submit.argtypes = [vp, vp]
    L.flo_dist_gather_flush.argtypes = [vp]
    L.flo_dist_gather_result.argtypes = [vp, C.POINTER(vp), C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint64))]
    L.flo_dist_stream.argtypes = [vp]
    L.flo_dist_stream.restype = vp
    L.flo_ctx_reserve_cus.argtypes = [vp, C.c_int]
    L.flo_ctx_reserve_cus.restype = C.c_int
    L.flo_batch_analysis_metadata.argtypes = [vp, sz, C.c_uint32, C.POINTER(vp), C.POINTER(sz)]
    L.flo_batch_clip_device_data.argtypes = [vp, sz]
    L.flo_batch_clip_device_data.restype = vp
    L.flo_batch_analyze_all.argtypes = [vp, C.c_uint32, vp, vp, sz, C.POINTER(C.c_uint64)]
    L.flo_batch_analysis_metadata_all.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.flo_batch_set_bit_depth.argtypes = [vp, C.c_uint8]
    L.flo_ctx_upload_path.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.flo_ctx_reserved_cus.argtypes = [vp]
    L.flo_ctx_reserved_cus.restype = C.c_int
    L.flo_dist_table_submit.argtypes = [vp, vp, C.c_size_t]
    L.flo_dist_table_flush.argtypes = [vp]
    L.flo_dist_table_result.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    u32p = C.POINTER(C.c_uint32)
    L.flo_stream_create.argtypes = [vp, C.c_uint32, C.c_uint8, C.c_uint8, C.c_uint8, C.POINTER(vp)]
    L.flo_stream_destroy.argtypes = [vp]
    L.flo_stream_destroy.restype = None
    L.flo_stream_push.argtypes = [vp, vp, sz]
    L.flo_stream_pending_samples.argtypes = [vp]
    L.flo_stream_pending_samples.restype = sz
    L.flo_stream_pending_frames.argtypes = [vp]
    L.flo_stream_pending_frames.restype = sz
    L.flo_stream_next_frame.argtypes = [vp, u32p, u32p, u32p, C.POINTER(vp), C.POINTER(sz)]
    L.flo_stream_flush.argtypes = L.flo_stream_next_frame.argtypes
    L.flo_stream_finalize.argtypes = [vp, C.c_char_p, sz, C.POINTER(vp), C.POINTER(sz)]
    L.flo_stream_create_lossy.argtypes = [vp, C.c_uint32, C.c_uint8, C.c_float, C.POINTER(vp)]
    L.flo_stream_append.argtypes = [vp, vp, sz]
    L.flo_stream_encode_ready.argtypes = [vp, sz, vp, vp]
    L.flo_analyze.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint8, C.c_uint32, vp, sz, C.POINTER(Analysis)]
    L.flo_analysis_metadata.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint8, C.c_uint32, C.POINTER(vp), C.POINTER(sz)]
    L.flo_decode.argtypes = [vp, C.c_char_p, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]
    L.flo_decode_lossless_i32.argtypes = L.flo_decode.argtypes
    L.flo_probe_container.argtypes = [C.c_char_p, sz, C.POINTER(ContainerInfo), C.c_char_p, sz]
    L.flo_get_toc.argtypes = [C.c_char_p, sz, C.POINTER(C.POINTER(TocEntryC)), C.POINTER(sz), C.c_char_p, sz]
    L.flo_seek_to_time.argtypes = [C.c_char_p, sz, C.c_uint32, C.POINTER(SeekResultC), C.c_char_p, sz]
    L.flo_decode_frame_at.argtypes = [vp, C.c_char_p, sz, C.c_uint32, C.POINTER(vp), C.POINTER(sz)]
    L.flo_corpus_create.argtypes = [vp, sz, C.POINTER(C.c_char_p), C.POINTER(sz), C.POINTER(vp)]
    L.flo_corpus_destroy.argtypes = [vp]
    L.flo_corpus_destroy.restype = None
    L.flo_corpus_format.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]
    L.flo_corpus_file_frames.argtypes = [vp, sz, C.POINTER(C.c_uint64)]
    L.flo_corpus_decode_windows.argtypes = [vp, sz, vp, vp, C.c_uint32, vp, sz, vp]
    L.flo_corpus_sync.argtypes = [vp]
    L.flo_sdec_create.argtypes = [vp, C.POINTER(vp)]
    L.flo_sdec_destroy.argtypes = [vp]
    L.flo_sdec_destroy.restype = None
    L.flo_sdec_attach.argtypes = [vp, vp]
    L.flo_sdec_last_error.argtypes = [vp]
    L.flo_sdec_last_error.restype = C.c_char_p
    L.flo_sdec_feed.argtypes = [vp, C.c_char_p, sz, C.POINTER(C.c_int)]
    L.flo_sdec_state.argtypes = [vp]
    L.flo_sdec_info.argtypes = [vp, C.POINTER(SdecInfoC)]
    for f in ("flo_sdec_frames_available", "flo_sdec_available_frames", "flo_sdec_current_frame_index", "flo_sdec_buffered_bytes"):
        getattr(L, f).argtypes = [vp]
        getattr(L, f).restype = sz
    L.flo_sdec_next_frame.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    L.flo_sdec_decode_available.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    L.flo_sdec_reset.argtypes = [vp]
    L.flo_sdec_reset.restype = None
    L.flo_sdec_decode_ready.argtypes = [vp, sz, vp, C.c_uint32, vp, sz, vp, vp, vp]
    fpp = C.POINTER(Fingerprint)
    L.flo_spectral_similarity.argtypes = [fpp, fpp]
    L.flo_spectral_similarity.restype = C.c_float
    L.flo_fpindex_create.argtypes = [vp, vp, sz, C.POINTER(vp)]
    L.flo_fpindex_destroy.argtypes = [vp]
    L.flo_fpindex_destroy.restype = None
    L.flo_fpindex_topk.argtypes = [vp, vp, sz, C.c_uint32, vp, vp]
    L.flo_fpindex_topk_self.argtypes = [vp, C.c_uint32, vp, vp]
    L.flo_fpindex_pairs.argtypes = [vp, C.c_float, C.c_uint64, vp, vp, vp, C.POINTER(C.c_uint64)]
    L.flo_batch_fidelity.argtypes = [vp, vp, vp, sz, vp]
    L.flo_compare.argtypes = [vp, vp, sz, C.c_char_p, sz, vp, vp, sz, C.POINTER(sz)]
    L.flo_batch_size_curve.argtypes = [vp, sz, vp, vp]
    L.flo_batch_set_quality.argtypes = [vp, C.c_float]
    L.flo_rate_pick.argtypes = [sz, vp, vp, C.c_uint64, u32p, C.POINTER(C.c_int)]
    L.flo_encode_batch_to_size.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(sz), C.c_uint32, C.c_uint8, sz, vp, vp, C.POINTER(vp),
                                           C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), vp, vp]
    L.flo_batch_encode_ladder.argtypes = [vp, sz, vp, C.POINTER(vp)]
    L.flo_ladder_shape.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]
    L.flo_ladder_file_bytes.argtypes = [vp, vp]
    L.flo_ladder_fetch.argtypes = [vp, sz, sz, C.c_char_p, sz, C.POINTER(vp), C.POINTER(sz)]
    L.flo_ladder_device_files.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint64))]
    L.flo_ladder_destroy.argtypes = [vp]
    L.flo_ladder_destroy.restype = None
    L.flo_encode_batch_ladder.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(sz), C.c_uint32, C.c_uint8, sz, vp, C.POINTER(vp),
                                          C.POINTER(sz), C.POINTER(vp), C.POINTER(sz)]
    L.flo_resample_filter.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(ResampleInfo), C.POINTER(vp), C.c_char_p, sz]
    L.flo_resample_out_frames.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]
    L.flo_batch_resample.argtypes = [vp, C.c_uint32, C.POINTER(vp)]
    L.flo_resample.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint32, C.c_uint8, C.POINTER(vp), C.POINTER(sz)]
    L.flo_batch_true_peak.argtypes = [vp, vp]
    L.flo_normalize_gain.argtypes = [C.c_double, C.c_double, C.c_float, C.POINTER(NormalizeOpts), C.POINTER(NormalizeReport), C.c_char_p, sz]
    L.flo_normalize_lookahead.argtypes = [C.c_uint32, C.POINTER(NormalizeOpts), C.POINTER(C.c_uint32), C.c_char_p, sz]
    L.flo_batch_normalize.argtypes = [vp, C.POINTER(NormalizeOpts), C.POINTER(vp), C.POINTER(NormalizeReport)]
    L.flo_normalize.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint8, C.POINTER(NormalizeOpts), C.POINTER(vp), C.POINTER(NormalizeReport)]
    L.flo_batch_edit.argtypes = [vp, sz, C.POINTER(EditSegment), C.c_uint8, vp, C.POINTER(vp)]
    L.flo_batch_active_range.argtypes = [vp, C.c_float, vp, vp]
    L.flo_edit.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint8, C.POINTER(EditSegment), C.c_uint8, vp, C.POINTER(vp), C.POINTER(sz)]
    L.flo_edit_tile_frames.argtypes = [C.c_uint8, C.c_uint8, C.POINTER(C.c_uint32)]
    L.flo_batch_mix.argtypes = [C.POINTER(vp), sz, sz, C.POINTER(C.c_uint64), sz, C.POINTER(MixPart), C.POINTER(vp)]
    L.flo_mix.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(sz), C.c_uint32, C.c_uint8, sz, C.POINTER(MixPart), C.c_uint64, C.POINTER(vp), C.POINTER(sz)]
    L.flo_batch_convolve.argtypes = [vp, vp, sz, C.POINTER(ConvJob), C.POINTER(vp)]
    L.flo_convolve.argtypes = [vp, vp, sz, vp, sz, C.c_uint32, C.c_uint8, C.c_uint8, C.POINTER(ConvJob), C.POINTER(vp), C.POINTER(sz)]
    L.flo_conv_geometry.argtypes = [C.c_uint8, C.c_uint8, C.POINTER(ConvInfo)]
    L.flo_batch_convolve_fft.argtypes = L.flo_batch_convolve.argtypes
    L.flo_convolve_fft.argtypes = L.flo_convolve.argtypes
    L.flo_conv_fft_geometry.argtypes = [C.c_uint8, C.c_uint8, C.POINTER(ConvFftInfo)]
    L.flo_fir_design.argtypes = [C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_uint32, C.c_double, C.POINTER(vp), C.c_char_p, sz]
    _LIB = L
    return L
