"""flo_amd — MI355X-native batch encoder for the .flo audio format (libflo's per-frame encode hot path).

The compute path is flo_amd/libflo_hip.so (hand-written gfx950 HIP kernels behind the C ABI in include/flo_hip.h);
this package is only the host-side mirror of the reference's encoder interface.
"""
from ._native import FloError, MODE_LOSSLESS, MODE_LOSSY  # noqa: F401
from .api import (Batch, Context, Decoder, EncodedFrame, Encoder, LossyEncoder, QualityPreset, StreamingEncoder,  # noqa: F401
                  TransformEncoder, default_context, decode, encode, encode_lossy, encode_with_bitrate, probe_container)
from .api import Corpus, SeekResult, TocEntry, decode_frame_at, get_toc, seek_to_time  # noqa: F401
from .api import DecoderState, StreamingAudioInfo, StreamingDecoder, decode_streams  # noqa: F401
from .api import EncodeStreamsResult, LossyStreamingEncoder, encode_streams  # noqa: F401
from .api import encode_lossy_many, encode_many, encode_with_bitrate_many  # noqa: F401
from .api import DEFAULT_RATE_GRID, encode_to_bitrate, encode_to_bitrate_many, rate_pick, size_curve  # noqa: F401
from .api import Ladder, encode_ladder, encode_ladder_many  # noqa: F401
from .api import resample, resample_filter, resample_many, resample_out_frames  # noqa: F401
from .api import normalize, normalize_gain, normalize_lookahead, normalize_many, true_peak  # noqa: F401
from .api import (active_range, active_range_many, edit, edit_many, edit_tile_frames, remix, remix_many, trim_silence,  # noqa: F401
                  trim_silence_many)
from .api import concat, concat_parts, mix  # noqa: F401
from .api import conv_geometry, conv_mode, convolve, fir_design, fir_filter  # noqa: F401
from .api import conv_fft_geometry  # noqa: F401
from .api import (FINGERPRINT_DTYPE, FingerprintIndex, extract_dominant_frequencies, fingerprint_array,  # noqa: F401
                  fingerprints_from_files, spectral_similarity)
from .api import FIDELITY_BLOCK_DTYPE, FIDELITY_DTYPE, compare, fidelity_dict  # noqa: F401
from .api import debug_delay_enqueue, debug_pool_fill, debug_stream_delay, debug_stream_delays  # noqa: F401
