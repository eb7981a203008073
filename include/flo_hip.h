/*
 * flo_hip.h — C ABI of the MI355X-native flo encoder (libflo_hip.so).
 *
 * Drop-in boundary for libflo's per-clip encode path. Every entry point is `extern "C"`, takes plain
 * pointers and sizes, and replaces one reference interface (cited as file:line under /root/reference):
 *
 *   flo_encode_lossy      <- lossy::TransformEncoder::new(sr,ch,q).encode_to_flo(samples, meta)
 *                            libflo/src/lossy/encoder.rs:36-53,167-239 (re-exported as LossyEncoder, lib.rs:21-24)
 *   flo_encode_lossless   <- lossless::Encoder::new(sr,ch,bits).with_compression(level).encode(samples, meta)
 *                            libflo/src/lossless/encoder.rs:17-45
 *   flo_encode_batch      <- the same two calls, once per clip (callers loop in reflo/src/lib.rs:286-306)
 *   flo_decode            <- libflo::decode(data) / lossless::Decoder::new().decode(data)
 *                            libflo/src/lib.rs:296-352, lossless/decoder.rs:14-72, lossy/decoder.rs:29-188
 *   flo_free              <- drop of the returned Vec<u8> / Vec<f32>
 *   error codes + flo_last_error <- FloResult<T> = Result<T, String>   (core/types.rs:281)
 *   flo_batch_fidelity / flo_compare <- no counterpart: the "compare original vs encoded" of the reference's TODO,
 *                            decoded audio against its source measured on the device (fidelity reports, below)
 *   flo_batch_size_curve / flo_encode_batch_to_size <- no counterpart: where QualityPreset::from_bitrate (lossy/mod.rs) maps a
 *                            bitrate to a preset, the file size at every candidate quality measured in one device pass
 *
 * Conventions mirror the reference: inputs are interleaved f32 PCM in [-1,1], length
 * n_interleaved = sample_frames * channels (a trailing partial sample-frame is ignored, as the reference's
 * integer division does); metadata is an opaque byte string appended verbatim as the META chunk; the output
 * is one malloc'ed buffer holding a complete .flo file, released with flo_free. One flo_ctx per host
 * thread / GPU; contexts are independent. A "fresh encoder per clip" is the contract for lossy encodes
 * (the reference never resets the psychoacoustic state between calls; all its callers build a new encoder).
 *
 * Sample rates: any rate the reference accepts (tested 8 kHz .. 384 kHz for lossy encode and decode, 8 .. 192 kHz
 * lossless); channels: 1 .. 8 lossy, 1 .. 255 lossless.
 *
 * There is NO CPU fallback: every encode and decode entry point runs the HIP kernels on the context's device and
 * fails with a non-zero code if no gfx950 device is usable.
 */
#ifndef FLO_HIP_H
#define FLO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLO_OK 0
#define FLO_ERR_ARG 1      /* invalid argument */
#define FLO_ERR_DEVICE 2   /* HIP runtime / device error (text in flo_last_error) */
#define FLO_ERR_NOMEM 3
#define FLO_ERR_STATE 4    /* call sequence error on a batch object */
#define FLO_ERR_FORMAT 5   /* not a decodable .flo file; flo_last_error holds the reference reader's message */

#define FLO_MODE_LOSSLESS 0
#define FLO_MODE_LOSSY 1

typedef struct flo_ctx flo_ctx; /* owns device id, stream, constant tables, scratch */

int flo_ctx_create(int device, flo_ctx **out);
void flo_ctx_destroy(flo_ctx *ctx);
const char *flo_last_error(const flo_ctx *ctx); /* message of the last failing call on this ctx */
/* message of the last failing flo_ctx_create (no ctx exists yet to hold it) */
const char *flo_last_create_error(void);
void flo_free(void *p);
/* device facts for reports: name, CU count, total HBM bytes */
int flo_ctx_device_info(const flo_ctx *ctx, char *name, size_t name_cap, int *compute_units, uint64_t *hbm_bytes);

/* ---- one clip in, one .flo file out (host buffers; includes H2D/D2H) ------------------------------- */
int flo_encode_lossy(flo_ctx *ctx, const float *pcm, size_t n_interleaved, uint32_t sample_rate, uint8_t channels,
                     float quality, const uint8_t *meta, size_t meta_len, uint8_t **out, size_t *out_len);
int flo_encode_lossless(flo_ctx *ctx, const float *pcm, size_t n_interleaved, uint32_t sample_rate,
                        uint8_t channels, uint8_t bit_depth, uint8_t level, const uint8_t *meta, size_t meta_len,
                        uint8_t **out, size_t *out_len);
/* many clips in one launch sequence; outs[i]/out_lens[i] receive one malloc'ed .flo per clip */
int flo_encode_batch(flo_ctx *ctx, int mode, size_t n_clips, const float *const *pcm, const size_t *n_interleaved,
                     uint32_t sample_rate, uint8_t channels, float quality_or_level, uint8_t **outs,
                     size_t *out_lens);

/* ---- one .flo file in, interleaved f32 PCM out (host buffers) ---------------------------------------------
 * Replaces libflo::decode (lib.rs:296-315): files with a transform frame go through the device inverse MDCT
 * (first frame dropped as the reference does: (frames - 1) * 1024 sample-frames come back), all others through the
 * device Rice / predictor kernels (bit-exact integers, then * 1/32767). The container is parsed on the host like
 * Reader::read (reader.rs:16-256): its error strings come back through flo_last_error with FLO_ERR_FORMAT. Like the
 * reference, the CRC is not verified by decode. *pcm is malloc'ed (flo_free); sample_rate / channels may be NULL. */
int flo_decode(flo_ctx *ctx, const uint8_t *flo, size_t len, float **pcm, size_t *n_interleaved,
               uint32_t *sample_rate, uint8_t *channels);
/* the integers before the float conversion (lossless files only): what parity tests compare bit for bit */
int flo_decode_lossless_i32(flo_ctx *ctx, const uint8_t *flo, size_t len, int32_t **pcm, size_t *n_interleaved,
                            uint32_t *sample_rate, uint8_t *channels);

/* What the container reader (Reader::read, reader.rs:16-256) extracts from a file, without touching the device: the
 * host half of flo_decode on its own. Returns FLO_OK or FLO_ERR_FORMAT with the reader's message in err (may be NULL,
 * err_cap bytes). No context needed. */
typedef struct flo_container_info {
    uint8_t version_major, version_minor, channels, bit_depth;
    uint8_t compression_level, is_transform, pad0, pad1;
    uint16_t flags, pad2;
    uint32_t sample_rate;
    uint32_t data_crc32;
    uint32_t n_frames;          /* frames the reader accepted */
    uint64_t total_samples;     /* header field */
    uint64_t data_start, data_size;
    uint64_t frame_samples_sum; /* sum of frame_samples over the frames read */
} flo_container_info;
int flo_probe_container(const uint8_t *flo, size_t len, flo_container_info *out, char *err, size_t err_cap);

/* ---- seeking: libflo/src/seeking.rs (wasm exports get_toc / decode_frame_at / seek_to_time, lib.rs:478-530) ----------
 * The reference's semantics, quirks included. A lossy file's TOC stamps frame i at i * 1024 / sample_rate ms, but frame i
 * decodes input samples [(i - 1) * 1024, i * 1024): the encoder's first frame is pre-roll that flo_decode drops. So
 * seek_to_time answers in the TOC's time base and decode_frame_at(i) is output block i - 1 of flo_decode (frame 0: the
 * pre-roll block flo_decode never returns). The corpus window decode below counts in flo_decode's samples instead. */
typedef struct flo_toc_entry {   /* core/types.rs:174-179 */
    uint32_t frame_index;
    uint32_t frame_size;
    uint64_t byte_offset;
    uint32_t timestamp_ms;
    uint32_t pad;
} flo_toc_entry;
typedef struct flo_seek_result {   /* seeking.rs:7-19 */
    uint32_t frame_index;
    uint32_t timestamp_ms;
    uint64_t byte_offset;
    uint32_t sample_offset;
    uint32_t next_timestamp_ms;
} flo_seek_result;
/* get_toc (seeking.rs:28-32): every TOC entry exactly as Reader::read returns it (reader.rs:76-100); *entries is malloc'ed
 * (flo_free; NULL when *n = 0). FLO_ERR_FORMAT with the reader's message in err. No context needed. */
int flo_get_toc(const uint8_t *flo, size_t len, flo_toc_entry **entries, size_t *n, char *err, size_t err_cap);
/* seek_to_time (seeking.rs:75-132, 136-159): the rightmost entry with timestamp_ms <= target_ms, clamped to the last frame
 * read; sample_offset into that frame; next_timestamp_ms (for the last frame: its timestamp + frame_samples * 1000 /
 * sample_rate). "No TOC available for seeking" for an empty TOC. Where the reference would panic (TOC entries but no
 * frames read, a zero sample rate) FLO_ERR_FORMAT; u32 differences wrap as in a release build. No context needed. */
int flo_seek_to_time(const uint8_t *flo, size_t len, uint32_t target_ms, flo_seek_result *out, char *err, size_t err_cap);
/* decode_frame_at (seeking.rs:43-63, 161-207): the interleaved f32 samples of one frame (*pcm malloc'ed, flo_free).
 * A lossless frame goes through the device lossless path on its own (frame_samples * channels floats). A transform frame
 * is the overlap-add of its first half with the second half of the last earlier frame that carries channels - zeros if
 * there is none - on the device, with flo_decode's kernel: 1024 * channels floats, for i >= 1 of an encoder-made file
 * bit for bit flo_decode(file)[(i - 1) * 1024 * ch .. i * 1024 * ch]. (The reference gets the same overlap by decoding
 * every earlier frame.) Errors as the reference's: "Frame index i out of bounds (total frames: n)", "Failed to deserialize
 * transform frame" - also when the earlier frame it overlaps with cannot be deserialised, where the reference skips it. */
int flo_decode_frame_at(flo_ctx *ctx, const uint8_t *flo, size_t len, uint32_t frame_index, float **pcm,
                        size_t *n_interleaved);

/* ---- corpus: many files resident in HBM, many short windows decoded at once -------------------------------------------
 * flo_corpus_create parses every file on the host once (reader errors come back as FLO_ERR_FORMAT with the reader's
 * message), uploads all bytes once and builds the per-file frame tables once. All files must share one sample rate and
 * one channel count (FLO_ERR_ARG otherwise); lossy and lossless files may be mixed. files[i] may be freed afterwards.
 *
 * flo_corpus_decode_windows: window w is (file[w], start[w]) in sample-frames of what flo_decode returns for that file;
 * its window_frames * channels interleaved floats go to dst_device + w * window_frames * channels and equal
 * flo_decode(file)[start * ch .. (start + window_frames) * ch] bit for bit, zeros past the end of the file. The call only
 * enqueues: the work runs on the ctx stream, ordered by events after what is queued on `stream` (a hipStream_t: NULL is
 * the null stream - torch's default stream - and flo_ctx_stream(ctx) orders against nothing else), and later work on
 * `stream` sees the result. Host work is O(windows + lossless frames touched); scratch grows to the largest call and is
 * kept. A frame touched by two windows of one call is decoded twice (once per window: no cross-window bookkeeping).
 * A lossy frame that cannot be deserialised sets an error word: flo_corpus_sync waits for the ctx stream and returns
 * FLO_ERR_FORMAT with flo_decode's message ("Failed to deserialize transform frame"), then clears the word. */
typedef struct flo_corpus flo_corpus;
int flo_corpus_create(flo_ctx *ctx, size_t n_files, const uint8_t *const *files, const size_t *lens, flo_corpus **out);
void flo_corpus_destroy(flo_corpus *c);
int flo_corpus_format(const flo_corpus *c, uint32_t *sample_rate, uint8_t *channels);
/* flo_decode's length of file `file` in sample-frames */
int flo_corpus_file_frames(const flo_corpus *c, size_t file, uint64_t *decoded_sample_frames);
int flo_corpus_decode_windows(flo_corpus *c, size_t n_windows, const uint32_t *file, const uint64_t *start,
                              uint32_t window_frames, float *dst_device, size_t dst_cap_floats, void *stream);
int flo_corpus_sync(flo_corpus *c);

/* ---- streaming decoder: StreamingDecoder of libflo/src/streaming/decoder.rs (WasmStreamingDecoder, lib.rs:545-681) -----
 * Bytes of one .flo file are fed in chunks as they arrive; each frame's samples come out once the frame is complete. The
 * state machine, the counters and the frame parser are the reference's, quirks included:
 *   - the header is read from a fixed 70 bytes; bad magic is the only thing that enters FLO_SDEC_ERROR (feed returns
 *     FLO_ERR_FORMAT then, "Invalid flo file: bad magic"); the TOC starts at 70, the frames at 70 + toc_size
 *     (header_size is ignored); a TOC shorter than its entry count leaves the entries read pushed, and the next feed
 *     pushes them again;
 *   - feed in FLO_SDEC_ERROR or FLO_SDEC_FINISHED drops the data (*new_frames = 0);
 *   - a frame is complete when its TOC end lies inside the buffer; counting stops at the first incomplete frame;
 *   - next_frame moves to FLO_SDEC_FINISHED once current_frame >= the TOC's length; a frame that does not parse
 *     ("Frame too small", "Frame truncated", "Channel data truncated", "Invalid LPC order", "ALPC channel too small",
 *     "Missing rice parameter") fails without advancing, so it fails again on the next call;
 *   - lossy: the first transform frame that deserialises is the pre-roll: an empty frame that primes the overlap; a
 *     frame that does not deserialise is an empty frame, consumed, no pre-roll, the overlap untouched;
 *   - decode_available decodes the whole buffer from frame 0 like the file reader (its errors leave the state as it was;
 *     on success the state is FLO_SDEC_FINISHED); it equals flo_decode except that a lossy frame that does not
 *     deserialise is skipped (flo_decode fails on it).
 * What the device decoder does not take comes back as FLO_ERR_FORMAT without advancing, like a parse error: transform
 * blocks other than Long, a transform frame with more channels than the stream, an ALPC wrapper with coefficients and
 * a non-Rice encoding byte (no encoder writes one), a frame of more than 2 000 000 samples, and a stream that mixes
 * transform frames with other frames (kind chosen by the header's lossy flag).
 *
 * A decoder without a context (ctx NULL) parses and counts; next_frame / decode_available return FLO_ERR_STATE until
 * flo_sdec_attach gives it one (flo_sdec_decode_ready attaches its context itself).
 * next_frame returns 1 with one frame in *pcm (malloc'ed, flo_free; NULL and *n = 0 for an empty frame), 0 when no
 * frame is ready, or a negated FLO_ERR_* code (-FLO_ERR_FORMAT for the errors above). flo_sdec_last_error(d) holds the
 * decoder's last message.
 *
 * flo_sdec_decode_ready: for each decoder, every complete frame that next_frame has not returned yet (at most
 * max_frames_per_stream of them, 0: all) is decoded into dst_device[offsets[i] .. offsets[i + 1]): bit for bit the
 * concatenation of what as many next_frame calls return, and the decoder's counters advance to match (a decoder with
 * nothing left to decode moves to FLO_SDEC_FINISHED, as a next_frame call would). offsets ([n + 1] floats) and status
 * ([n]: FLO_OK, or the error the decoder's next next_frame reports, message in flo_sdec_last_error) are filled before
 * the call returns; the decode is enqueued on the ctx stream, ordered after what is queued on `stream` and before its
 * later work (as flo_corpus_decode_windows). Decoders not yet ready contribute nothing. All decoders that decode in one
 * call share one sample rate and channel count (FLO_ERR_ARG otherwise); lossy and lossless streams may be mixed. A
 * lossy stream's overlap stays on the device between calls: each frame is decoded once, except one frame re-decoded
 * at every 16-frame run boundary inside a call. Per call only the payload bytes of the frames decoded are uploaded.
 * dst_device NULL: sizing only - offsets and status are filled, nothing is decoded and no decoder changes; the next call
 * on the same context over the same decoders and cap, none of them changed in between, reuses that plan. */
#define FLO_SDEC_WAITING_HEADER 0
#define FLO_SDEC_WAITING_TOC 1
#define FLO_SDEC_READY 2
#define FLO_SDEC_FINISHED 3
#define FLO_SDEC_ERROR 4
typedef struct flo_sdec flo_sdec;
typedef struct flo_sdec_audio_info {   /* StreamingAudioInfo, streaming/types.rs */
    uint32_t sample_rate;
    uint8_t channels, bit_depth, is_lossy, pad;
    uint64_t total_samples;
} flo_sdec_audio_info;
int flo_sdec_create(flo_ctx *ctx /* may be NULL: parse only */, flo_sdec **out);
void flo_sdec_destroy(flo_sdec *d);
int flo_sdec_attach(flo_sdec *d, flo_ctx *ctx);   /* FLO_ERR_STATE if it already has another context */
const char *flo_sdec_last_error(const flo_sdec *d);
int flo_sdec_feed(flo_sdec *d, const uint8_t *data, size_t len, int *new_frames);
int flo_sdec_state(const flo_sdec *d);
int flo_sdec_info(const flo_sdec *d, flo_sdec_audio_info *out);   /* FLO_ERR_STATE before the header */
size_t flo_sdec_frames_available(const flo_sdec *d);      /* complete frames, NOT minus the current one (decoder.rs:63-68) */
size_t flo_sdec_available_frames(const flo_sdec *d);      /* complete frames minus the current one (:143-149) */
size_t flo_sdec_current_frame_index(const flo_sdec *d);
size_t flo_sdec_buffered_bytes(const flo_sdec *d);
int flo_sdec_next_frame(flo_sdec *d, float **pcm, size_t *n);
int flo_sdec_decode_available(flo_sdec *d, float **pcm, size_t *n);
void flo_sdec_reset(flo_sdec *d);
int flo_sdec_decode_ready(flo_ctx *ctx, size_t n, flo_sdec *const *decs, uint32_t max_frames_per_stream, float *dst_device,
                          size_t dst_cap_floats, uint64_t *offsets, int *status, void *stream);

/* ---- device-resident batch (the throughput path: PCM already in HBM, bitstreams left in HBM) -------- */
typedef struct flo_batch flo_batch;

/* Plan a batch: clip i has n_interleaved[i] samples. Allocates the HBM input buffer (clips back to back,
 * each start 16-byte aligned), the output bitstream buffer and scratch. mode = FLO_MODE_LOSSY/LOSSLESS. */
int flo_batch_create(flo_ctx *ctx, int mode, size_t n_clips, const size_t *n_interleaved, uint32_t sample_rate,
                     uint8_t channels, float quality_or_level, flo_batch **out);
void flo_batch_destroy(flo_batch *b);
/* device pointer to clip i's interleaved f32 PCM (n_interleaved[i] floats) — fill it however you like */
float *flo_batch_clip_device_ptr(flo_batch *b, size_t clip);
/* the same address, for reading the clip as it sits in the batch. flo_batch_clip_device_ptr is taken to mean that the
 * caller writes the clip (a lossy clip's kept trailing samples are then dropped, see flo_batch_analyze_all); this is not */
const float *flo_batch_clip_device_data(const flo_batch *b, size_t clip);
/* H2D copy of one clip */
int flo_batch_upload(flo_batch *b, size_t clip, const float *pcm);
/* fill every clip with the integer-exact synthetic signal of flo_synth.h (device kernel), seeded by seed;
 * clip ids start at clip_id0 so that ranks of a sharded job generate disjoint parts of one corpus */
int flo_batch_fill_synthetic(flo_batch *b, uint32_t seed, uint64_t clip_id0);
/* launch the encode kernels on the ctx stream (asynchronous). which = 0: auto, 1: clip-chain kernel with one wave
 * per channel, 2: frame-parallel kernels, 5: clip-chain kernel with one transform wave that carries both channels in
 * lock-step (packed f32 arithmetic) + one quantiser-and-packer wave per stereo clip, persistent workgroups that deal
 * the clips dynamically: the form auto picks for stereo batches; 3 and 4 (stereo chain forms of earlier rounds,
 * retired) mean 5 (lossy only; all forms produce identical bytes, a masking level of +inf - a band energy that overflows
 * f32 - included: the frame-parallel form records where one first occurs; 5 falls back to 1 for mono) */
int flo_batch_encode(flo_batch *b, int which);
int flo_batch_sync(flo_batch *b);
/* after sync: total compressed DATA bytes of the batch, and of one clip */
int flo_batch_data_bytes(flo_batch *b, uint64_t *total);
/* D2H + container assembly (header, TOC, CRC32, META) of one clip -> malloc'ed .flo */
int flo_batch_fetch(flo_batch *b, size_t clip, const uint8_t *meta, size_t meta_len, uint8_t **out,
                    size_t *out_len);
/* device address and size of the packed per-clip DATA chunks, for a zero-copy hand-off (e.g. an RCCL gather):
 * clip i's DATA chunk is at base + offsets[i], sizes[i] bytes (both arrays host-side, n_clips entries) */
int flo_batch_device_streams(flo_batch *b, const uint8_t **base, const uint64_t **offsets, const uint64_t **sizes);

/* pack every clip's DATA chunk back to back (16-byte aligned offsets) into a caller-owned device buffer on the ctx
 * stream: the single contiguous payload a rank contributes to the RCCL gather. offsets has n_clips + 1 entries. */
int flo_batch_pack_streams(flo_batch *b, void *dst_device, size_t dst_cap, uint64_t *offsets);
/* The same for FINISHED FILES: after flo_batch_sync every clip's header (version 1.2, CRC32 of DATA, sizes), TOC and
 * DATA sit contiguously in HBM — writer.rs:132-224 and core/crc32.rs done on the device — i.e. a complete .flo file
 * with an empty META chunk. device_files exposes them in place; pack_files copies them back to back (16-byte aligned
 * offsets) into caller-owned device memory: the payload of the multi-GPU gather. (bit_depth in the header is 16;
 * flo_batch_fetch / flo_encode_lossless patch the caller's value and the META size when they copy a file out.) */
int flo_batch_device_files(flo_batch *b, const uint8_t **base, const uint64_t **offsets, const uint64_t **sizes);
int flo_batch_pack_files(flo_batch *b, void *dst_device, size_t dst_cap, uint64_t *offsets);
/* after sync: decode every clip from its device bitstream into dst (device memory, dst_cap floats). Clip i's PCM —
 * exactly what flo_decode returns for its file: (frames_i - 1) * 1024 * channels floats for a lossy clip, the
 * clip's interleaved samples for a lossless one — starts at offsets[i] floats (host array, n_clips entries). The
 * payload never leaves HBM and nothing is parsed: frame and wrapper descriptions come from the batch's own encode
 * records. Full-size round-trip checks and the decode throughput figures. */
int flo_batch_decode(flo_batch *b, float *dst_device, size_t dst_cap_floats, uint64_t *offsets);

/* ---- multi-GPU: one process per GPU, one exchange step per batch -------------------------
 * Clips shard across ranks with no communication during the encode. The exchange step is the variable-size gather of
 * every rank's finished .flo files to the root, written directly against RCCL over xGMI: ncclAllGather of the packed
 * sizes, then grouped ncclSend / ncclRecv on a communication stream of the library's own, double-buffered so that the
 * transfer of step k overlaps the encode of step k + 1. (The reference has no counterpart: its callers encode clips one
 * after the other in one thread, reflo/src/lib.rs:286-306.)
 *   rank 0:   flo_dist_unique_id(id); share id with the other ranks by any side channel (file, socket, MPI, ...)
 *   all:      flo_dist_create(ctx, id, rank, world, root, &d);
 *   per step: flo_batch_encode(b, 0); flo_batch_sync(b); flo_dist_gather_submit(d, b);
 *   at the end: flo_dist_gather_flush(d);   root: flo_dist_gather_result(d, &base, &offs, &sizes)
 * gather_submit never waits on the host for the device: it packs the batch's files (device), all-gathers the packed
 * sizes into pinned host memory (asynchronous) and posts the point-to-point transfers of the PREVIOUS submit, whose
 * sizes arrived while this step was being encoded. */
typedef struct flo_dist flo_dist;
#define FLO_DIST_ID_BYTES 128
int flo_dist_unique_id(uint8_t *id /* FLO_DIST_ID_BYTES */);
int flo_dist_create(flo_ctx *ctx, const uint8_t *id, int rank, int world, int root, flo_dist **out);
void flo_dist_destroy(flo_dist *d);
int flo_dist_gather_submit(flo_dist *d, flo_batch *b);
int flo_dist_gather_flush(flo_dist *d);
/* root, after a flush: rank r's packed files (each a complete .flo file without META, starts 16-byte aligned, lengths
 * in their headers) lie at base + rank_offsets[r], rank_sizes[r] bytes, in device memory owned by d */
int flo_dist_gather_result(flo_dist *d, const uint8_t **base, const uint64_t **rank_offsets, const uint64_t **rank_sizes);
void *flo_dist_stream(flo_dist *d);   /* hipStream_t of the communication stream */
/* Second exchange mode, offered beside the gather (the gather is what the path's single exchange step is; this shows what
 * the encode scales to when the root's link ingress is not in the way): the files stay on the ranks that made them and
 * ONE ncclAllGather of 24 bytes per clip tells every rank where each file of every rank lies (byte offset in its
 * owner's device buffer), how long it is and the CRC32 of its DATA chunk. max_clips = the largest clip count of any
 * rank (the same value on all ranks). Asynchronous on the communication stream, double-buffered like the gather.
 *   per step: flo_batch_encode(b, 0); flo_batch_sync(b); flo_dist_table_submit(d, b, max_clips);
 *   at the end: flo_dist_table_flush(d);  every rank: flo_dist_table_result(d, &rows, &row_words, &max_clips)
 * rows = host memory owned by d, `world` rows of row_words u64: [0] the rank's clip count | [1 .. max] sizes |
 * [1 + max .. 2 max] offsets | [1 + 2 max .. 3 max] CRC32 values (of the last submitted step). */
int flo_dist_table_submit(flo_dist *d, flo_batch *b, size_t max_clips);
int flo_dist_table_flush(flo_dist *d);
int flo_dist_table_result(flo_dist *d, const uint64_t **rows, size_t *row_words, size_t *max_clips);
/* The persistent encode kernels start one workgroup per compute unit; RCCL's send / receive are kernels too, so with
 * more than one rank the library leaves `n` compute units free for them (default 8 once a communicator with world > 1
 * exists, 0 otherwise; the environment variable FLO_RESERVE_CUS sets it at context creation). Costs n / 256 of the
 * single-GPU rate; without it the transfer of step k cannot start before the encode of step k + 1 has ended. */
int flo_ctx_reserve_cus(flo_ctx *ctx, int n);
/* Host-buffer entry points (flo_encode_*): which path uploads beyond 8 MB take on this host - "pageable-direct" (the
 * runtime's copy straight from the caller's memory) or "pinned-ring" (copy threads + pinned staging) - and the rates the
 * one-time probe measured for both (GB/s; 0 and "not measured yet" before the first large upload). A single clip always
 * goes direct. FLO_UPLOAD_PATH=direct|ring overrides the probe. */
int flo_ctx_upload_path(flo_ctx *ctx, char *name, size_t name_cap, double *direct_gbs, double *ring_gbs);
/* compute units the persistent encode kernels currently leave free (0 when nothing is reserved). A reservation that
 * flo_dist_create made by default ends with flo_dist_destroy; one set by the caller or FLO_RESERVE_CUS stays. */
int flo_ctx_reserved_cus(flo_ctx *ctx);

/* ---- analysis metadata: what libflo::encode / encode_lossy / encode_with_bitrate add to META (lib.rs:219-283) -------
 * flo_analyze computes, on the device, what add_analysis_data_if_missing computes from the samples: waveform peaks
 * (core/analysis.rs:38-115), the spectral fingerprint (analysis.rs:223-357: BLAKE3 of the content, band energies and
 * peak bins of three 256-point FFT sections, average loudness) and the EBU R128 integrated loudness
 * (core/ebu_r128.rs:182-318). flo_analysis_metadata frames them as the MessagePack FloMetadata the reference serialises
 * for an empty input META (fields length_ms, waveform_data, spectrum_fingerprint, loudness_profile; malloc'ed, flo_free):
 * pass the result as `meta` to flo_encode_lossless / flo_encode_lossy to get what libflo::encode* return. */
typedef struct flo_analysis {
    uint32_t n_peaks;            /* waveform peaks written to `peaks` (normalised to the largest) */
    uint32_t duration_ms, sample_rate;
    uint8_t channels, avg_loudness, pad0, pad1;
    uint8_t hash[32];
    uint8_t frequency_peaks[8];
    uint8_t energy_profile[16];
    double integrated_lufs;
    uint64_t length_ms;
    /* the rest of compute_ebu_r128_loudness (ebu_r128.rs:182-355; not part of the META chunk, printed by the CLI's
     * `analysis` command like reflo's): range of the gated block loudness, the 49-tap "true peak", the sample peak */
    double loudness_range_lu, true_peak_dbtp, sample_peak_dbfs;
    /* the f32 accumulator avg_loudness is derived from (analysis.rs:338: the sequential sum of s * s over all samples),
     * bit for bit the reference's value at any length; exposed for the tests */
    float sum_squares;
    uint32_t pad2;
} flo_analysis;
int flo_analyze(flo_ctx *ctx, const float *pcm, size_t n_interleaved, uint32_t sample_rate, uint8_t channels,
                uint32_t peaks_per_second, float *peaks, size_t peaks_cap, flo_analysis *out);
int flo_analysis_metadata(flo_ctx *ctx, const float *pcm, size_t n_interleaved, uint32_t sample_rate, uint8_t channels,
                          uint32_t peaks_per_second, uint8_t **out, size_t *out_len);
/* the same for a clip that already sits in a batch (after flo_batch_upload): libflo::encode* analyse and encode the SAME
 * samples (lib.rs:105-116), so the free functions upload once, analyse on the device copy, then encode it:
 *   flo_batch_create(1 clip); flo_batch_upload; flo_batch_analysis_metadata -> META (merge with the caller's);
 *   flo_batch_set_bit_depth (lossless); flo_batch_encode; flo_batch_sync; flo_batch_fetch(meta) */
int flo_batch_analysis_metadata(flo_batch *b, size_t clip, uint32_t peaks_per_second, uint8_t **out, size_t *out_len);
/* the analysis of EVERY clip of a batch (after its uploads) in one device pass: a fixed number of launches per group of
 * clips, not per clip (groups keep the device scratch under FLO_BATCH_ANALYSIS_GROUP_BYTES, default 1 GiB, read per call).
 * out[n_clips]; the peaks concatenated, clip i's at peaks[peak_off[i] .. peak_off[i + 1]). With peaks == NULL only
 * peak_off (n_clips + 1 entries) is filled: the sizing call. Every field, peak and META byte equals what
 * flo_batch_analysis_metadata / flo_analyze give for a clip whose device copy holds all of the caller's samples.
 * Lossy clips of n_interleaved % channels != 0 uploaded through flo_batch_upload are analysed over ALL of the caller's
 * samples (the trailing partial sample-frame, which the encoder drops, is kept on the host for this), as libflo::encode_lossy
 * does; clips written through flo_batch_clip_device_ptr or flo_batch_fill_synthetic are analysed as the device holds them. */
int flo_batch_analyze_all(flo_batch *b, uint32_t peaks_per_second, flo_analysis *out, float *peaks, size_t peaks_cap,
                          uint64_t *peak_off);
/* the MessagePack META of every clip, concatenated in one malloc'ed buffer (flo_free): clip i's at off[i] .. off[i + 1] */
int flo_batch_analysis_metadata_all(flo_batch *b, uint32_t peaks_per_second, uint8_t **out, uint64_t *off);
/* the bit depth a lossless batch's files declare (16 unless set; flo_encode_lossless's argument) */
int flo_batch_set_bit_depth(flo_batch *b, uint8_t bit_depth);

/* ---- size curves and the rate-targeted lossy encode (no counterpart: the reference maps a bitrate to one of five presets
 * by the raw-PCM ratio, QualityPreset::from_bitrate, and never looks at the audio) ----------------------------------------
 * Quality enters TransformEncoder only through the keep threshold of quantize_coefficients (encoder.rs:130-151), so one
 * transform of the PCM prices every candidate quality: the sizes below are the exact lengths of the files an encode of
 * the batch at that quality produces, without running the packer.
 * flo_batch_size_curve: a lossy batch holding PCM (uploaded or filled; encoded or not): file_bytes[clip * n_q + j] = length
 *   of the finished file (empty META) an encode of this batch at qualities[j] produces: 74 + 20 frames + DATA. 1 <= n_q <= 32.
 *   Synchronous. The batch's own quality plays no part; the batch's encode state and results are untouched. The device
 *   scratch is taken per call and processed in groups of clips that stay under FLO_SIZE_CURVE_GROUP_BYTES (default 256 MiB,
 *   read per call). FLO_ERR_ARG for a lossless batch, n_q of 0 or above 32 and null pointers; FLO_ERR_STATE before any PCM
 *   was uploaded.
 * flo_batch_set_quality: re-point a lossy batch at another quality (the tables of (sample_rate, quality)); results of an
 *   earlier encode are dropped (encode + sync again).
 * flo_rate_pick: the candidate of the largest quality value (clamped like the encoder's: NaN -> 0, [0, 1]) whose size is
 *   <= budget; every candidate is looked at, sizes need not grow with quality; equal quality values: the lower index.
 *   *fits = 1. When none fits: the candidate of the smallest quality value, *fits = 0. No context needed.
 * flo_encode_batch_to_size: host buffers in, one finished .flo per clip out (malloc'ed, flo_free), each at the best
 *   candidate quality whose whole file (META included) fits target_bytes[i]; chosen[i] = candidate index, fits[i] as
 *   flo_rate_pick. meta / meta_lens may be NULL (both). One upload, one curve, then every clip is encoded once, at its
 *   chosen quality, in a batch per chosen candidate filled by device-to-device copies. Lossy only, 1 to 8 channels. */
int flo_batch_size_curve(flo_batch *b, size_t n_q, const float *qualities, uint64_t *file_bytes);
int flo_batch_set_quality(flo_batch *b, float quality);
int flo_rate_pick(size_t n_q, const float *qualities, const uint64_t *sizes, uint64_t budget, uint32_t *index, int *fits);
int flo_encode_batch_to_size(flo_ctx *ctx, size_t n_clips, const float *const *pcm, const size_t *n_interleaved,
                             uint32_t sample_rate, uint8_t channels, size_t n_q, const float *qualities,
                             const uint64_t *target_bytes, const uint8_t *const *meta, const size_t *meta_lens,
                             uint8_t **outs, size_t *out_lens, uint32_t *chosen, int *fits);

/* ---- quality ladders: every clip of a lossy batch as a finished file at each of K qualities, from ONE transform pass -------
 * The identity behind the size curve, taken to the bytes: window, MDCT, band statistics, masking chain, scale factors and
 * round(c * sf) do not depend on quality, so a frame at quality q_j is the same integers under another keep mask, packed
 * again. Rung j of clip i is, byte for byte, the file flo_encode_lossy makes of that clip at qualities[j].
 * flo_batch_encode_ladder: a lossy batch holding PCM (uploaded or filled; encoded or not); 1 <= n_q <= 32; duplicate and
 *   unordered qualities are allowed, every rung is a file of its own. Synchronous: the ladder is complete on return. The
 *   batch's own quality plays no part and its encode state and results are untouched. Device scratch is taken per call
 *   and the clips are processed in groups that stay under FLO_LADDER_GROUP_BYTES (default 4 GiB, read per call; a clip
 *   larger than the limit is a group of its own; one host synchronisation per group). Afterwards only the finished files
 *   stay resident: their exact bytes, each at a 16-byte aligned offset of one allocation. FLO_ERR_ARG for a lossless
 *   batch, n_q of 0 or above 32 and null pointers; FLO_ERR_STATE before any PCM was uploaded; the context stays usable.
 * A ladder holds its own device memory and nothing of the batch: it may outlive the batch it was made from. It must be
 *   destroyed before its context.
 * flo_ladder_file_bytes: file_bytes[clip * n_q + j], the length without META (what flo_batch_size_curve returns).
 * flo_ladder_fetch: the file of (clip, rung), malloc'ed (flo_free), META appended and meta_size patched as flo_batch_fetch.
 * flo_ladder_device_files: the files of one rung as they sit in HBM (no META): clip i at base + offsets[i] (multiples of
 *   16), sizes[i] bytes; the arrays belong to the ladder.
 * flo_encode_batch_ladder: host buffers in, n_clips * n_q finished files out (outs[clip * n_q + j], malloc'ed, flo_free);
 *   clip i's META goes behind each of its rungs; meta / meta_lens may be NULL (both). One upload, one ladder. */
typedef struct flo_ladder flo_ladder;
int flo_batch_encode_ladder(flo_batch *b, size_t n_q, const float *qualities, flo_ladder **out);
int flo_ladder_shape(const flo_ladder *l, size_t *n_clips, size_t *n_q);
int flo_ladder_file_bytes(const flo_ladder *l, uint64_t *file_bytes);
int flo_ladder_fetch(flo_ladder *l, size_t clip, size_t rung, const uint8_t *meta, size_t meta_len, uint8_t **out, size_t *out_len);
int flo_ladder_device_files(flo_ladder *l, size_t rung, const uint8_t **base, const uint64_t **offsets, const uint64_t **sizes);
void flo_ladder_destroy(flo_ladder *l);
int flo_encode_batch_ladder(flo_ctx *ctx, size_t n_clips, const float *const *pcm, const size_t *n_interleaved,
                            uint32_t sample_rate, uint8_t channels, size_t n_q, const float *qualities,
                            const uint8_t *const *meta, const size_t *meta_lens, uint8_t **outs, size_t *out_lens);

/* ---- sample-rate conversion: a resident batch at one rate becomes a resident batch at another, on the device ---------------
 * in_rate -> out_rate with g = gcd: L = out_rate / g phases, M = in_rate / g. Output frame j of a clip sits at input time
 * j * M / L: with i = floor(j * M / L) and p = (j * M) mod L, y[j] = sum_k h[p][k] * x[i + k - taps/2 + 1] per channel, x zero
 * outside the clip; n_in frames give ceil(n_in * L / M). h is a Kaiser-windowed sinc (beta 9, 32 zero crossings each side at
 * the lower of the two rates, cut-off at 0.91 of the lower Nyquist frequency: about 90 dB in the stop band, flat to about
 * 0.82 of that Nyquist), every row normalised to a sum of 1 in f64, then rounded to f32.
 * Supported: both rates in 1 .. 384000, L <= 1024, taps <= 2048, L * taps * 4 <= 1 MiB; anything else is FLO_ERR_ARG with a
 * message that names the offending quantity. Equal rates are not filtered: the result is a copy, bit for bit.
 * flo_resample_filter: host only, no context: the table [L][taps] (malloc'ed, flo_free; table may be NULL) and the geometry
 *   in force: a workgroup of the kernel makes tile_outputs consecutive outputs of one clip. err (may be NULL) gets the message.
 * flo_resample_out_frames: ceil(in_frames * L / M); FLO_ERR_ARG for an unsupported pair.
 * flo_batch_resample: a new batch of the same mode, channels, quality / level and bit depth at out_rate, every clip
 *   converted in one launch (enqueued on the ctx stream; flo_batch_sync on either batch orders it). Clip i has
 *   out_frames(n_interleaved[i] / channels) * channels samples: whole sample-frames are converted, a trailing partial one is
 *   not carried over. The source batch stays valid and unchanged; a batch of no clips gives a batch of no clips. The result
 *   of a clip does not depend on the batch around it. The new batch is destroyed like any other, before its context.
 * flo_resample: one clip from host memory and back (upload, the same kernel, fetch): *out malloc'ed, flo_free. */
typedef struct flo_resample_info { uint32_t L, M, taps, tile_outputs; } flo_resample_info;
int flo_resample_filter(uint32_t in_rate, uint32_t out_rate, flo_resample_info *info, float **table, char *err, size_t err_cap);
int flo_resample_out_frames(uint32_t in_rate, uint32_t out_rate, uint64_t in_frames, uint64_t *out_frames);
int flo_batch_resample(flo_batch *src, uint32_t out_rate, flo_batch **out);
int flo_resample(flo_ctx *ctx, const float *pcm, size_t n_interleaved, uint32_t in_rate, uint32_t out_rate, uint8_t channels,
                 float **out, size_t *n_out_interleaved);

/* ---- loudness normalisation and true-peak limiting: a resident batch becomes a resident batch at a target level -------------
 * (no counterpart in the reference; DESIGN 4.14 has the definition in full.)
 * The measure: with h the 1 -> 4 interpolator of the sample-rate conversion (flo_resample_filter(1, 4): 4 rows of 64 taps),
 * e_q[n, c] = the f32 FMA chain over k = 0 .. 63 of h[q][k] * y[n + k - 31, c] from 0, y zero outside the clip: bit for bit
 * output 4n + q of a conversion to four times the rate. p[n] = max over c of max(|y[n, c]|, max_q |e_q[n, c]|).
 * flo_analysis::true_peak_dbtp is another quantity (the reference's 49-tap figure) and stays as it is.
 * flo_batch_true_peak: linear[i] = max_n p[n] of clip i with y = x, whole sample-frames only; 0 for a clip without frames,
 *   NaN (0x7FC00000) where a sample or an envelope value is NaN. Synchronous.
 * flo_normalize_gain: host only, no context. The gain of one clip from its integrated loudness (flo_analysis::integrated_lufs),
 *   its sample peak (flo_analysis::sample_peak_dbfs) and its true peak (flo_batch_true_peak): gain_db = target_lufs -
 *   integrated, clamped to +- max_gain_db; C = (float)10^(ceiling_dbtp / 20); gain = (float)10^(gain_db / 20). In
 *   FLO_NORM_GAIN mode the gain is lowered until true_peak * gain <= C (1 - 2^-15) in f64 (the margin covers the roundings, so
 *   the output's own true peak is at most C); in FLO_NORM_LIMIT mode the limiter holds the
 *   ceiling, and the gain is lowered only until true_peak * gain <= 2^100, so that nothing overflows. A clip whose sample
 *   peak is -150 (silent) and a clip with a non-finite loudness, sample peak or true peak are copied unchanged: gain 1 and a
 *   status flag. opts NULL means the defaults: -14 LUFS, -1 dBTP, FLO_NORM_GAIN, look-ahead 0, max_gain_db 30.
 *   FLO_ERR_ARG with a message in err (may be NULL) that names the quantity: a non-finite target_lufs or ceiling_dbtp, a
 *   ceiling_dbtp outside -60 .. 60, a max_gain_db outside 0 .. 120, an unknown mode, lookahead_frames above 1024.
 * flo_normalize_lookahead: the look-ahead A in frames at `rate`: opts->lookahead_frames, or for 0 max(1, round(0.0015 * rate));
 *   FLO_ERR_ARG with a message that names lookahead_frames when that is above 1024.
 * FLO_NORM_GAIN: out[n, c] = fl32(x[n, c] * gain): one rounding, linear.
 * FLO_NORM_LIMIT: y = fl32(x * gain); r[n] = 2^24 where p[n] <= C, else (uint32)((C / p[n]) * 16777216.0f), IEEE division,
 *   truncated; m[k] = min r[k - A .. k + A], r outside the clip counting as 2^24; S[n] = sum m[n - A .. n + A];
 *   s[n] = S[n] div (2A + 1); z[n, c] = fl32(y[n, c] * ((float)s[n] * 2^-24)). s[n] <= r[n], so no sample of z exceeds C by
 *   more than the two roundings (C (1 + 2^-22)); the oversampled peak of z passes C only through the modulation of s
 *   (DESIGN 4.14 has the measured figures). Every step behind p is integer arithmetic.
 * flo_batch_normalize: a new batch of the same mode, rate, channels, quality / level and bit depth; clip i has its whole
 *   sample-frames (a trailing partial one is not carried over). The loudness of every clip comes from
 *   flo_batch_analyze_all, the true peak from flo_batch_true_peak, then one launch makes every clip. The source batch stays
 *   valid and unchanged; a batch of no clips gives a batch of no clips; the result of a clip does not depend on the batch
 *   around it. reports (may be NULL): [n_clips]. Synchronous: the new batch is complete on return.
 * flo_normalize: one clip from host memory and back: *out (n_interleaved / channels whole frames) malloc'ed, flo_free.
 * FLO_NORM_NO_SKIP in the environment (read per call, any value but "0") makes every tile of a LIMIT launch take the long
 *   path: a tile whose staged samples cannot reach the ceiling otherwise stores y without computing p. Same bits. */
#define FLO_NORM_GAIN 0
#define FLO_NORM_LIMIT 1
#define FLO_NORM_STATUS_SILENT 1u      /* sample_peak_dbfs is -150: copied */
#define FLO_NORM_STATUS_NONFINITE 2u   /* a non-finite loudness, sample peak or true peak: copied */
typedef struct flo_normalize_opts {
    double target_lufs, ceiling_dbtp, max_gain_db;
    uint32_t mode, lookahead_frames;
} flo_normalize_opts;
typedef struct flo_normalize_report {
    double input_lufs;              /* the integrated loudness the gain was computed from */
    double input_true_peak_dbtp;    /* 20 log10 of input_true_peak, -150 at or below 1e-9 */
    double gain_db;                 /* 20 log10 of gain */
    double ceiling_reduction_db;    /* what the ceiling (GAIN mode) or the overflow guard took off the clamped gain_db; >= 0 */
    float input_true_peak, gain;    /* linear */
    uint32_t status;                /* FLO_NORM_STATUS_* */
    uint32_t min_gain_q24;          /* LIMIT mode: the smallest s[n], 2^24 = unity (2^24 in GAIN mode and for a copied clip) */
    uint64_t limited_frames;        /* LIMIT mode: frames with s[n] < 2^24 */
} flo_normalize_report;
int flo_batch_true_peak(flo_batch *b, float *linear);
int flo_normalize_gain(double integrated_lufs, double sample_peak_dbfs, float true_peak_linear, const flo_normalize_opts *opts,
                       flo_normalize_report *report, char *err, size_t err_cap);
int flo_normalize_lookahead(uint32_t rate, const flo_normalize_opts *opts, uint32_t *frames, char *err, size_t err_cap);
int flo_batch_normalize(flo_batch *src, const flo_normalize_opts *opts, flo_batch **out, flo_normalize_report *reports);
int flo_normalize(flo_ctx *ctx, const float *pcm, size_t n_interleaved, uint32_t sample_rate, uint8_t channels,
                  const flo_normalize_opts *opts, float **out, flo_normalize_report *report);

/* ---- trimming, fades, padding and channel remixing: a resident batch becomes a resident batch of cuts, on the device --------
 * (no counterpart in the reference; DESIGN 4.15 has the definition in full.)
 * Source: clip i of the source batch has N_i whole sample-frames of Cin channels, x_i[n, c]; a trailing partial sample-frame
 * is not part of it. Output clip k is one cut of one source clip, described by segment k: T = pad_head + frames + pad_tail
 * frames of Cout channels. Any number of segments may name the same source clip, overlapping or not; they are independent.
 * Output frame t, with u = t - pad_head: where u < 0, u >= frames or start + u >= N_clip, every channel is +0.0 (not the mix
 * of zeros: a negative coefficient would make -0.0). Otherwise, with n = start + u:
 *   mix: matrix NULL (only with Cout == Cin): y[j] = x[n, j], bit for bit. With a matrix m[Cout][Cin] (row-major f32, every
 *     entry finite, Cin and Cout in 1 .. 8): a = fl32(m[j][0] * x[n, 0]), then a = fmaf(m[j][i], x[n, i], a) for
 *     i = 1 .. Cin - 1 in that order, y[j] = a. The first step is a plain product, so m = [[1]] keeps -0.0.
 *   fade: fade_in and fade_out are each <= frames and < 2^24, so every integer below converts to f32 exactly.
 *     w_in = fl32((float)u / (float)fade_in) if u < fade_in; with v = frames - 1 - u, w_out = fl32((float)v / (float)fade_out)
 *     if v < fade_out; both IEEE divisions. Neither applies: out = y, no multiplication. One applies: out = fl32(y * w).
 *     Both apply: out = fl32(y * fl32(w_in * w_out)).
 * Active range: frame n of a clip is active when !(fabsf(x[n, c]) <= threshold) for some channel c (a NaN sample is active).
 *   first = the smallest active frame, end = the largest active frame plus one; first = end = 0 for a clip without one.
 *   threshold must be >= 0 and not NaN; +inf is allowed.
 * FLO_ERR_ARG with a message that names the quantity: clip >= n_clips; reserved != 0; fade_in or fade_out longer than
 *   frames or >= 2^24; matrix NULL with out_channels != the source's channels; a non-finite matrix entry; in_channels or
 *   out_channels above 8 with a matrix; out_channels above 8 for a lossy batch; a T * out_channels that overflows what
 *   flo_batch_create accepts; a threshold that is negative or NaN.
 * flo_batch_edit: a new batch of the same mode, rate, quality / level and bit depth as src with out_channels channels and
 *   n_out clips, made by one launch (enqueued on the ctx stream; flo_batch_sync on either batch orders it). The work list
 *   lives in pinned and device memory that the new batch owns until it is destroyed. The source batch stays valid and
 *   unchanged; n_out == 0 gives a batch of no clips; an output clip does not depend on the batch around it. The new batch
 *   behaves like an uploaded one: it encodes, analyses, resamples and normalises like any other.
 * flo_batch_active_range: first[i], end[i] of every clip, [n_clips] each. Synchronous.
 * flo_edit: one clip from host memory and back (upload, the same kernel, fetch): *out (*n_out interleaved samples)
 *   malloc'ed, flo_free.
 * flo_edit_tile_frames: host only, no context: the output frames one workgroup of the kernel makes for this pair of channel
 *   counts (out_channels >= 1). The tiles of an output clip start at multiples of it. */
typedef struct flo_edit_segment {
    uint64_t start, frames;       /* source frames [start, start + frames) of clip `clip`; may reach past its end */
    uint32_t clip;
    uint32_t pad_head, pad_tail;  /* frames of +0.0 in front of and behind the cut */
    uint32_t fade_in, fade_out;   /* linear, in frames of the cut; 0 = none */
    uint32_t reserved;            /* must be 0 */
} flo_edit_segment;               /* 40 bytes */
int flo_batch_edit(flo_batch *src, size_t n_out, const flo_edit_segment *segs, uint8_t out_channels,
                   const float *matrix /* NULL: copy */, flo_batch **out);
int flo_batch_active_range(flo_batch *b, float threshold, uint64_t *first, uint64_t *end);
int flo_edit(flo_ctx *ctx, const float *pcm, size_t n_interleaved, uint32_t sample_rate, uint8_t channels,
             const flo_edit_segment *seg, uint8_t out_channels, const float *matrix, float **out, size_t *n_out);
int flo_edit_tile_frames(uint8_t in_channels, uint8_t out_channels, uint32_t *frames);

/* ---- mixing and concatenation: several resident batches become one resident batch of sums of their clips, on the device ----
 * (no counterpart in the reference; DESIGN 4.17 has the definition in full.)
 * Sources: n_srcs >= 1 resident batches of one context, one sample rate and one channel count C. Clip i of a source has N_i
 * whole sample-frames; a trailing partial sample-frame is not part of it. The output batch has n_out clips, clip k of
 * out_frames[k] = T_k frames of C channels. A list of n_parts parts says what is laid where: source frames
 * [start, start + frames) of clip `clip` of srcs[batch] land on output frames [at, at + frames) of output clip `out`, times
 * `gain`, faded linearly over fade_in frames at the part's start and fade_out frames at its end.
 * The list: `out` is non-decreasing along it; inside one output clip the list order is the order of summation, which need
 * not be the order in time; any number of parts may name the same source clip, and they may overlap; an output clip may
 * have no part at all.
 * Part p is live on output frame t of clip k = p.out when at <= t < at + frames, t < T_k and start + (t - at) < N: parts
 * that reach past the source's end or past the output's end are cut there, not refused. For a live frame, u = t - at and
 * v = frames - 1 - u; the fade weight is flo_batch_edit's: w_in = fl32((float)u / (float)fade_in) if u < fade_in,
 * w_out = fl32((float)v / (float)fade_out) if v < fade_out, both IEEE divisions, w = fl32(w_in * w_out) where both apply.
 * The part's coefficient is k_p = gain where no fade applies, else k_p = fl32(gain * w).
 * Output sample (t, c): a = +0.0f; for every part of clip k that is live on t, in list order,
 * a = fmaf(k_p, x_p[start + u, c], a); the result is a. So a frame that no part covers is +0.0; one part at gain 1
 * reproduces the source bit for bit except that -0.0 becomes +0.0 (fmaf(1, -0, +0) = +0); one part at gain 1 with fades
 * gives fl32(w * x), flo_batch_edit's value up to the same sign of zero.
 * FLO_ERR_ARG with a message that names the quantity: n_srcs == 0 or a NULL source; sources of different context, rate or
 *   channel count; out >= n_out; out decreasing along the list; batch >= n_srcs; clip >= n_clips of that batch; fade_in or
 *   fade_out longer than frames or >= 2^24; a non-finite gain; at + frames or start + frames wrapping 64 bits;
 *   n_parts >= 2^32; T_k * C beyond what flo_batch_create accepts; too many tiles for one launch. FLO_ERR_STATE when a
 *   source that some part names holds no PCM yet.
 * flo_batch_mix: a new batch of the mode, quality / level and bit depth of srcs[0], at the common rate and C channels, made
 *   by one launch (enqueued on the ctx stream; flo_batch_sync on any of the batches orders it). The work list lives in
 *   pinned and device memory that the new batch owns until it is destroyed. The sources stay valid and unchanged. The new
 *   batch behaves like an uploaded one: it encodes, analyses, resamples, normalises and edits like any other. One workgroup
 *   makes flo_edit_tile_frames(C, C) output frames of one clip; it scans all parts of its clip.
 * flo_mix: n_clips clips from host memory as one source (every part has batch == 0 and out == 0) and the one output clip
 *   of out_frames frames back: *out (*n_out interleaved samples) malloc'ed, flo_free. */
typedef struct flo_mix_part {
    uint64_t start, frames, at;   /* source frames [start, start + frames) land on output frames [at, at + frames) */
    uint32_t out, batch, clip;    /* output clip; index into srcs; clip of that batch */
    uint32_t fade_in, fade_out;   /* linear, in frames of the part; 0 = none */
    float gain;
} flo_mix_part;                   /* 48 bytes */
int flo_batch_mix(flo_batch *const *srcs, size_t n_srcs, size_t n_out, const uint64_t *out_frames, size_t n_parts,
                  const flo_mix_part *parts, flo_batch **out);
int flo_mix(flo_ctx *ctx, size_t n_clips, const float *const *pcm, const size_t *n_interleaved, uint32_t sample_rate,
            uint8_t channels, size_t n_parts, const flo_mix_part *parts, uint64_t out_frames, float **out, size_t *n_out);

/* ---- FIR filtering and convolution: the clips of a resident batch filtered by clips of another, on the device ---------------
 * (no counterpart in the reference; DESIGN 4.18 has the definition in full.)
 * Sources: src is a resident batch of C channels (1 .. 8) at rate R; clip i has N_i whole sample-frames x_i[n, c], a trailing
 * partial sample-frame is not part of it. irs is a resident batch of the same context and the same rate with Ch channels,
 * Ch == 1 or Ch == C; clip j has P_j whole frames. irs == src is allowed.
 * Output clip k is described by job k. With N and P the frames of source clip `clip` and of response clip `ir`:
 *   K = min(taps, P - min(ir_start, P)) taps, so taps = UINT32_MAX means "to the end of the response clip";
 *   h[k, c] is frame ir_start + k of response clip `ir`, channel (Ch == 1 ? 0 : c).
 * Output clip k has T = frames frames of C channels. Sample (t, c): a = +0.0f; for k = 0 .. K - 1 in ascending order, with
 * m = t + skip - k as a mathematical integer and xv = x[m, c] if 0 <= m < N, else +0.0f: a = fmaf(h[k, c], xv, a). The result
 * is a. Every tap is applied, against +0.0 outside the clip; no tap is skipped. So:
 *   K == 0 gives +0.0 everywhere;
 *   h = [1] with skip = 0 reproduces the source, except that -0.0 becomes +0.0 (fmaf(1, -0, +0) = +0);
 *   a NaN tap makes every sample of its channel NaN; an infinite tap makes NaN wherever it meets a zero (every frame outside
 *   the clip is one: inf * 0 is NaN, and NaN stays) and an infinity elsewhere;
 *   the result depends on the job alone: not on the batch around it, the tile, the tap chunk or the kernel variant.
 * There is no gain and there are no fades: flo_batch_mix on the result does wet/dry.
 * FLO_ERR_ARG with a message that names the quantity: a NULL batch; batches of different contexts; different rates (see
 *   flo_batch_resample); channels of src outside 1 .. 8; Ch other than 1 or C; clip >= n_clips of src; ir >= n_clips of irs;
 *   reserved != 0; K > FLO_CONV_MAX_TAPS; frames + skip wrapping 64 bits; frames * C beyond what flo_batch_create accepts; too
 *   many tiles for one launch. FLO_ERR_STATE when a batch that some job names holds no PCM yet.
 * flo_batch_convolve: a new batch of the mode, quality / level and bit depth of src, at its rate and C channels, made by one
 *   launch (enqueued on the ctx stream; flo_batch_sync on any of the three batches orders it). The work list lives in pinned
 *   and device memory that the new batch owns until it is destroyed. The sources stay valid and unchanged; n_out == 0 gives a
 *   batch of no clips. The new batch behaves like an uploaded one.
 * flo_convolve: one clip and one response from host memory and back (clip == ir == 0; upload, the same kernel, fetch): *out
 *   (*n_out interleaved samples) malloc'ed, flo_free.
 * flo_conv_geometry: host only, no context: the geometry of the kernel variant these two channel counts select. The tiles
 *   of an output clip start at multiples of tile_frames; taps are staged tap_chunk at a time; one lane owns lane_outputs
 *   consecutive output frames.
 * flo_fir_design: host only, no context: a windowed-sinc FIR of taps = 2H + 1 coefficients (odd, 3 .. 65535) at `rate`,
 *   *table malloc'ed (flo_free). All arithmetic is f64, the table is rounded to f32 once at the end. With
 *   g[k] = (2f/R) sinc(2f (k - H)/R) I0(beta sqrt(1 - ((k - H)/H)^2)) / I0(beta) and lp(f)[k] = g[k] / sum(g):
 *   LOWPASS = lp(f_hi); HIGHPASS = delta[k - H] - lp(f_lo); BANDPASS = lp(f_hi) - lp(f_lo); BANDSTOP = delta - BANDPASS.
 *   beta is finite in 0 .. 16; the frequencies a kind uses are in Hz, 0 < f < rate / 2, f_lo < f_hi where both are used; the
 *   one a kind does not use is ignored. FLO_ERR_ARG with a message in err otherwise. */
#define FLO_CONV_MAX_TAPS 65536u
#define FLO_FIR_LOWPASS 0u
#define FLO_FIR_HIGHPASS 1u
#define FLO_FIR_BANDPASS 2u
#define FLO_FIR_BANDSTOP 3u
typedef struct flo_conv_job {
    uint64_t frames, skip, ir_start;   /* T; the delay taken off the front; the response's first frame */
    uint32_t clip, ir, taps, reserved; /* clip of src; clip of irs; at most this many taps; must be 0 */
} flo_conv_job;                        /* 40 bytes */
typedef struct flo_conv_info {
    uint32_t tile_frames, tap_chunk, lane_outputs;
} flo_conv_info;
int flo_batch_convolve(flo_batch *src, flo_batch *irs, size_t n_out, const flo_conv_job *jobs, flo_batch **out);
int flo_convolve(flo_ctx *ctx, const float *pcm, size_t n_interleaved, const float *ir, size_t ir_interleaved,
                 uint32_t sample_rate, uint8_t channels, uint8_t ir_channels, const flo_conv_job *job, float **out, size_t *n_out);
int flo_conv_geometry(uint8_t channels, uint8_t ir_channels, flo_conv_info *info);
int flo_fir_design(uint32_t kind, uint32_t rate, double f_lo, double f_hi, uint32_t taps, double beta, float **table, char *err,
                   size_t err_cap);

/* ---- partitioned FFT convolution: the same jobs for long responses, on the device ------------------------------------------
 * (no counterpart in the reference; DESIGN 4.19 has the definition in full.)
 * A second way to run a list of flo_conv_job: sources, jobs, K, h[k, c], Ch, irs == src and the skip clamp min(skip, N + K)
 * mean what they mean above. The result approximates the chain above in f32; it does not reproduce it to the bit.
 * Uniformly partitioned overlap-save with B = block_frames, F = 2B, Pn = ceil(K / B):
 *   partition p is taps [pB, min((p + 1)B, K)) of channel c, zero-padded to F, real-FFT'd to H_p;
 *   segment q of a job (q may be negative) is source frames [(q - 1)B + skip, (q + 1)B + skip), +0.0 outside [0, N),
 *     real-FFT'd to X_q; a segment wholly outside the clip is zero and takes no part;
 *   output block b is frames [bB, (b + 1)B) of the output, ragged at T: Y_b = sum over p = 0 .. Pn - 1 of X_{b-p} * H_p,
 *     accumulated from zero in ascending p; the last B values of irfft(Y_b) are the block.
 *   There are no atomics: a job's output depends on the job alone, not on the batch, the job's place in the list, the
 *   grouping of the scratch (FLO_CONV_FFT_GROUP_BYTES, read per call, default 1 GiB) or what the scratch held before.
 *   A NaN or infinite sample or tap leaves every block it reaches (q in [b - Pn + 1, b]; any partition) unspecified and no
 *   other; no call refuses them. Blocks whose every segment or partition is zero compare equal to zero; K == 0 gives zeros.
 * FLO_ERR_ARG and FLO_ERR_STATE as for flo_batch_convolve, in the same order, with K > FLO_CONV_FFT_MAX_TAPS in the place of
 *   K > FLO_CONV_MAX_TAPS. A failed call leaves no batch and a usable context.
 * flo_batch_convolve_fft: a new batch like flo_batch_convolve's. Responses are transformed once per distinct
 *   (ir, ir_start, K) of the call; segment spectra live in pool scratch that goes back before the call returns, so the call
 *   returns when its launches have run.
 * flo_convolve_fft: flo_convolve over this path.
 * flo_conv_fft_geometry: host only, no context: block_frames (B); lane_blocks, the output blocks a lane accumulates side by
 *   side (a tile is lane_blocks * B output frames); max_taps; crossover_taps, the smallest measured K from which this path
 *   is no slower than the direct one (what method "auto" of the Python package goes by). */
#define FLO_CONV_FFT_MAX_TAPS 1048576u
typedef struct flo_conv_fft_info {
    uint32_t block_frames, lane_blocks, max_taps, crossover_taps;
} flo_conv_fft_info;                   /* 16 bytes */
int flo_batch_convolve_fft(flo_batch *src, flo_batch *irs, size_t n_out, const flo_conv_job *jobs, flo_batch **out);
int flo_convolve_fft(flo_ctx *ctx, const float *pcm, size_t n_interleaved, const float *ir, size_t ir_interleaved,
                     uint32_t sample_rate, uint8_t channels, uint8_t ir_channels, const flo_conv_job *job, float **out, size_t *n_out);
int flo_conv_fft_geometry(uint8_t channels, uint8_t ir_channels, flo_conv_fft_info *info);

/* ---- spectral similarity: spectral_similarity (core/analysis.rs:395-437, exported as spectral_similarity_score,
 * lib.rs:1357) over fingerprint sets ----------------------------------------------------------------------------------
 * flo_fingerprint is SpectralFingerprint (analysis.rs:10-26): what flo_analyze / flo_batch_analyze_all return in those
 * fields, or the `spectrum_fingerprint` of a file's META. The score of two fingerprints is the reference's, bit for bit in
 * f32: 1.0 for equal hashes (tested first), else 0.0 for a different sample rate or channel count, else
 * fl(fl(fl(e * 0.5) + fl(p * 0.3)) + fl(l * 0.2)) with e, p the sequential sums over the 16 energy and 8 peak bytes of
 * 1 - |a - b| / 255, divided by 16 and 8, and l that term of the loudness bytes. Symmetric bit for bit.
 * flo_spectral_similarity scores one pair on the host (no context needed).
 * flo_fpindex_create copies n fingerprints to the device once (fps may be freed afterwards; n = 0 is a valid, empty index);
 * the queries below run on the device, on the context's stream, and return when their results are in the caller's arrays.
 * Ranking: score descending, then member index ascending; the result does not depend on how the work is split.
 *   flo_fpindex_topk:      for each of n_q queries, the k best members: idx / score [n_q][k]. k in 0 .. 64 (FLO_ERR_ARG
 *                          above); n_q = 0 or k = 0 do nothing. Members of another format are candidates at 0.0.
 *   flo_fpindex_topk_self: the same for every member against the others: idx / score [n][k]; a member is never its own
 *                          neighbour (other members with its hash are, at 1.0).
 *   Slots beyond the candidates there are hold UINT32_MAX and -1.0f.
 *   flo_fpindex_pairs:     every pair i < j with score >= threshold as (i[p], j[p], score[p]), ordered by (i, j).
 *                          *n_pairs is always the exact count; when it exceeds cap, nothing is written and the call
 *                          returns FLO_ERR_NOMEM (call again with cap = *n_pairs). A NaN threshold is FLO_ERR_ARG. */
typedef struct flo_fingerprint {   /* SpectralFingerprint, analysis.rs:10-26 */
    uint8_t hash[32];
    uint32_t duration_ms, sample_rate;
    uint8_t channels, avg_loudness, pad0, pad1;
    uint8_t frequency_peaks[8];
    uint8_t energy_profile[16];
} flo_fingerprint;
float flo_spectral_similarity(const flo_fingerprint *a, const flo_fingerprint *b);
typedef struct flo_fpindex flo_fpindex;
int flo_fpindex_create(flo_ctx *ctx, const flo_fingerprint *fps, size_t n, flo_fpindex **out);
void flo_fpindex_destroy(flo_fpindex *ix);
int flo_fpindex_topk(flo_fpindex *ix, const flo_fingerprint *q, size_t n_q, uint32_t k, uint32_t *idx, float *score);
int flo_fpindex_topk_self(flo_fpindex *ix, uint32_t k, uint32_t *idx, float *score);
int flo_fpindex_pairs(flo_fpindex *ix, float threshold, uint64_t cap, uint32_t *i, uint32_t *j, float *score,
                      uint64_t *n_pairs);

/* ---- fidelity reports: decoded audio against its source, on the device (the "compare original vs encoded" of the
 * reference's TODO) ------------------------------------------------------------------------------------------------------
 * x is the source, y what flo_decode returns for the clip's file, both interleaved f32 with `channels` channels. Only whole
 * sample-frames are compared, decoded frame t against source frame t (the 1024-frame pre-roll is dropped, encoder.rs:176-179,
 * lib.rs:338-341). compared = min(source_frames, decoded_frames); a lossy clip of n frames decodes to ceil(n / 1024) * 1024
 * frames, a tail of fewer than 1024 frames past the source's end.
 * Block b covers frames [1024 b, 1024 (b + 1)) of the compared range: n_blocks = ceil(compared / 1024). Per block and
 * channel, all arithmetic in f64 without contraction:
 *   signal = sum x^2, error = sum (y - x)^2 (the difference taken in f64), peak_error = max |y - x| rounded to f32 once,
 *   peak_out = max |y|, clipped = the count of |y| > 1, n = the compared frames of the block.
 * Summation order: lane l of 64 holds the block positions j = l + 64 k, k = 0 .. 15, and adds its terms in k ascending from
 * its k = 0 term; positions past the block's compared part add 0; the lanes then combine by an xor butterfly over offsets
 * 32, 16, 8, 4, 2, 1 (v[l] = v[l] + v[l ^ o]).
 * Per clip and channel: signal and error are the sequential f64 sums of the block values in block order, from 0.0;
 * tail_energy is sum y^2 over the decoded frames past `compared`, per block of the same grid in the same lane order, the
 * blocks then summed in order from 0.0; peak_error, peak_out and clipped are taken over all blocks.
 *   snr_db = 10 log10(signal / error): +inf when error = 0 (silence included), -inf when signal = 0 < error.
 *   seg_snr_db = the mean (sequential sum in block order, then / seg_blocks) over the blocks with signal / n >= 1e-10 of
 *   clamp(10 log10(signal_b / error_b), -10, 60), an error_b of 0 counting as 60; NaN when no block qualifies.
 * Non-finite samples (NaN, +-inf, in the source or in the decode): the sums carry them as the IEEE additions above give
 * them (inf - inf in the difference is NaN), and snr_db follows from the sums by the same three cases. A block qualifies
 * by the same test (a NaN signal_b does not), an error_b that is not exactly 0 never counts as 60, and the clamp of NaN is
 * NaN, so one such block makes seg_snr_db NaN. peak_error, peak_out and clipped leave NaN terms out: the maxima are
 * fmax from 0 (an infinite term is a maximum like any other) and NaN is not > 1. Which NaN encoding a field holds is not
 * defined. A clip's report depends on that clip alone.
 * No float atomics: two calls return identical bits, whatever the split of the work.
 * flo_batch_fidelity, after flo_batch_sync: out[n_clips * channels], clip-major; clip i's block records at
 * blocks[(block_off[i] + b) * channels + c], block_off (n_clips + 1 entries) the running sum of n_blocks; blocks_cap counts
 * records. out == NULL: the sizing call, only block_off is filled. blocks == NULL: the per-clip records only. A lossy batch
 * is decoded and compared in one pass that writes no PCM; a lossless batch is decoded into device scratch and compared behind
 * it (FLO_FIDELITY_UNFUSED=1, read per call, does the same for a lossy batch). The source is the batch's device copy.
 * flo_compare: one .flo file against n_interleaved floats of host PCM with the file's channel count. out[channels];
 * blocks (may be NULL) receives the clip's n_blocks * channels records, block-major (n_blocks <= ceil(source frames /
 * 1024)); *n_blocks (may be NULL) is the clip's block count.
 * Errors: FLO_ERR_STATE before sync; FLO_ERR_FORMAT for an unreadable file or a transform frame that does not deserialise,
 * with flo_decode's message; FLO_ERR_ARG for null or short buffers. */
typedef struct flo_fidelity_block {
    double signal, error;
    float peak_error, peak_out;
    uint32_t clipped, n;
} flo_fidelity_block;
typedef struct flo_fidelity {   /* one channel of one clip */
    double signal, error, tail_energy, snr_db, seg_snr_db;
    float peak_error, peak_out;
    uint64_t clipped, compared_frames, source_frames, decoded_frames;
    uint32_t n_blocks, seg_blocks;
} flo_fidelity;
int flo_batch_fidelity(flo_batch *b, flo_fidelity *out, flo_fidelity_block *blocks, size_t blocks_cap, uint64_t *block_off);
int flo_compare(flo_ctx *ctx, const float *pcm, size_t n_interleaved, const uint8_t *flo, size_t len, flo_fidelity *out,
                flo_fidelity_block *blocks, size_t blocks_cap, size_t *n_blocks);

/* ---- streaming encoder: StreamingEncoder of libflo/src/streaming/encoder.rs:6-257 -----------------------------
 * Samples are pushed (interleaved f32); every complete one-second frame is encoded losslessly - all frames a push
 * completes in ONE device batch - and queued; frames are pulled one by one, or assembled into a complete .flo file.
 * Frame bytes are the reference's encode_frame_data / serialize_channel bytes (encoder.rs:215-257).
 *   flo_stream_create  <- StreamingEncoder::new(sr, ch, bits).with_compression(level)      encoder.rs:33-56
 *   flo_stream_push    <- push_samples                                                     :71-75
 *   flo_stream_next_frame <- next_frame (1: a frame came out, data malloc'ed / flo_free; 0: none; -1: error)   :78-85
 *   flo_stream_flush   <- flush: the buffered remainder as one partial frame, returned, not queued   :88-110
 *   flo_stream_finalize <- finalize: header + TOC + DATA (+ META) of the frames not pulled yet       :113-185 */
typedef struct flo_stream flo_stream;
int flo_stream_create(flo_ctx *ctx, uint32_t sample_rate, uint8_t channels, uint8_t bit_depth, uint8_t level,
                      flo_stream **out);
void flo_stream_destroy(flo_stream *s);
int flo_stream_push(flo_stream *s, const float *samples, size_t n_interleaved);
size_t flo_stream_pending_samples(const flo_stream *s);   /* sample-frames waiting for a full second */
size_t flo_stream_pending_frames(const flo_stream *s);
int flo_stream_next_frame(flo_stream *s, uint32_t *index, uint32_t *timestamp_ms, uint32_t *samples, uint8_t **data,
                          size_t *len);
int flo_stream_flush(flo_stream *s, uint32_t *index, uint32_t *timestamp_ms, uint32_t *samples, uint8_t **data,
                     size_t *len);
int flo_stream_finalize(flo_stream *s, const uint8_t *meta, size_t meta_len, uint8_t **out, size_t *out_len);

/* ---- lossy streaming encoder: encode_to_flo (libflo/src/lossy/encoder.rs:167-239) frame by frame, many streams per pass ----
 * A lossy stream is a flo_stream: pending_*, push, next_frame, flush, finalize and destroy apply to it.
 *   - Byte identity: samples pushed in any pieces (a piece may split a sample-frame), nothing pulled, then finalize(meta)
 *     gives byte for byte flo_encode_lossy(ctx, x, sr, ch, quality, meta), the empty signal included; a trailing partial
 *     sample-frame is dropped as the offline encoder drops it.
 *   - Frame h (0: the pre-roll frame) is encoded and queued once (h + 1) * 1024 sample-frames have been pushed; its
 *     (index, timestamp_ms, samples = 1024, data) are the offline file's TOC entry h and frame bytes. How the input is
 *     cut into pushes, and how many frames each stream brings to a flo_stream_encode_ready call, change no byte.
 *   - flush ends the input: the one or two trailing frames that the offline encoder makes from its zero padding join the
 *     queue, then it returns the queue's front like next_frame (1 / 0). Afterwards push and append return FLO_ERR_STATE.
 *     finalize flushes if that has not happened, then writes a file of the frames not pulled yet (META verbatim).
 *   - pending_samples: sample-frames pushed but not yet the second half of an encoded frame (0 .. 1023 after a push).
 * flo_stream_create_lossy: quality clamped to [0, 1] (TransformEncoder::new); channels 1 .. 8, FLO_ERR_ARG otherwise.
 * flo_stream_append (either kind of stream): buffers the samples, encodes nothing.
 * flo_stream_encode_ready: every complete frame of every listed stream is encoded and queued; status[i] is FLO_OK or the
 *   stream's error (FLO_ERR_ARG for a stream of another context); returns FLO_OK or the first error. Lossy streams of any
 *   mix of (sample rate, channels, quality): per distinct configuration one upload (the streams' windows - the 1024
 *   sample-frames each carried over and its new ones - with their carried masking levels), one set of launches and one
 *   read-back; the call synchronises once. A stream's carried state stays on the host: streams own no device memory.
 *   Lossless streams: their complete seconds in one lossless batch per (sample rate, channels, bit depth, level), frames
 *   as flo_stream_push makes them. Streams with nothing complete contribute nothing. On a lossy stream flo_stream_push is
 *   append + encode_ready(ctx, 1, &s); on a lossless stream it is what it was. */
int flo_stream_create_lossy(flo_ctx *ctx, uint32_t sample_rate, uint8_t channels, float quality, flo_stream **out);
int flo_stream_append(flo_stream *s, const float *samples, size_t n_interleaved);
int flo_stream_encode_ready(flo_ctx *ctx, size_t n, flo_stream *const *streams, int *status);

/* ---- measurement hooks ----------------------------------------------------------------------------- */
/* When enabled, every launch of a named kernel on the ctx stream is bracketed by hipEvents on that stream. */
int flo_ctx_profile_enable(flo_ctx *ctx, int on);
/* sum and count of bracketed launches of `kernel` since the last reset (call after a sync) */
int flo_ctx_profile_query(flo_ctx *ctx, const char *kernel, double *total_ms, uint64_t *launches);
int flo_ctx_profile_reset(flo_ctx *ctx);
/* test hook: force the lossy kernel form (0 auto, 1 .. 5 as in flo_batch_encode) */
int flo_ctx_force_path(flo_ctx *ctx, int which);
/* test hook, process-wide: while byte is 0 .. 255 every block the device pool hands out (fresh or recycled) is set to that
 * byte over its whole size class before it is returned (null-stream memset + device synchronise), and every recycled
 * pinned download buffer over its capacity; -1 turns the fill off, which is the state at start. Returns the previous
 * setting (any other argument changes nothing). Results never depend on it: every byte read is written first. Off,
 * the allocation path pays one relaxed atomic load. */
int flo_debug_pool_fill(int byte);
/* test hook, process-wide: while microseconds is 0 .. 5000 the library queues a delay of about that long (one wavefront
 * that sleeps; no memory access, no waiting, no polling) in front of every launch of its own and, on every stream of its
 * own, right behind every wait for an event, so that the device runs late behind the host; -1 turns it off, which is
 * the state at start. Returns the previous setting (any other argument changes nothing). Results never depend on it:
 * every host read and every release of a block waits for the work it depends on. Off, a site pays one relaxed atomic
 * load. The exchange stream of flo_dist_* is not delayed. */
int flo_debug_stream_delay(int microseconds);
/* the number of delays queued so far in this process (by the switch above and by flo_debug_delay_enqueue) */
uint64_t flo_debug_stream_delays(void);
/* queues one such delay of 0 .. 5000 microseconds on any stream (hipStream_t), whatever the switch says: for tests that
 * make a caller's stream run late. Nothing is queued on a stream that is being captured. */
int flo_debug_delay_enqueue(void *stream, int microseconds);
/* stream handle (hipStream_t) of the context, for callers that enqueue their own work around the encode */
void *flo_ctx_stream(flo_ctx *ctx);

/* ---- stage-level entry points (parity tests call the kernels through these) -------------------------- */
/* forward MDCT of n_frames windows of 2048 samples (mono, back to back) -> n_frames*1024 coefficients.
 * Replaces Mdct::forward(samples, BlockSize::Long) with the Vorbis window — lossy/mdct.rs:337-347,166-226 */
int flo_mdct_forward(flo_ctx *ctx, const float *frames, size_t n_frames, float *coeffs);
/* per-frame intermediates of one clip's lossy encode, device path: arrays [hops][ch][1024] / [hops][ch][25];
 * any pointer may be NULL. Replaces TransformEncoder::encode_frame — lossy/encoder.rs:63-106 */
int flo_lossy_analyze(flo_ctx *ctx, const float *pcm, size_t n_interleaved, uint32_t sample_rate,
                      uint8_t channels, float quality, float *coeffs, int16_t *quantized, uint16_t *sf_words,
                      size_t *num_hops);
/* quantise + serialise given MDCT coefficients (device quantiser fed caller-supplied spectra):
 * coeffs [hops][ch][1024] -> quantized [hops][ch][1024], sf_words [hops][ch][25]. Replaces
 * PsychoacousticModel::calculate_smr + TransformEncoder::quantize_coefficients
 * (lossy/psychoacoustic.rs:151-235, lossy/encoder.rs:109-154). exact = 0 runs the quantiser exactly as every encode
 * entry point does (keep test in the amplitude domain); exact = 1 additionally re-decides coefficients within 1e-5
 * of the threshold with the reference's own dB-domain f32 expression (a test yardstick, never used by an encode). */
int flo_lossy_quantize(flo_ctx *ctx, const float *coeffs, size_t num_hops, uint32_t sample_rate, uint8_t channels,
                       float quality, int exact, int16_t *quantized, uint16_t *sf_words);
/* flo_lossy_quantize (exact = 0) that keeps what the encode wrote: beside the integers and scale words (either may be NULL)
 * the clip's DATA chunk (data_cap bytes of room, *data_len written; FLO_ERR_ARG when it does not fit) and the size of each
 * of its num_hops frames. The form is the one flo_ctx_force_path names (5: the lock-step chain kernel's coefficient-input
 * instantiation, 2: the frame-parallel kernels, otherwise 1), so the packer of each form runs on hand-made spectra. */
int flo_lossy_pack_frames(flo_ctx *ctx, const float *coeffs, size_t num_hops, uint32_t sample_rate, uint8_t channels,
                          float quality, int16_t *quantized, uint16_t *sf_words, uint8_t *data, size_t data_cap,
                          size_t *data_len, uint32_t *frame_sizes);
/* TransformEncoder::quantize_coefficients as the reference exposes it (lossy/encoder.rs:109-154): n_vec vectors of 1024
 * coefficients with the caller's own signal-to-mask ratios -> i16 (kept iff smr > the quality's threshold, c * scale factor
 * rounded half away from zero) and the 25 band scale factors (30000 / band maximum, 1.0 for a silent band) per vector.
 * smr = NULL: scale factors only (quantized is not written). */
int flo_lossy_quantize_smr(flo_ctx *ctx, const float *coeffs, const float *smr, size_t n_vec, uint32_t sample_rate, float quality,
                           int16_t *quantized, float *scale_factors);
/* serialize_sparse on device: n_vec vectors of 1024 i16 -> bytes; out_off[n_vec+1] prefix offsets.
 * Replaces lossy/encoder.rs:284-314. form = 0: the packer as the encoder runs it (item form up to 128 non-zeros, behind it
 * the block form, behind that the general form for the dense vectors it declines); form = 1: the general form for every
 * vector; form = 2: block form, then general (tests compare the three). */
int flo_sparse_pack(flo_ctx *ctx, const int16_t *q, size_t n_vec, int form, uint8_t *out, size_t out_cap,
                    uint32_t *out_off);

#ifdef __cplusplus
}
#endif
#endif
