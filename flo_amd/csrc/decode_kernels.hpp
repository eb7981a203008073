// decode_kernels.hpp — argument blocks and launchers of the device decode path (see decode_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fidelity_kernels.hpp"
#include "ll_route.hpp"
#include "lossy_device.hpp"

namespace flo {

// Corpus windows (lossy_decode_kernel<kDecWindow>): one descriptor per window, built per call.
struct LossyWinDev {
    unsigned long long frame0;        // the file's first frame in the corpus's compacted frame list (blob_off / blob_len)
    unsigned long long start;         // first sample-frame of the window in the file's decoded signal
    unsigned long long dst;           // float offset of the window's slot in `out`
    unsigned int n_frames;            // the file's frames (the decoded signal is (n_frames - 1) * 1024 sample-frames)
    unsigned int pad;
};
struct LossyWinArgs {
    const LossyWinDev *win;
    unsigned int n_windows;
    unsigned int runs_per_window;     // runs of LossyDecArgs::run blocks per window
    unsigned int length;              // window_frames
};
// Streaming decoders (lossy_decode_kernel<kDecStream>, flo_sdec_decode_ready): one descriptor per run of a stream's
// frames, built per call. A stream's overlap (the second half of the last frame it decoded, 1024 floats per channel,
// channel-major) lives in device memory between calls, in two halves: a call loads from one and stores into the other
// (kRunOdd: load the second half, store the first), since the runs of one stream are unordered workgroups of one launch.
constexpr unsigned kRunLoad = 1u;         // start from the stream's overlap state (else: the first frame only primes it)
constexpr unsigned kRunStore = 2u;        // store the run's final overlap into the other half of the state
constexpr unsigned kRunWriteFirst = 4u;   // the first frame writes a block (else it is a lead frame or the pre-roll)
constexpr unsigned kRunOdd = 8u;          // the call's parity: which half of the state is read
constexpr unsigned kRunBackLoad = 16u;    // a channel none of the `back` frames carries starts from the stream's overlap state
struct LossyRunDev {
    unsigned long long frame0;        // first frame of the run in the call's frame list (blob_off / blob_len)
    unsigned long long dst;           // float offset in `out` of the first block the run writes
    float *state;                     // [2][channels][1024] the stream's overlap, read half and written half (kRunOdd)
    unsigned int n_frames;            // frames of the run, 1 .. kDecRunLong + 1 (16 at most with kRunWriteFirst)
    unsigned int flags;               // kRun*
    unsigned int back;                // the stream's frames in front of frame0 in the call's frame list: where the overlap of a
    unsigned int pad;                 // channel that frame0 does not carry is looked for (the last of them that carries it)
};
struct LossyStreamArgs {
    const LossyRunDev *runs;
    unsigned int n_runs;
    unsigned int pad;
};
// kDecCompare: whole clips as kDecWhole, every block compared with the clip's source instead of stored (fidelity reports:
// LossyDecArgs::cmp, fidelity_kernels.hpp)
enum DecMode : int { kDecWhole = 0, kDecWindow = 1, kDecStream = 2, kDecCompare = 3 };

// One transform frame = one wavefront. Frames of a clip are addressed by (clip, local frame index).
struct LossyDecArgs {
    LossyDevTables T;                 // pack (rotation + FFT twiddles) and the coefficient -> band map of the file's sample rate
    const float *window;              // [2048] Vorbis window (mdct.rs:106-113)
    const uint8_t *bytes;             // device copy of the file(s)
    const unsigned long long *blob_off;   // [total_frames] offset of the frame's blob (channel 0 "residuals")
    const unsigned int *blob_len;         // [total_frames]
    const unsigned long long *clip_frame0;  // [n_clips] first frame of the clip
    const unsigned int *clip_frames;        // [n_clips] decodable frames of the clip
    const unsigned long long *clip_out;     // [n_clips] float offset of the clip's PCM in `out`
    int n_clips;
    int channels;                     // header channel count (output interleave)
    float *out;                       // (frames - 1) * 1024 * channels floats per clip, every one written
    int *error;                       // set to 1 when a frame cannot be deserialised
    int run;                          // output blocks per wavefront (set by the launcher)
    unsigned int n_runs;              // runs per clip (set by the launcher)
    unsigned int lead;                // frames in front of every clip's first frame in the frame list that belong to its file
                                      // (decode_frame_at: the file's earlier frames, for a channel its predecessor lacks)
    unsigned long long *dbg;          // FLO_DEC_STAMPS builds only: phase tick sums (set by the launcher)
    LossyWinArgs win;                 // corpus windows only (set by launch_lossy_window)
    LossyStreamArgs strm;             // streaming decoders only (set by launch_lossy_stream)
    LossyCmpArgs cmp;                 // fidelity reports only (launch_lossy_compare); `out` is not written then
};

// (LlChannelDev, LlFrameDev and the tile constants kRiceTileBits / kRiceStates / kRiceMaxK: ll_route.hpp)
struct LlDecArgs {
    const uint8_t *bytes;
    const LlChannelDev *ch;
    unsigned int n_ch;
    int *scratch;                     // decoded integers, one run per channel wrapper
    const int *only;                  // nullable [n_ch]: decode only the wrappers whose entry is nonzero
};

// Parallel form of the ALPC decode (lldec_kernels.hip). A Rice stream is cut into tiles of kRiceTileBits bits;
// `tile0` is the running tile count over the wrappers (0 tiles for raw / silent wrappers and for those the host
// already handed to the serial kernel through `serial`).
struct LlParArgs {
    const uint8_t *bytes;
    const LlChannelDev *ch;
    unsigned int n_ch;
    int *scratch;                     // residuals, then samples in place (every wrapper's kernels write all of its samples)
    const unsigned int *tile0;        // [n_ch + 1]
    unsigned int *tabs;               // [tiles][kRiceStates]: exit state | codes started << 5, per entry state
    uint2 *tile_entry;                // [tiles]: (index of the first code that starts in the tile, entry state)
    int *serial;                      // [n_ch] nonzero: the serial kernel decodes this wrapper (set by the host for
                                      // k > 14 or large coefficients, by the device for a 256-ones escape or a sample
                                      // outside i32)
    const unsigned int *others;       // [n_others] the wrappers that are no LPC recurrence (fixed predictors, raw, silent, too short): one
    unsigned int n_others;            // workgroup each in ll_predict behind the LPC groups (a workgroup per wrapper cost 0.2 ms in dispatch alone)
};
struct LlFinishArgs {
    const LlFrameDev *fr;
    const LlChannelDev *ch;
    unsigned int n_frames;
    int channels;
    const int *scratch;
    float *out;                       // zero-filled interleaved f32 (nullable)
    int *out_i32;                     // zero-filled interleaved i32 (nullable; parity tests)
};

// Zeros of every window past the end of its file: floats [first, end) of the window's slot.
struct WinTailDev {
    unsigned long long dst;           // float offset of the window's slot
    unsigned int first, end;
};
// Lossless windows: one item = one decoded frame of one window (a frame two windows touch is decoded once for each).
struct LlWinItem {
    unsigned long long dst;           // float offset of the sample-frame `from` lands on, in the window's slot
    unsigned int first_channel;       // the frame's wrappers in the call's wrapper list (scratch offsets in out_off)
    unsigned int n_channels;
    unsigned int from, count;         // sample-frames [from, from + count) of the frame go to the window
    unsigned int mid_side;
    unsigned int pad;
};
struct LlWinFinishArgs {
    const LlWinItem *items;
    const LlChannelDev *ch;
    unsigned int n_items;
    int channels;
    const int *scratch;
    float *out;
};

int launch_lossy_decode(const LossyDecArgs &A, unsigned max_frames, hipStream_t s);
int launch_ll_decode(const LlDecArgs &A, hipStream_t s);
int launch_ll_decode_parallel(const LlParArgs &A, unsigned max_tiles, hipStream_t s);
int launch_ll_finish(const LlFinishArgs &A, unsigned max_samples, hipStream_t s);
// corpus windows: runs of `run` blocks (<= 16), runs_per_window of them per window
int launch_lossy_window(const LossyDecArgs &A, const LossyWinArgs &W, unsigned run, hipStream_t s);
int launch_ll_window_finish(const LlWinFinishArgs &A, unsigned max_count, hipStream_t s);
// streaming decoders: one wavefront per run and channel
int launch_lossy_stream(const LossyDecArgs &A, const LossyStreamArgs &S, hipStream_t s);
int launch_window_tail(const WinTailDev *tails, unsigned n, float *out, hipStream_t s);
// fidelity reports: the grid of launch_lossy_decode, every block compared with A.cmp's sources instead of stored
int launch_lossy_compare(const LossyDecArgs &A, unsigned max_frames, hipStream_t s);

}  // namespace flo
