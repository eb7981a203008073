// ctx_internal.hpp — the context object and the host helpers that the library's source files share; every declaration
// names the file that defines it. Not part of the C ABI. (struct flo_batch: batch_internal.hpp; the scoped device blocks:
// devmem.hpp.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/flo_hip.h"
#include "analysis_kernels.hpp"
#include "fidelity_kernels.hpp"
#include "file_layout.hpp"
#include "lossy_device.hpp"
#include "stager.hpp"
#include "stream_delay.hpp"
#include "tables.hpp"

using namespace flo;

struct TableSet {
    LossyTablesHost host;
    void *blob = nullptr;  // one device allocation holding every table
    LossyDevTables dev{};
    const float *dev_window = nullptr;  // [2048], decode side
    const StatMasks *dev_masks = nullptr;  // host.masks on the device (the lock-step stereo chain form's band statistics and bands' hearing floors)
};

struct ProfRec {
    std::string name;
    hipEvent_t a, b;
};
struct ProfSum {   // launches already read out (their events are destroyed)
    double ms = 0;
    uint64_t n = 0;
};

struct flo_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    std::vector<TableSet *> tables;
    bool profile = false;
    std::vector<ProfRec> prof;              // bracketed launches not yet read out
    std::map<std::string, ProfSum> prof_sum;
    int force_path = 0;
    hipDeviceProp_t prop{};
    Stager *stager = nullptr;   // pinned staging ring + copy threads of the host-buffer entry points (made on first use)
    hipStream_t up_stream = nullptr, down_stream = nullptr;   // uploads / downloads of flo_encode_batch's pipeline
    int reserve_cus = -1;   // compute units the persistent chain kernel leaves free (-1: not set; see flo_ctx_reserve_cus)
    AnalysisSide an_side;   // side streams of the analysis (made on first use)
    bool an_side_ready = false;
    struct SdecWork *sdec = nullptr;   // flo_sdec_decode_ready's staging slots and scratch (sdec.cpp; made on first use)
    struct LstreamWork *lstream = nullptr;   // flo_stream_encode_ready's device scratch (lstream.cpp; made on first use)
};

// sets the context's error text and returns `code` (context.cpp)
int fail(flo_ctx *c, int code, const std::string &msg);
// the message of an entry point that has no context: into the caller's buffer (nullable), cut to its size
inline void put_err(char *err, size_t cap, const std::string &m) {
    if (err && cap) {
        strncpy(err, m.c_str(), cap - 1);
        err[cap - 1] = 0;
    }
}
// the text behind flo_last_create_error: failures that have no context to carry it (context.cpp)
extern thread_local std::string g_create_err;
// releases flo_ctx::sdec (sdec.cpp)
void sdec_work_free(flo_ctx *c);
// releases flo_ctx::lstream (lstream.cpp)
void lstream_work_free(flo_ctx *c);

// ---- streaming encoder (flo_stream_*: stream.cpp, the lossy stream step and flo_stream_encode_ready: lstream.cpp) ---------
struct StreamFrame {
    uint32_t index, timestamp_ms, samples;
    std::vector<uint8_t> data;
};
struct flo_stream {
    flo_ctx *ctx = nullptr;
    uint32_t sr = 0;
    uint8_t ch = 0, bit_depth = 16, level = 5;
    std::vector<float> buf;   // pushed samples not yet encoded (lossy: not yet the second half of an encoded frame)
    std::vector<StreamFrame> pending;
    uint64_t total_samples = 0;
    uint32_t frame_index = 0;
    // lossy stream (flo_stream_create_lossy): the state the encoder carries from frame to frame
    bool lossy = false;
    bool flushed = false;      // flush / finalize ended the input
    float quality = 0.f;       // clamped to [0, 1]
    std::vector<float> carry;  // [1024 * ch]: the last 1024 sample-frames of the input seen (zeros: the pre-roll)
    std::vector<float> mask;   // [ch * 25]: temporal masking level after the last encoded frame
};
// the lossless frames of many streams of one (sample rate, channels, bit depth, level): stream items[i].first's next
// items[i].second complete seconds, in one lossless batch; frames come back in item order (stream.cpp)
int stream_encode_lossless(flo_ctx *c, const std::vector<std::pair<flo_stream *, size_t>> &items, std::vector<std::vector<uint8_t>> &frames);
// queue the frames stream_encode_lossless made for `count` seconds of s and drop those seconds from its buffer (stream.cpp)
void stream_queue_lossless(flo_stream *s, std::vector<std::vector<uint8_t>> &frames, size_t first, size_t count);
// a lossy stream's share of flo_stream_push, and the end of its input: the trailing frames join the queue (lstream.cpp)
int lossy_stream_push(flo_stream *s, const float *samples, size_t n);
int lossy_stream_end(flo_stream *s);
#define HIPCHK(ctx, expr)                                                                               \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(ctx, FLO_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));        \
    } while (0)
// ... for functions that must release something on the way out: returns leave(code), and tells out-of-memory apart
#define HIPCHK_OR(ctx, expr, leave)                                                                     \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return leave(fail(ctx, e_ == hipErrorOutOfMemory ? FLO_ERR_NOMEM : FLO_ERR_DEVICE,          \
                              std::string(#expr) + ": " + hipGetErrorString(e_)));                      \
    } while (0)
// A finished file out of device memory (n bytes at d_file) as a malloc'd block with META attached (file_layout.hpp);
// bit_depth >= 0 goes into the header as well. Errors read "<what>: <HIP's text>" (context.cpp)
int fetch_file(flo_ctx *c, const uint8_t *d_file, size_t n, const uint8_t *meta, size_t meta_len, int bit_depth, const char *what,
               uint8_t **out, size_t *out_len);
// folds every finished profiling bracket (wait: every bracket) into the per-kernel sums (context.cpp)
int profile_drain(flo_ctx *c, bool wait);
// the constant tables of one sample rate (made on first use, kept by the context; context.cpp)
int get_tables(flo_ctx *c, uint32_t sr, float quality, TableSet **out);
// the context's pinned staging ring and copy threads (made on first use; context.cpp)
int ctx_stager(flo_ctx *c);

// ---- decode (decode.cpp): the device paths of flo_decode, which the fidelity reports (fidelity.cpp) run as well --------
namespace flo {
struct ParsedFile;
}
struct LlWrapperList;   // decode_plan.hpp
// the transform blobs of a parsed file, in order (decode_transform_file, lib.rs:325-352: frames without channels are skipped)
void file_transform_blobs(const ParsedFile &f, std::vector<unsigned long long> &blob_off, std::vector<unsigned int> &blob_len);
// the wrappers of every frame of a parsed lossless file, frame after frame in the output; returns the sample-frames in all
uint64_t file_ll_wrappers(const ParsedFile &f, LlWrapperList &w);
// Enqueue the decode of `w` (out_sf sample-frames) on the ctx stream: integers per wrapper into a scratch, then
// mid/side, interleave and the 1/32767 scale into d_out (f32, nullable) / d_out_i32 (nullable), both out_sf * nch
// elements. Returns when the kernels have run.
int ll_decode_device(flo_ctx *c, const LlWrapperList &w, uint64_t out_sf, const uint8_t *d_bytes, int nch, float *d_out, int *d_out_i32);
// lossy_decode_kernel<kDecWhole> over the clips whose bytes sit at `bytes`: the frame and clip tables and a cleared
// error word go up, the kernel runs, the error word comes back (the ctx stream is idle on return). FLO_ERR_FORMAT when a
// frame does not deserialise. With `cmp` (fidelity reports), lossy_decode_kernel<kDecCompare>: clip i is compared with
// cmp's clip i and nothing is written to `out`.
int lossy_decode_whole(flo_ctx *c, const TableSet *ts, const uint8_t *bytes, int channels, const std::vector<unsigned long long> &blob_off,
                       const std::vector<unsigned int> &blob_len, const std::vector<unsigned long long> &clip_frame0,
                       const std::vector<unsigned int> &clip_frames, const std::vector<unsigned long long> &clip_out,
                       unsigned max_frames, float *out, const LossyCmpArgs *cmp = nullptr, unsigned lead = 0);

// Launch through `launch` on the ctx stream; with profiling on, bracketed by events under `name`.
template <typename F>
inline int timed_launch(flo_ctx *c, const char *name, F &&launch) {
    HIPCHK(c, stream_delay(c->stream));   // (flo_debug_stream_delay: off, one relaxed load)
    if (!c->profile) {
        int rc = launch();
        return rc == 0 ? FLO_OK : fail(c, FLO_ERR_DEVICE, std::string("launch ") + name + " failed: " +
                                                              hipGetErrorString((hipError_t)(rc > 0 ? rc : 1)));
    }
    if (c->prof.size() >= 256) {   // bound the queue of live events
        int drc = profile_drain(c, false);
        if (drc != FLO_OK) return drc;
    }
    ProfRec r;
    r.name = name;
    HIPCHK(c, hipEventCreate(&r.a));
    HIPCHK(c, hipEventCreate(&r.b));
    HIPCHK(c, hipEventRecord(r.a, c->stream));
    int rc = launch();
    HIPCHK(c, hipEventRecord(r.b, c->stream));
    c->prof.push_back(r);
    return rc == 0 ? FLO_OK : fail(c, FLO_ERR_DEVICE, std::string("launch ") + name + " failed");
}

