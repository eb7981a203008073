// ctx_internal.hpp — the context object and the host helpers that the library's source files share (flo_api.cpp owns
// the definitions; corpus.cpp uses them). Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/flo_hip.h"
#include "analysis_kernels.hpp"
#include "fidelity_kernels.hpp"
#include "lossy_device.hpp"
#include "stager.hpp"
#include "tables.hpp"

using namespace flo;

struct TableSet {
    LossyTablesHost host;
    void *blob = nullptr;  // one device allocation holding every table
    LossyDevTables dev{};
    const float *dev_window = nullptr;  // [2048], decode side
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

int fail(flo_ctx *c, int code, const std::string &msg);
// releases flo_ctx::sdec (sdec.cpp)
void sdec_work_free(flo_ctx *c);
// releases flo_ctx::lstream (lstream.cpp)
void lstream_work_free(flo_ctx *c);

// ---- streaming encoder (flo_stream_*: flo_api.cpp, the lossy stream step and flo_stream_encode_ready: lstream.cpp) --------
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
// items[i].second complete seconds, in one lossless batch; frames come back in item order (flo_api.cpp)
int stream_encode_lossless(flo_ctx *c, const std::vector<std::pair<flo_stream *, size_t>> &items, std::vector<std::vector<uint8_t>> &frames);
// queue the frames stream_encode_lossless made for `count` seconds of s and drop those seconds from its buffer
void stream_queue_lossless(flo_stream *s, std::vector<std::vector<uint8_t>> &frames, size_t first, size_t count);
#define HIPCHK(ctx, expr)                                                                               \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(ctx, FLO_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));        \
    } while (0)
int profile_drain(flo_ctx *c, bool wait);
// the constant tables of one sample rate (made on first use, kept by the context)
int get_tables(flo_ctx *c, uint32_t sr, float quality, TableSet **out);
// the context's pinned staging ring and copy threads (made on first use)
int ctx_stager(flo_ctx *c);

// ---- fidelity reports (fidelity.cpp): what flo_api.cpp, which owns batches and the file decode paths, lends them --------
// A synced batch as the comparison sees it: clip i's source is the batch's device copy, src_frames[i] whole frames at
// pcm + src_off[i]; dec_frames[i] is what its file decodes to. FLO_ERR_STATE before sync.
struct FidBatchView {
    flo_ctx *ctx = nullptr;
    bool lossy = false;
    int channels = 0;
    const float *pcm = nullptr;
    std::vector<unsigned long long> src_off, src_frames, dec_frames;
};
int batch_fidelity_view(flo_batch *b, FidBatchView &v);
// the fused pass over a synced lossy batch: lossy_decode_kernel<kDecCompare>, clip i against cmp's clip i (stream idle on return)
int batch_lossy_compare(flo_batch *b, const LossyCmpArgs &cmp);
// a parsed file whose bytes are at d_bytes: the fused pass of a transform file (one clip), the decode of a lossless one
// into d_out (its frames' samples x channels floats); both leave the stream idle
namespace flo {
struct ParsedFile;
}
int file_lossy_compare(flo_ctx *c, const ParsedFile &f, const uint8_t *d_bytes, const LossyCmpArgs &cmp);
int file_lossless_decode(flo_ctx *c, const ParsedFile &f, const uint8_t *d_bytes, float *d_out);

// Launch through `launch` on the ctx stream; with profiling on, bracketed by events under `name`.
template <typename F>
inline int timed_launch(flo_ctx *c, const char *name, F &&launch) {
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

