// seeking.cpp — the host half of libflo's seeking API (libflo/src/seeking.rs): the TOC and the time -> frame search. Both
// are pure container reads; flo_decode_frame_at (decode.cpp) decodes on the device.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/flo_hip.h"
#include "container.hpp"

using namespace flo;

static int seek_fail(char *err, size_t err_cap, const char *msg) {
    if (err && err_cap) snprintf(err, err_cap, "%s", msg);
    return FLO_ERR_FORMAT;
}

extern "C" int flo_get_toc(const uint8_t *flo, size_t len, flo_toc_entry **entries, size_t *n, char *err, size_t err_cap) {
    if (!entries || !n || (!flo && len)) return FLO_ERR_ARG;
    *entries = nullptr;
    *n = 0;
    if (err && err_cap) err[0] = 0;
    ParsedFile f;
    const char *perr = "";
    if (parse_file(flo, len, f, &perr) != 0) return seek_fail(err, err_cap, perr);
    if (f.toc.empty()) return FLO_OK;
    flo_toc_entry *e = (flo_toc_entry *)malloc(f.toc.size() * sizeof(flo_toc_entry));
    if (!e) return FLO_ERR_NOMEM;
    for (size_t i = 0; i < f.toc.size(); i++) {
        e[i] = flo_toc_entry{};
        e[i].frame_index = f.toc[i].frame_index;
        e[i].frame_size = f.toc[i].frame_size;
        e[i].byte_offset = f.toc[i].byte_offset;
        e[i].timestamp_ms = f.toc[i].timestamp_ms;
    }
    *entries = e;
    *n = f.toc.size();
    return FLO_OK;
}

extern "C" int flo_seek_to_time(const uint8_t *flo, size_t len, uint32_t target_ms, flo_seek_result *out, char *err,
                                size_t err_cap) {
    if (!out || (!flo && len)) return FLO_ERR_ARG;
    memset(out, 0, sizeof *out);
    if (err && err_cap) err[0] = 0;
    ParsedFile f;
    const char *perr = "";
    if (parse_file(flo, len, f, &perr) != 0) return seek_fail(err, err_cap, perr);
    const std::vector<TocDesc> &toc = f.toc;
    if (toc.empty()) return seek_fail(err, err_cap, "No TOC available for seeking");
    // binary_search_frame (seeking.rs:136-159): the rightmost entry with timestamp_ms <= target_ms (0 if there is none)
    size_t left = 0, right = toc.size() - 1;
    while (left < right) {
        const size_t mid = left + (right - left + 1) / 2;
        if (toc[mid].timestamp_ms <= target_ms) left = mid;
        else right = mid - 1;
    }
    uint32_t fi = (uint32_t)left;
    // clamp to the frames read (seeking.rs:87-90); with no frame read the reference's `len() - 1` underflows
    if (f.frames.empty()) return seek_fail(err, err_cap, "No frames available for seeking");
    if ((size_t)fi >= f.frames.size()) fi = (uint32_t)(f.frames.size() - 1);
    const TocDesc &e = toc[fi];
    const bool has_next = (uint64_t)fi + 1 < (uint64_t)(uint32_t)toc.size();
    uint32_t frame_duration_ms = 0;
    if (has_next) {
        frame_duration_ms = toc[fi + 1].timestamp_ms - e.timestamp_ms;   // (u32: wraps as a release build does)
    } else {
        if (f.sample_rate == 0) return seek_fail(err, err_cap, "Invalid sample rate for seeking");   // the reference divides by zero
        frame_duration_ms = (uint32_t)(((uint64_t)f.frames[fi].samples * 1000u) / (uint64_t)f.sample_rate);
    }
    const uint32_t ms_into = target_ms > e.timestamp_ms ? target_ms - e.timestamp_ms : 0u;   // saturating_sub
    uint32_t sample_offset = (uint32_t)(((uint64_t)ms_into * (uint64_t)f.sample_rate) / 1000u);
    if (sample_offset > f.frames[fi].samples) sample_offset = f.frames[fi].samples;
    out->frame_index = fi;
    out->byte_offset = e.byte_offset;
    out->timestamp_ms = e.timestamp_ms;
    out->sample_offset = sample_offset;
    out->next_timestamp_ms = has_next ? toc[fi + 1].timestamp_ms : e.timestamp_ms + frame_duration_ms;
    return FLO_OK;
}
