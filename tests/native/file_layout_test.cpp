// file_layout_test.cpp — the shape of a finished file in device memory and what the host does to it on the way out
// (flo_amd/csrc/file_layout.hpp) on the host. Prints "ok <checks>" and returns 0, or names the first case that fails.
#include <cstdio>
#include <vector>

#include "../../flo_amd/csrc/file_layout.hpp"

static int g_checks = 0;
static bool g_ok = true;

static void check(bool cond, const char *what) {
    g_checks++;
    if (!cond && g_ok) fprintf(stderr, "%s\n", what);
    g_ok = g_ok && cond;
}

// a "file" of n bytes of a known pattern with room for META behind it, and two guard bytes behind that
static std::vector<uint8_t> pattern(size_t n) {
    std::vector<uint8_t> f(n);
    for (size_t i = 0; i < n; i++) f[i] = (uint8_t)(0xA5 ^ (i * 7));
    return f;
}

int main() {
    using namespace flo;
    check(kFileHeaderBytes == 74 && kTocEntryBytes == 20 && kBitDepthByte == 13 && kMetaSizeByte == 62, "constants");
    check(head_bytes(0) == 74, "head_bytes(0)");
    check(head_bytes(1) == 94, "head_bytes(1)");
    check(head_bytes(45) == 974, "head_bytes(45)");
    {   // one priming hop, the tail padded to whole hops (encoder.rs:177-179)
        const uint64_t sf[] = {0, 1, 1023, 1024, 1025}, want[] = {1, 2, 2, 2, 3};
        for (int i = 0; i < 5; i++) check(lossy_hops(sf[i]) == want[i], "lossy_hops");
    }
    {   // placement from cursor 0: DATA aligned, header + TOC right in front, no file overlaps the one before
        const uint64_t frames[] = {1, 2, 45}, cap[] = {64, 0, 4096};
        uint64_t cursor = 0, prev_end = 0;
        for (int i = 0; i < 3; i++) {
            const FilePlace at = place_file(cursor, frames[i], cap[i]);
            if (i == 0) check(at.file_off == 2 && at.data_off == 96, "first file at 2 / 96");
            check(at.data_off % 16 == 0, "data_off aligned");
            check(at.file_off + head_bytes(frames[i]) == at.data_off, "head right in front of DATA");
            check(at.file_off >= prev_end, "no overlap with the file before");
            check(cursor >= at.data_off + cap[i], "cursor behind the DATA chunk's room");
            prev_end = at.data_off + cap[i];
        }
        check(cursor == 96 + 64 + 128 + 0 + 976 + 4096, "cursor in all");
    }
    {   // a capacity that is no multiple of 16 still leaves the next DATA chunk aligned
        uint64_t cursor = 0;
        place_file(cursor, 1, 17);
        const FilePlace at = place_file(cursor, 1, 1);
        check(at.data_off % 16 == 0 && at.file_off >= 96 + 17, "odd capacity");
    }
    {   // packed offsets: multiples of 16, no overlap, sizes of 0 take no room
        const std::vector<uint64_t> sizes = {94, 0, 16, 17, 4096, 1};
        std::vector<uint64_t> off(sizes.size());
        const uint64_t total = packed_offsets(sizes.data(), sizes.size(), off.data());
        const std::vector<uint64_t> want = {0, 96, 96, 112, 144, 4240};
        check(off == want && total == 4256, "packed_offsets");
        check(packed_offsets(sizes.data(), sizes.size(), nullptr) == 4256, "packed_offsets, total only");
        check(packed_offsets(nullptr, 0, nullptr) == 0, "packed_offsets of nothing");
    }
    for (size_t meta_len : {(size_t)0, (size_t)1, (size_t)258}) {
        const size_t n = 200;
        const std::vector<uint8_t> before = pattern(n + meta_len + 2);
        std::vector<uint8_t> f = before, meta(meta_len);
        for (size_t i = 0; i < meta_len; i++) meta[i] = (uint8_t)(i + 1);
        attach_meta(f.data(), n, meta_len ? meta.data() : nullptr, meta_len);
        bool size_ok = true, rest_ok = true, meta_ok = true;
        for (size_t i = 0; i < 8; i++) size_ok = size_ok && f[62 + i] == (uint8_t)((uint64_t)meta_len >> (8 * i));
        for (size_t i = 0; i < n; i++) rest_ok = rest_ok && ((i >= 62 && i < 70) || f[i] == before[i]);
        for (size_t i = 0; i < meta_len; i++) meta_ok = meta_ok && f[n + i] == meta[i];
        check(size_ok, "attach_meta: meta_size little-endian at 62..69");
        check(rest_ok, "attach_meta: bytes outside 62..69 untouched");
        check(meta_ok, "attach_meta: META behind the file");
        check(f[n + meta_len] == before[n + meta_len] && f[n + meta_len + 1] == before[n + meta_len + 1], "attach_meta: tail untouched");
    }
    {
        const std::vector<uint8_t> before = pattern(74);
        std::vector<uint8_t> f = before;
        set_bit_depth(f.data(), 24);
        bool rest_ok = f[13] == 24;
        for (size_t i = 0; i < f.size(); i++) rest_ok = rest_ok && (i == 13 || f[i] == before[i]);
        check(rest_ok, "set_bit_depth touches byte 13 only");
    }
    if (!g_ok) return 1;
    printf("ok %d\n", g_checks);
    return 0;
}
