// file_layout.hpp — the shape of a finished .flo file as the encoders leave it in device memory, and what the host does to
// it on the way out: header (writer.rs:132-224) + TOC right in front of the 16-byte aligned DATA chunk; META, if any, is
// appended on the host, which then patches meta_size. Plain C++: no HIP headers, so a host test builds it with g++ alone
// (tests/native/file_layout_test.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace flo {

constexpr uint64_t kFileHeaderBytes = 74;   // magic .. meta_size (70) and the TOC's entry count (4)
constexpr uint64_t kTocEntryBytes = 20;     // per frame: index u32, offset u64, size u32, timestamp u32
constexpr size_t kBitDepthByte = 13;
constexpr size_t kMetaSizeByte = 62;        // meta_size: 8 bytes, little-endian

// bytes in front of a file's DATA chunk
constexpr uint64_t head_bytes(uint64_t frames) { return kFileHeaderBytes + kTocEntryBytes * frames; }
// frames of a lossy clip: one priming hop in front, the tail padded to whole hops (encoder.rs:177-179)
constexpr uint64_t lossy_hops(uint64_t sample_frames) { return (sample_frames + 1024 + 1023) / 1024; }
constexpr uint64_t align16(uint64_t x) { return (x + 15) & ~(uint64_t)15; }

// Where the next file of a buffer comes to lie: DATA (room for data_cap bytes) at the first 16-byte aligned place that
// leaves room for header + TOC right in front of it; the cursor moves behind the DATA chunk's room.
struct FilePlace {
    uint64_t file_off, data_off;   // file_off = data_off - head_bytes(frames)
};
inline FilePlace place_file(uint64_t &cursor, uint64_t frames, uint64_t data_cap) {
    const uint64_t head = head_bytes(frames), data_off = cursor + align16(head);
    cursor = data_off + align16(data_cap);
    return {data_off - head, data_off};
}

// n blobs packed one behind the other at 16-byte aligned offsets (a size of 0 takes no room); returns the bytes in all.
// offsets: [n], or null when only the total is wanted.
inline uint64_t packed_offsets(const uint64_t *sizes, size_t n, uint64_t *offsets) {
    uint64_t pos = 0;
    for (size_t k = 0; k < n; k++) {
        if (offsets) offsets[k] = pos;
        pos += align16(sizes[k]);
    }
    return pos;
}

// META behind the n bytes of a finished file (room for n + meta_len), and its length into the header
inline void attach_meta(uint8_t *file, size_t n, const uint8_t *meta, size_t meta_len) {
    if (meta_len) memcpy(file + n, meta, meta_len);
    for (int i = 0; i < 8; i++) file[kMetaSizeByte + i] = (uint8_t)((uint64_t)meta_len >> (8 * i));
}
inline void set_bit_depth(uint8_t *file, uint8_t depth) { file[kBitDepthByte] = depth; }

}  // namespace flo
