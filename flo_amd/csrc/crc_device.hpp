// crc_device.hpp — CRC32 (IEEE, reflected, init/xorout 0xFFFFFFFF) of DATA chunks already in HBM, shared by the finish
// kernels (container_kernels.hip: one workgroup of 256 threads per slice) and the idle tail of the stereo chain encode
// (lossy_kernels.hip: one wave per slice). Replaces core/crc32.rs:2-30 for chunks that live on the device.
//
// The CRC register after a message M from initial value I is (I x^(8n) + M(x) x^32) mod P: linear in I and in M. So a
// slice of the DATA chunk is cut into 64-byte blocks dealt round-robin to the NT threads (every load of the group is one
// NT * 64-byte contiguous stripe); a thread carries one register across its blocks, multiplying by x^(8 (NT * 64 - 64)) to
// skip the other threads' bytes (a 4 x 256 table per NT, like the byte tables), and at the end each register is moved to
// the end of the slice by x^(8 tail) and all are xor-ed together. CRC is exact GF(2) arithmetic: any thread count and
// any cut into slices give the same register. Products x^k * r mod P are 32-step shift-and-xor loops.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace flo {

constexpr uint32_t kPoly = 0xEDB88320u;

__host__ __device__ inline uint32_t multmodp(uint32_t a, uint32_t b) {   // a(x) * b(x) mod P, reflected bit order
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ kPoly : b >> 1;
    }
    return p;
}
__host__ __device__ inline uint32_t x8n_modp(unsigned long long n) {   // x^(8 n) mod P
    uint32_t sq = 0x00800000u;   // x^8 in the reflected representation (x^0 = 0x80000000)
    uint32_t p = 0x80000000u;
    while (n) {
        if (n & 1ull) p = multmodp(sq, p);
        sq = multmodp(sq, sq);
        n >>= 1;
    }
    return p;
}

constexpr unsigned kBlk = 64;                   // bytes a thread consumes per stripe
constexpr unsigned kSliceAlign = 256 * kBlk;    // 16 KiB: slices of a clip start on multiples of this

// Device table of the CRC code (crc_device_tables), in u32 words:
constexpr unsigned kCrcTabByte = 0;             // tab[4][256]: slicing-by-4 byte tables (crc32.rs:2-20 builds the first)
constexpr unsigned kCrcTabSkip256 = 1024;       // skip[4][256]: multiplication by x^(8 (256 * 64 - 64)), 256 threads
constexpr unsigned kCrcTabSkip64 = 2048;        // ... by x^(8 (64 * 64 - 64)), one wave
constexpr unsigned kCrcTabBlkPow = 3072;        // [256] x^(8 * 64 * i)
constexpr unsigned kCrcTabBytePow = 3328;       // [64] x^(8 * i)
constexpr unsigned kCrcTabWords = 3392;

// slice `part` of `parts` of an n-byte chunk: [beg, beg + len)
__device__ __forceinline__ void crc_slice_range(unsigned long long n, unsigned parts, unsigned part, unsigned long long &beg,
                                                unsigned long long &len) {
    unsigned long long s = (n + parts - 1) / parts;
    s = (s + kSliceAlign - 1) / kSliceAlign * kSliceAlign;
    beg = (unsigned long long)part * s < n ? (unsigned long long)part * s : n;
    len = beg + s < n ? s : n - beg;
}

// CRC register (initial value 0) of the n bytes at `data` (16-byte aligned), computed by the NT threads t = 0 .. NT-1 of
// a wave (NT = 64) or a workgroup (NT = 256). tab / skip: the byte tables and this NT's skip table, in LDS (every thread
// must see them filled); blk_pow / byte_pow: x^(8 * 64 * i) and x^(8 * i). s_red: NT / 64 words of LDS when NT > 64 (the
// call ends in a barrier then). The result is valid in thread 0.
template <int NT>
__device__ __forceinline__ uint32_t crc_slice_reg(const uint32_t (*tab)[256], const uint32_t (*skip)[256], const unsigned *blk_pow,
                                                  const unsigned *byte_pow, const uint8_t *data, unsigned long long n,
                                                  const unsigned t, uint32_t *s_red) {
    static_assert(NT % 64 == 0 && NT <= 256, "thread count: whole waves, at most 256");
    constexpr unsigned kStripe = NT * kBlk;
    const unsigned long long full = n / kStripe;          // complete stripes
    const unsigned long long rem0 = full * kStripe;       // first byte behind them
    const unsigned rem = (unsigned)(n - rem0);
    const unsigned nb = rem / kBlk, last = rem % kBlk;
    auto eat = [&](uint32_t reg, const uint8_t *p, unsigned bytes) {   // bytes is a multiple of 4, p 4-byte aligned
        for (unsigned i = 0; i < bytes; i += 4) {
            const uint32_t w = *reinterpret_cast<const uint32_t *>(p + i) ^ reg;
            reg = tab[3][w & 0xFFu] ^ tab[2][(w >> 8) & 0xFFu] ^ tab[1][(w >> 16) & 0xFFu] ^ tab[0][w >> 24];
        }
        return reg;
    };
    const uint32_t pw_last = byte_pow[last];
    uint32_t acc = 0;
    if (full) {
        uint32_t reg = 0;
        const uint8_t *p = data + (unsigned long long)t * kBlk;
        for (unsigned long long sidx = 0; sidx < full; sidx++, p += kStripe) {
            reg = skip[0][reg & 0xFFu] ^ skip[1][(reg >> 8) & 0xFFu] ^ skip[2][(reg >> 16) & 0xFFu] ^ skip[3][reg >> 24];
            const uint4 a = *reinterpret_cast<const uint4 *>(p), b = *reinterpret_cast<const uint4 *>(p + 16),
                        c = *reinterpret_cast<const uint4 *>(p + 32), d = *reinterpret_cast<const uint4 *>(p + 48);
            const uint32_t w[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint32_t v = w[i] ^ reg;
                reg = tab[3][v & 0xFFu] ^ tab[2][(v >> 8) & 0xFFu] ^ tab[1][(v >> 16) & 0xFFu] ^ tab[0][v >> 24];
            }
        }
        // the register now stands behind this thread's block of the last complete stripe
        // ... and moves to the end of the slice: x^(8 (64 (NT - 1 - t) + rem)) = x^(8 * 64 (NT - 1 - t + nb)) x^(8 last)
        acc = multmodp(multmodp(blk_pow[NT - 1 - t], multmodp(blk_pow[nb], pw_last)), reg);
    }
    {   // the incomplete stripe: one 64-byte block per thread, then the last < 64 bytes on thread 0
        if (t < nb) {
            const uint32_t reg = eat(0, data + rem0 + (unsigned long long)t * kBlk, kBlk);
            acc ^= multmodp(multmodp(blk_pow[nb - 1 - t], pw_last), reg);
        }
        if (t == 0) {
            uint32_t reg = 0;
            const uint8_t *p = data + rem0 + (unsigned long long)nb * kBlk;
            for (unsigned i = 0; i < last; i++) reg = tab[0][(reg ^ p[i]) & 0xFFu] ^ (reg >> 8);
            acc ^= reg;
        }
    }
    for (int d = 32; d > 0; d >>= 1) acc ^= __shfl_down(acc, d);
    if (NT > 64) {
        if ((t & 63) == 0) s_red[t >> 6] = acc;
        __syncthreads();
        if (t == 0)
            for (int k = 1; k < NT / 64; k++) acc ^= s_red[k];
        __syncthreads();   // s_red may be reused by the caller's next slice
    }
    return acc;
}

}  // namespace flo
