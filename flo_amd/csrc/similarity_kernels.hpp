// similarity_kernels.hpp — spectral similarity of fingerprint sets (flo_fpindex_*, similarity.cpp): the device record,
// the score as the reference computes it (core/analysis.rs:395-437), the cheap upper bound of the pair kernels, and the
// launch wrappers of similarity_kernels.hip. The score and the bound are __host__ __device__: flo_spectral_similarity
// and the kernels run the same lines.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace flo {

// One fingerprint on the device, 32 bytes (8 words), made once on the host:
//   w[0..3]  energy_profile[16], byte k of the profile in byte k % 4 of word k / 4
//   w[4..5]  frequency_peaks[8], the same packing
//   w[6]     avg_loudness in bits 0-7, the format id of (sample_rate, channels) in bits 8-31
//   w[7]     hash id: equal ids <=> equal 32-byte hashes
struct FpRec {
    uint32_t w[8];
};
constexpr uint32_t kFpFmtNone = 0xFFFFFFu;     // format id of a query whose format no member has
constexpr uint32_t kFpHashNone = 0xFFFFFFFFu;  // hash id of a query whose hash no member has
constexpr int kFpTile = 256;                   // queries per workgroup (one per lane) = references per LDS tile
constexpr int kFpMaxK = 64;

// fl(1.0f - fl(d / 255.0f)) for d = 0..255, the reference's term `1.0 - |a - b| / 255.0` (built on the host with
// contraction off, correctly rounded division; read from LDS by the kernels)
void fp_term_table(float *t);

// The score's three chains for two records of one format and different hashes, in the reference's order: the 16 and
// 8 terms summed left to right from 0 (Iterator::sum), each sum divided by its length, then
// fl(fl(fl(e * 0.5) + fl(p * 0.3)) + fl(l * 0.2)). Needs -ffp-contract=off (both the Makefile's device flags and the
// rule of similarity.cpp have it).
__host__ __device__ inline float fp_chain_score(const uint32_t *a, const uint32_t *b, const float *T) {
    float e = 0.0f, p = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int d = (int)((a[k >> 2] >> (8 * (k & 3))) & 255u) - (int)((b[k >> 2] >> (8 * (k & 3))) & 255u);
        e = e + T[d < 0 ? -d : d];
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int d = (int)((a[4 + (k >> 2)] >> (8 * (k & 3))) & 255u) - (int)((b[4 + (k >> 2)] >> (8 * (k & 3))) & 255u);
        p = p + T[d < 0 ? -d : d];
    }
    const int dl = (int)(a[6] & 255u) - (int)(b[6] & 255u);
    const float l = T[dl < 0 ? -dl : dl];
    e = e / 16.0f;
    p = p / 8.0f;
    const float x = e * 0.5f, y = p * 0.3f, z = l * 0.2f;
    const float xy = x + y;
    return xy + z;
}

// spectral_similarity (analysis.rs:395-437) on two records: equal hashes first, then the format check, then the chains
__host__ __device__ inline float fp_score(const uint32_t *a, const uint32_t *b, const float *T) {
    if (a[7] == b[7]) return 1.0f;
    if ((a[6] >> 8) != (b[6] >> 8)) return 0.0f;
    return fp_chain_score(a, b, T);
}

// ---- the cheap bound ---------------------------------------------------------------------------------------------------
// With SAD_e = sum |ea_k - eb_k| over the 16 energy bytes, SAD_p over the 8 peak bytes and D_l = |la - lb|, the real-valued
// score (exact arithmetic, exact weights 0.5 / 0.3 / 0.2) is
//     R = 0.5 (1 - SAD_e / (16 * 255)) + 0.3 (1 - SAD_p / (8 * 255)) + 0.2 (1 - D_l / 255) = 1 - K / 40800,
//     K = 5 SAD_e + 6 SAD_p + 32 D_l   (an integer in 0 .. 40800).
// Claim: |s - R| <= 11 u for the f32 score s of fp_chain_score, u = 2^-24 (round to nearest, no underflow: every
// intermediate is 0 or >= 2^-9). Proof, with |fl(x) - x| <= u |x|:
//   terms   t = fl(1 - fl(d / 255)):  |fl(d/255) - d/255| <= u, |t - (1 - fl(d/255))| <= u, so |t - (1 - d/255)| <= 2u.
//   sums    n terms in [0, 1], added left to right: the i-th partial sum is <= i, its addition errs by <= i u, so the
//           sum errs by <= u (2 + ... + n) + 2u n: 167u for n = 16, 51u for n = 8.
//   e       fl(S_e / 16), fl(e * 0.5) are exact (powers of two): the e term errs by <= 167u / 32 < 5.3u.
//   p       fl(S_p / 8) exact, error <= 51u / 8 < 6.4u; times 0.3f (|0.3f - 0.3| < 0.21u) and rounded (<= 0.31u):
//           <= 0.3 * 6.4u + 0.21u + 0.31u < 2.5u.
//   l       2u * 0.2 + |0.2f - 0.2| (< 0.05u) + rounding of the product (<= 0.21u) < 0.7u.
//   adds    fl(x + y) <= 0.81 errs by <= 0.81u, the last addition (<= 1.01) by <= 1.01u.
//   Sum: 5.3 + 2.5 + 0.7 + 0.81 + 1.01 < 11 u.
// fp_bound evaluates U = fl(fl(1 - fl(K * c)) + 2^-17) with c = fl(1 / 40800): fl(K * c) is within K |c - 1/40800| +
// u K c <= 2u of K / 40800, so fl(1 - fl(K c)) is within 3u of R (one more rounding, of a value <= 1), and adding
// 2^-17 = 128u (rounded, <= u more) gives U >= R + 124u > s. So s <= U for every pair of one format and different
// hashes; the kernels compute s only where U can still change a result (U >= the lane's k-th score, or U >= threshold).
// Since K steps by 1 / 40800 = 411u and U - R, R - s stay below 132u + 11u, a pair whose K exceeds the K of the lane's
// k-th entry is always rejected: the filter computes exact scores only for the ties and near-ties of K.
// tests/test_similarity_cpu.py checks the claim on random and permuted pairs.
__host__ __device__ inline uint32_t fp_bound_key(uint32_t sad_e, uint32_t sad_p, uint32_t dl) {
    return 5u * sad_e + 6u * sad_p + 32u * dl;
}
__host__ __device__ inline float fp_bound(uint32_t key) {
    const float c = 1.0f / 40800.0f;
    const float r = 1.0f - (float)key * c;
    return r + 0x1p-17f;
}

// ---- launches (similarity_kernels.hip) ----------------------------------------------------------------------------------
struct FpTopkArgs {
    const FpRec *q;          // [n_q] queries (== ref for a self-join)
    const FpRec *ref;        // [n_ref]
    const float *table;      // [256] fp_term_table
    uint32_t n_q, n_ref;
    uint32_t chunk;          // references per chunk (a multiple of kFpTile); grid.y = ceil(n_ref / chunk)
    uint32_t k;              // 1 .. kFpMaxK
    uint32_t self;           // 1: query i never lists reference i
    uint32_t *part_idx;      // [n_chunks][n_q][k] per-chunk lists, best first
    float *part_score;
};
// per-chunk top-k lists, then pairwise merges of the chunk lists until one remains; the result lands in out_* [n_q][k].
// scratch_*: [ceil(n_chunks / 2)][n_q][k] each (unused with one chunk)
int launch_fp_topk(const FpTopkArgs &a, uint32_t *out_idx, float *out_score, uint32_t *scratch_idx, float *scratch_score,
                   hipStream_t s);

struct FpPairsArgs {
    const FpRec *rec;        // [n] members
    const float *table;
    uint32_t n, chunk;       // chunk as above; grid.y = n_chunks
    float threshold;
    uint32_t *count;         // [n][n_chunks] count pass: pairs (i, j > i) of chunk c with score >= threshold
    const unsigned long long *off;   // [n][n_chunks] write pass: exclusive prefix of count (row-major)
    uint64_t cap;            // write pass: entries of i/j/score; pairs at offsets >= cap are not written
    uint32_t *pi, *pj;
    float *ps;
};
int launch_fp_pairs_count(const FpPairsArgs &a, hipStream_t s);
int launch_fp_pairs_write(const FpPairsArgs &a, hipStream_t s);

}  // namespace flo
