// similarity_kernels.hip — spectral similarity over fingerprint sets (flo_fpindex_*): top-k neighbours and threshold pairs
// under spectral_similarity (core/analysis.rs:395-437), every score bit for bit the reference's.
//
// Pair tile: a workgroup of kFpTile lanes owns kFpTile queries, one per lane, their 32-byte records in registers, and
// walks one CHUNK of the references (grid.y) in tiles of kFpTile records staged in LDS as whole 16-byte rows. Every lane
// reads the same row at the same time: ds_read_b128 broadcasts, no bank conflicts. Per pair the lane forms the integer key
// K of the cheap bound with v_sad_u8 (six instructions over the 24 bytes, the loudness byte through the format bytes,
// which are equal whenever the bound is used), turns it into the upper bound U (similarity_kernels.hpp) and computes the
// exact ordered-chain score only where U can still change the result. The term table (fl(1 - fl(d / 255))) sits in LDS.
//
// Top-k, k <= 16: each lane keeps its list sorted best first in registers, KM entries (KM = 4 or 16 by k): the last k
// of them are the list, the first KM - k are pinned at score 2 and never move. A candidate bubbles in from the top in KM
// compare-and-swap steps (static register indices); the lane's k-th entry is always es[KM - 1]. k = 17 .. 64 would not
// fit in registers (64 entries spill): fp_topk_lds_kernel keeps the lists in LDS, [slot][lane] so that a wave's accesses
// to one slot hit 64 different banks, in workgroups of 64 lanes (32 KiB of lists), the k-th entry mirrored in registers.
// Within a chunk the references come in ascending index order, so a candidate ties the k-th only against an empty slot.
// fp_merge_kernel then merges the chunks' lists pairwise under the ranking rule (score descending, index ascending) until one list is left:
// the result depends on neither the chunking nor the tile size.
//
// Pairs: the same walk over j > i counts, per (row, chunk), the pairs at or above the threshold; the host forms the
// exclusive prefix and a second walk writes (i, j, score) at the row's offset in j order: output ordered by (i, j).
#include "similarity_kernels.hpp"

namespace flo {

namespace {

constexpr int kFpLdsLanes = 64;   // workgroup of fp_topk_lds_kernel (kFpTile is a multiple: chunks stay whole tiles)

__device__ inline bool fp_better(float s, uint32_t i, float ts, uint32_t ti) { return s > ts || (s == ts && i < ti); }

// stage the tile [base, base + blockDim.x) of `ref` (clipped at end) into LDS rows, one record per lane
__device__ inline void fp_stage(uint4 (*tile)[2], const FpRec *ref, uint32_t base, uint32_t end) {
    const uint32_t t = threadIdx.x;
    if (base + t < end) {
        const uint4 *r = reinterpret_cast<const uint4 *>(ref + base + t);
        tile[t][0] = r[0];
        tile[t][1] = r[1];
    }
}

__device__ inline void fp_load(uint32_t (&q)[8], const FpRec *rec, uint32_t i, bool live) {
    uint4 a = make_uint4(0, 0, 0, 0), b = a;
    if (live) {
        const uint4 *r = reinterpret_cast<const uint4 *>(rec + i);
        a = r[0];
        b = r[1];
    }
    q[0] = a.x, q[1] = a.y, q[2] = a.z, q[3] = a.w, q[4] = b.x, q[5] = b.y, q[6] = b.z, q[7] = b.w;
}

// U of the pair (q, r): 1 for equal hashes, 0 for different formats (the exact scores), else fp_bound of the SAD key
__device__ inline float fp_pair_bound(const uint32_t (&q)[8], const uint4 &r0, const uint4 &r1) {
    uint32_t se = __builtin_amdgcn_sad_u8(q[0], r0.x, 0u);
    se = __builtin_amdgcn_sad_u8(q[1], r0.y, se);
    se = __builtin_amdgcn_sad_u8(q[2], r0.z, se);
    se = __builtin_amdgcn_sad_u8(q[3], r0.w, se);
    uint32_t sp = __builtin_amdgcn_sad_u8(q[4], r1.x, 0u);
    sp = __builtin_amdgcn_sad_u8(q[5], r1.y, sp);
    const uint32_t dl = __builtin_amdgcn_sad_u8(q[6], r1.z, 0u);   // = |la - lb| when the format bytes agree
    const float u = fp_bound(fp_bound_key(se, sp, dl));
    return q[7] == r1.w ? 1.0f : ((q[6] >> 8) != (r1.z >> 8) ? 0.0f : u);
}

__device__ inline float fp_pair_score(const uint32_t (&q)[8], const uint4 &r0, const uint4 &r1, const float *T) {
    const uint32_t r[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
    return fp_score(q, r, T);
}

template <int KM>
__global__ __launch_bounds__(kFpTile) void fp_topk_kernel(FpTopkArgs a) {
    __shared__ uint4 tile[kFpTile][2];
    __shared__ float T[256];
    const uint32_t t = threadIdx.x;
    const uint32_t qi = blockIdx.x * kFpTile + t;
    const uint32_t c0 = blockIdx.y * a.chunk, c1 = min(a.n_ref, c0 + a.chunk);
    const bool live = qi < a.n_q;
    T[t] = a.table[t];
    uint32_t q[8];
    fp_load(q, a.q, qi, live);
    const int pin = KM - (int)a.k;
    float es[KM];
    uint32_t ei[KM];
#pragma unroll
    for (int i = 0; i < KM; i++) {
        es[i] = i < pin ? 2.0f : -1.0f;
        ei[i] = i < pin ? 0u : 0xFFFFFFFFu;
    }
    for (uint32_t base = c0; base < c1; base += kFpTile) {
        __syncthreads();
        fp_stage(tile, a.ref, base, c1);
        __syncthreads();
        if (!live) continue;
        const uint32_t nt = min((uint32_t)kFpTile, c1 - base);
        for (uint32_t jj = 0; jj < nt; jj++) {
            const uint4 r0 = tile[jj][0], r1 = tile[jj][1];
            const uint32_t j = base + jj;
            if (fp_pair_bound(q, r0, r1) < es[KM - 1] || (a.self && j == qi)) continue;
            float cs = fp_pair_score(q, r0, r1, T);
            if (!fp_better(cs, j, es[KM - 1], ei[KM - 1])) continue;
            uint32_t ci = j;
#pragma unroll
            for (int i = 0; i < KM; i++) {
                const bool b = fp_better(cs, ci, es[i], ei[i]);
                const float ts = es[i];
                const uint32_t ti = ei[i];
                es[i] = b ? cs : ts;
                ei[i] = b ? ci : ti;
                cs = b ? ts : cs;
                ci = b ? ti : ci;
            }
        }
    }
    if (!live) return;
    const size_t o = ((size_t)blockIdx.y * a.n_q + qi) * a.k - (size_t)pin;
#pragma unroll
    for (int i = 0; i < KM; i++) {
        if (i >= pin) {
            a.part_idx[o + i] = ei[i];
            a.part_score[o + i] = es[i];
        }
    }
}

// k = 17 .. 64: the lists in LDS (see the head of the file); NT lanes = NT queries, tiles of NT references
template <int NT>
__global__ __launch_bounds__(NT) void fp_topk_lds_kernel(FpTopkArgs a) {
    __shared__ uint4 tile[NT][2];
    __shared__ float T[256];
    __shared__ float ls[kFpMaxK][NT];
    __shared__ uint32_t li[kFpMaxK][NT];
    const uint32_t t = threadIdx.x;
    const uint32_t qi = blockIdx.x * NT + t;
    const uint32_t c0 = blockIdx.y * a.chunk, c1 = min(a.n_ref, c0 + a.chunk);
    const bool live = qi < a.n_q;
    for (uint32_t d = t; d < 256; d += NT) T[d] = a.table[d];
    for (uint32_t s = 0; s < a.k; s++) {
        ls[s][t] = -1.0f;
        li[s][t] = 0xFFFFFFFFu;
    }
    uint32_t q[8];
    fp_load(q, a.q, qi, live);
    float ts = -1.0f;            // the k-th entry
    uint32_t ti = 0xFFFFFFFFu;
    for (uint32_t base = c0; base < c1; base += NT) {
        __syncthreads();
        fp_stage(tile, a.ref, base, c1);
        __syncthreads();
        if (!live) continue;
        const uint32_t nt = min((uint32_t)NT, c1 - base);
        for (uint32_t jj = 0; jj < nt; jj++) {
            const uint4 r0 = tile[jj][0], r1 = tile[jj][1];
            const uint32_t j = base + jj;
            if (fp_pair_bound(q, r0, r1) < ts || (a.self && j == qi)) continue;
            const float cs = fp_pair_score(q, r0, r1, T);
            if (!fp_better(cs, j, ts, ti)) continue;
            uint32_t p = a.k - 1;
            for (; p > 0 && fp_better(cs, j, ls[p - 1][t], li[p - 1][t]); p--) {
                ls[p][t] = ls[p - 1][t];
                li[p][t] = li[p - 1][t];
            }
            ls[p][t] = cs;
            li[p][t] = j;
            ts = ls[a.k - 1][t];
            ti = li[a.k - 1][t];
        }
    }
    if (!live) return;
    const size_t o = ((size_t)blockIdx.y * a.n_q + qi) * a.k;
    for (uint32_t s = 0; s < a.k; s++) {
        a.part_idx[o + s] = li[s][t];
        a.part_score[o + s] = ls[s][t];
    }
}

// lists 2p and 2p + 1 of src ([n_lists][n_q][k]) -> list p of dst, the best k of the two under the ranking rule
__global__ __launch_bounds__(256) void fp_merge_kernel(const uint32_t *si, const float *ss, uint32_t n_lists, uint32_t n_q,
                                                       uint32_t k, uint32_t *di, float *ds) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n_out = (n_lists + 1) / 2;
    if (g >= (uint64_t)n_out * n_q) return;
    const uint32_t p = (uint32_t)(g / n_q), qi = (uint32_t)(g % n_q);
    const size_t A = ((size_t)(2 * p) * n_q + qi) * k, D = ((size_t)p * n_q + qi) * k;
    if (2 * p + 1 >= n_lists) {
        for (uint32_t t = 0; t < k; t++) {
            di[D + t] = si[A + t];
            ds[D + t] = ss[A + t];
        }
        return;
    }
    const size_t B = A + (size_t)n_q * k;
    uint32_t ia = 0, ib = 0;
    for (uint32_t t = 0; t < k; t++) {   // ia + ib == t < k: both heads stay inside their lists
        const float sa = ss[A + ia], sb = ss[B + ib];
        const uint32_t xa = si[A + ia], xb = si[B + ib];
        const bool fa = fp_better(sa, xa, sb, xb);
        di[D + t] = fa ? xa : xb;
        ds[D + t] = fa ? sa : sb;
        ia += fa ? 1u : 0u;
        ib += fa ? 0u : 1u;
    }
}

template <bool WRITE>
__global__ __launch_bounds__(kFpTile) void fp_pairs_kernel(FpPairsArgs a) {
    __shared__ uint4 tile[kFpTile][2];
    __shared__ float T[256];
    const uint32_t t = threadIdx.x;
    const uint32_t i0 = blockIdx.x * kFpTile, i = i0 + t;
    const uint32_t nc = gridDim.y, c = blockIdx.y;
    const uint32_t c0 = c * a.chunk, c1 = min(a.n, c0 + a.chunk);
    const bool live = i < a.n;
    // rows of this block see j > i only: the tiles before the first j > i0 hold nothing for them
    const uint32_t first = max(c0, i0 + 1);
    if (first >= c1) {
        if (!WRITE && live) a.count[(size_t)i * nc + c] = 0;
        return;
    }
    T[t] = a.table[t];
    uint32_t q[8];
    fp_load(q, a.rec, i, live);
    const float thr = a.threshold;
    uint64_t pos = WRITE && live ? a.off[(size_t)i * nc + c] : 0;
    uint32_t n = 0;
    for (uint32_t base = c0 + (first - c0) / kFpTile * kFpTile; base < c1; base += kFpTile) {
        __syncthreads();
        fp_stage(tile, a.rec, base, c1);
        __syncthreads();
        if (!live) continue;
        const uint32_t nt = min((uint32_t)kFpTile, c1 - base);
        for (uint32_t jj = 0; jj < nt; jj++) {
            const uint4 r0 = tile[jj][0], r1 = tile[jj][1];
            const uint32_t j = base + jj;
            if (j <= i || fp_pair_bound(q, r0, r1) < thr) continue;
            const float s = fp_pair_score(q, r0, r1, T);
            if (!(s >= thr)) continue;
            if (WRITE) {
                if (pos < a.cap) {
                    a.pi[pos] = i;
                    a.pj[pos] = j;
                    a.ps[pos] = s;
                }
                pos++;
            }
            n++;
        }
    }
    if (!WRITE && live) a.count[(size_t)i * nc + c] = n;
}

}  // namespace

int launch_fp_topk(const FpTopkArgs &a0, uint32_t *out_idx, float *out_score, uint32_t *scratch_idx, float *scratch_score,
                   hipStream_t s) {
    FpTopkArgs a = a0;
    const uint32_t nc = (a.n_ref + a.chunk - 1) / a.chunk;
    if (nc == 1) {
        a.part_idx = out_idx;
        a.part_score = out_score;
    }
    const dim3 grid((a.n_q + kFpTile - 1) / kFpTile, nc);
    if (a.k <= 4)
        hipLaunchKernelGGL(fp_topk_kernel<4>, grid, dim3(kFpTile), 0, s, a);
    else if (a.k <= 16)
        hipLaunchKernelGGL(fp_topk_kernel<16>, grid, dim3(kFpTile), 0, s, a);
    else
        hipLaunchKernelGGL(fp_topk_lds_kernel<kFpLdsLanes>, dim3((a.n_q + kFpLdsLanes - 1) / kFpLdsLanes, nc),
                           dim3(kFpLdsLanes), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    // pairwise merges: part -> scratch -> part -> ... ; the last one writes out_*
    uint32_t n_lists = nc;
    uint32_t *si = a.part_idx;
    float *ss = a.part_score;
    while (n_lists > 1) {
        const uint32_t n_out = (n_lists + 1) / 2;
        uint32_t *di = n_out == 1 ? out_idx : (si == a.part_idx ? scratch_idx : a.part_idx);
        float *ds = n_out == 1 ? out_score : (ss == a.part_score ? scratch_score : a.part_score);
        const uint64_t threads = (uint64_t)n_out * a.n_q;
        hipLaunchKernelGGL(fp_merge_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, si, ss, n_lists, a.n_q,
                           a.k, di, ds);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        si = di;
        ss = ds;
        n_lists = n_out;
    }
    return 0;
}

int launch_fp_pairs_count(const FpPairsArgs &a, hipStream_t s) {
    const dim3 grid((a.n + kFpTile - 1) / kFpTile, (a.n + a.chunk - 1) / a.chunk);
    hipLaunchKernelGGL(fp_pairs_kernel<false>, grid, dim3(kFpTile), 0, s, a);
    return (int)hipGetLastError();
}

int launch_fp_pairs_write(const FpPairsArgs &a, hipStream_t s) {
    const dim3 grid((a.n + kFpTile - 1) / kFpTile, (a.n + a.chunk - 1) / a.chunk);
    hipLaunchKernelGGL(fp_pairs_kernel<true>, grid, dim3(kFpTile), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace flo
