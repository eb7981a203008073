// fidelity_kernels.hip — the fidelity reports' own kernels for gfx950 (fidelity_kernels.hpp; host side in fidelity.cpp):
// the compare of a decoded buffer with its source (lossless batches and files, and lossy batches under
// FLO_FIDELITY_UNFUSED=1) and the per-clip totals. The fused lossy form is lossy_decode_kernel<kDecCompare>
// (decode_kernels.hip); all three build their block records through fid_acc_add / fid_block_store.
#include "fidelity_kernels.hpp"

namespace flo {

// One wavefront per (decoded block, channel), four per workgroup: the channels of a block are neighbouring waves of one
// workgroup, so the interleaved lines they share are read by one CU. The clip comes from a binary search over the clips'
// first blocks.
__global__ __launch_bounds__(256) void fid_compare_kernel(FidCompareArgs A) {
    const int lane = (int)(threadIdx.x & 63u);
    const unsigned long long u = (unsigned long long)blockIdx.x * 4ull + (threadIdx.x >> 6);
    if (u >= A.n_units) return;
    const unsigned nch = (unsigned)A.channels;
    const unsigned long long gb = u / nch;
    const unsigned c = (unsigned)(u % nch);
    unsigned lo = 0, hi = A.n_clips;   // the last clip whose first block is <= gb
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (A.clip[mid].blk0 <= gb) lo = mid;
        else hi = mid;
    }
    const FidClipDev cd = A.clip[lo];
    const unsigned long long f0 = (gb - cd.blk0) * 1024ull;
    if (f0 >= cd.dec_frames) return;   // (the host sizes the grid by the decoded blocks: cannot happen)
    const unsigned long long cmp = cd.src_frames < cd.dec_frames ? cd.src_frames : cd.dec_frames;
    const uint32_t in_end = cmp > f0 ? (cmp - f0 < 1024ull ? (uint32_t)(cmp - f0) : 1024u) : 0u;
    const uint32_t dec_end = cd.dec_frames - f0 < 1024ull ? (uint32_t)(cd.dec_frames - f0) : 1024u;
    const float *sb = A.src + cd.src + f0 * nch + c;
    const float *db = A.dec + cd.dec + f0 * nch + c;
    float xs[16], ys[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t j = (uint32_t)lane + 64u * (uint32_t)k;
        xs[k] = j < in_end ? sb[j * nch] : 0.0f;
        ys[k] = j < dec_end ? db[j * nch] : 0.0f;
    }
    FidAcc acc = fid_acc_zero();
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t j = (uint32_t)lane + 64u * (uint32_t)k;
        fid_acc_add(acc, xs[k], ys[k], j < in_end, j >= in_end && j < dec_end);
    }
    fid_block_store(acc, in_end, A.blk + gb * nch + c, lane);
}

// One wavefront per (clip, channel), four per workgroup: the clip's records in chunks of 64 blocks, one per lane (the
// next chunk's loads in flight while the current one is summed). The segmental SNR of a block, the maxima and the
// clipped counts are lane-parallel; the sums are sequential in block order, so each lane leaves its block's terms in LDS
// (0.0 for a block outside the sum: adding +0.0 to these sums changes nothing) and the wave walks them in order, the
// reads of a chunk all in flight at once. (One thread per clip and channel walking its records one load after the other
// took 4.6 ms for the 7 752 blocks of a 180 s clip; lanes handing their terms over by readlane, 0.93 ms.)
__global__ __launch_bounds__(256) void fid_totals_kernel(FidTotalsArgs A) {
    const int lane = (int)(threadIdx.x & 63u);
    const unsigned nch = (unsigned)A.channels;
    const unsigned long long t = (unsigned long long)blockIdx.x * 4ull + (threadIdx.x >> 6);
    if (t >= (unsigned long long)A.n_clips * nch) return;
    const unsigned i = (unsigned)(t / nch), c = (unsigned)(t % nch);
    const FidClipDev cd = A.clip[i];
    const unsigned long long cmp = cd.src_frames < cd.dec_frames ? cd.src_frames : cd.dec_frames;
    const unsigned long long nb = (cmp + 1023ull) >> 10, nd = (cd.dec_frames + 1023ull) >> 10;
    const FidBlockDev *rec = A.blk + cd.blk0 * nch + c;
    auto load = [&](unsigned long long b) -> FidBlockDev {
        FidBlockDev r{};
        if (b < nd) r = rec[b * nch];
        return r;
    };
    __shared__ double sh[4][4][64];   // per wave: the chunk's signal, error, tail and segmental terms
    double(*const w)[64] = sh[threadIdx.x >> 6];
    double s = 0.0, e = 0.0, tail = 0.0, seg = 0.0;   // (wave-uniform)
    unsigned int seg_n = 0;
    float pe = 0.0f, po = 0.0f;                        // (per lane, combined at the end)
    unsigned long long cl = 0;
    FidBlockDev next = load((unsigned long long)lane);
    for (unsigned long long b0 = 0; b0 < nd; b0 += 64) {
        const FidBlockDev r = next;
        next = load(b0 + 64 + (unsigned long long)lane);
        const unsigned long long b = b0 + (unsigned long long)lane;
        const bool in = b < nb;   // (blocks nb .. nd - 1 are all tail, their compared sums 0: `in` bounds the public records' store)
        double v = 0.0;
        bool q = false;
        if (in) {
            pe = fmaxf(pe, r.peak_error);
            po = fmaxf(po, r.peak_out);
            cl += r.clipped;
            if (r.signal / (double)r.n >= 1e-10) {
                q = true;
                v = 60.0;
                if (r.error != 0.0) {   // (only an error of exactly 0 counts as 60: a NaN error gives a NaN term)
                    v = 10.0 * log10(r.signal / r.error);
                    v = v < -10.0 ? -10.0 : (v > 60.0 ? 60.0 : v);
                }
            }
            if (A.pub) {
                FidPublicBlock p;
                p.signal = r.signal;
                p.error = r.error;
                p.peak_error = r.peak_error;
                p.peak_out = r.peak_out;
                p.clipped = r.clipped;
                p.n = r.n;
                A.pub[(cd.pub0 + b) * nch + c] = p;
            }
        }
        seg_n += (unsigned)__popcll(__ballot(q));
        w[0][lane] = in ? r.signal : 0.0;
        w[1][lane] = in ? r.error : 0.0;
        w[2][lane] = r.tail;            // (0.0 past the decoded blocks: load() gives a zero record)
        w[3][lane] = v;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 16
        for (int l = 0; l < 64; l++) {
            s = s + w[0][l];
            e = e + w[1][l];
            tail = tail + w[2][l];
            seg = seg + w[3][l];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        pe = fmaxf(pe, __shfl_xor(pe, o, 64));
        po = fmaxf(po, __shfl_xor(po, o, 64));
        cl += (unsigned long long)__shfl_xor((long long)cl, o, 64);
    }
    if (lane != 0) return;
    FidTotal o;
    o.signal = s;
    o.error = e;
    o.tail_energy = tail;
    o.snr_db = e == 0.0 ? __builtin_inf() : (s == 0.0 ? -__builtin_inf() : 10.0 * log10(s / e));
    o.seg_snr_db = seg_n ? seg / (double)seg_n : __builtin_nan("");
    o.peak_error = pe;
    o.peak_out = po;
    o.clipped = cl;
    o.compared_frames = cmp;
    o.source_frames = cd.src_frames;
    o.decoded_frames = cd.dec_frames;
    o.n_blocks = (unsigned int)nb;
    o.seg_blocks = seg_n;
    A.out[t] = o;
}

#define FLO_LAUNCH_CHECK()                      \
    do {                                        \
        hipError_t e_ = hipGetLastError();      \
        if (e_ != hipSuccess) return (int)e_;   \
    } while (0)

int launch_fid_compare(const FidCompareArgs &A, hipStream_t s) {
    if (!A.n_units || !A.n_clips || A.channels < 1) return 0;
    const unsigned long long wgs = (A.n_units + 3ull) / 4ull;
    if (wgs > 0x7FFFFFFFull) return -1;
    hipLaunchKernelGGL(fid_compare_kernel, dim3((unsigned)wgs), dim3(256), 0, s, A);
    FLO_LAUNCH_CHECK();
    return 0;
}
int launch_fid_totals(const FidTotalsArgs &A, hipStream_t s) {
    const unsigned long long n = (unsigned long long)A.n_clips * (unsigned)(A.channels > 0 ? A.channels : 0);
    if (!n) return 0;
    if ((n + 3) / 4 > 0x7FFFFFFFull) return -1;
    hipLaunchKernelGGL(fid_totals_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, A);
    FLO_LAUNCH_CHECK();
    return 0;
}

}  // namespace flo
