// fidelity_kernels.hpp — device side of the fidelity reports (flo_batch_fidelity, flo_compare; fidelity.cpp): the block
// record, the per-block reduction every kernel that compares goes through, and the launchers.
//
// The block reduction is the contract of include/flo_hip.h: lane l of a wavefront holds block positions j = l + 64 k,
// k = 0 .. 15, adds its terms in k ascending (positions outside the block's compared part add nothing, which for these
// non-negative sums is the same as adding 0.0), and the lanes combine by an xor butterfly over 32, 16, 8, 4, 2, 1. The
// fused decode mode (lossy_decode_kernel<kDecCompare>, decode_kernels.hip) and fid_compare_kernel both feed the same
// FidAcc through the same two functions, so their records agree bit for bit by construction. f64 throughout, no
// contraction (the Makefile builds device code with -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace flo {

// One (decoded block, channel) record. The device keeps a record for every block of the DECODED signal: the compared
// part's sums and the block's tail energy (decoded frames past the compared range). The public flo_fidelity_block is the
// first six fields of the records of the compared blocks.
struct FidBlockDev {
    double signal, error, tail;
    float peak_error, peak_out;
    unsigned int clipped, n;
};
static_assert(sizeof(FidBlockDev) == 40, "FidBlockDev layout");

// One clip of a fidelity pass.
struct FidClipDev {
    unsigned long long src;          // float offset of the clip's source (interleaved, channels per frame)
    unsigned long long dec;          // float offset of the clip's decoded PCM (fid_compare_kernel only)
    unsigned long long src_frames;   // whole source frames
    unsigned long long dec_frames;   // decoded frames
    unsigned long long blk0;         // first decoded block of the clip: its records are blk[(blk0 + b) * channels + c]
    unsigned long long pub0;         // first public block of the clip (fid_totals_kernel)
};

// Appended to LossyDecArgs for lossy_decode_kernel<kDecCompare>: clip i of the decode is clip[i] here.
struct LossyCmpArgs {
    const float *src;
    const FidClipDev *clip;
    FidBlockDev *blk;
};

struct FidAcc {
    double s, e, t;
    float pe, po;
    unsigned int cl;
};

__device__ __forceinline__ FidAcc fid_acc_zero() {
    FidAcc a;
    a.s = 0.0;
    a.e = 0.0;
    a.t = 0.0;
    a.pe = 0.0f;
    a.po = 0.0f;
    a.cl = 0u;
    return a;
}

// one position: x the source sample, y the decoded one. `in`: inside the compared range; `tail`: a decoded frame past it.
// (peak_error: f32 rounding is monotone, so the maximum of the rounded |y - x| is the rounded maximum)
__device__ __forceinline__ void fid_acc_add(FidAcc &a, float x, float y, bool in, bool tail) {
    if (in) {
        const double xd = (double)x, d = (double)y - xd;
        a.s = a.s + xd * xd;
        a.e = a.e + d * d;
        a.pe = fmaxf(a.pe, (float)fabs(d));
        a.po = fmaxf(a.po, fabsf(y));
        a.cl += fabsf(y) > 1.0f ? 1u : 0u;
    } else if (tail) {
        const double yd = (double)y;
        a.t = a.t + yd * yd;
    }
}

// the butterfly over the wavefront, then lane 0 stores the record (every lane holds the same sums: each step adds the
// same two values in either order)
__device__ __forceinline__ void fid_block_store(FidAcc a, unsigned int n, FidBlockDev *r, int lane) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        a.s = a.s + __shfl_xor(a.s, o, 64);
        a.e = a.e + __shfl_xor(a.e, o, 64);
        a.t = a.t + __shfl_xor(a.t, o, 64);
        a.pe = fmaxf(a.pe, __shfl_xor(a.pe, o, 64));
        a.po = fmaxf(a.po, __shfl_xor(a.po, o, 64));
        a.cl += (unsigned int)__shfl_xor((int)a.cl, o, 64);
    }
    if (lane == 0) {
        FidBlockDev v;
        v.signal = a.s;
        v.error = a.e;
        v.tail = a.t;
        v.peak_error = a.pe;
        v.peak_out = a.po;
        v.clipped = a.cl;
        v.n = n;
        *r = v;
    }
}

// fid_compare_kernel: decoded PCM (dec) against the source (src), one wavefront per (decoded block, channel).
struct FidCompareArgs {
    const float *src;
    const float *dec;
    const FidClipDev *clip;     // [n_clips]
    FidBlockDev *blk;
    unsigned int n_clips;
    int channels;
    unsigned long long n_units;   // decoded blocks of all clips x channels
};

// fid_totals_kernel: one thread per (clip, channel) walks the clip's records in block order.
struct FidPublicBlock {   // = flo_fidelity_block
    double signal, error;
    float peak_error, peak_out;
    unsigned int clipped, n;
};
struct FidTotal {         // = flo_fidelity
    double signal, error, tail_energy, snr_db, seg_snr_db;
    float peak_error, peak_out;
    unsigned long long clipped, compared_frames, source_frames, decoded_frames;
    unsigned int n_blocks, seg_blocks;
};
struct FidTotalsArgs {
    const FidClipDev *clip;
    const FidBlockDev *blk;
    FidTotal *out;              // [n_clips * channels]
    FidPublicBlock *pub;        // nullable: the compared blocks' public records at (pub0 + b) * channels + c
    unsigned int n_clips;
    int channels;
};

int launch_fid_compare(const FidCompareArgs &A, hipStream_t s);
int launch_fid_totals(const FidTotalsArgs &A, hipStream_t s);

}  // namespace flo
