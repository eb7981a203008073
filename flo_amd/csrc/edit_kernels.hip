// edit_kernels.hip — cuts of the clips of a batch, padded, faded and mixed to another channel count, and the active range
// of every clip (flo_batch_edit, flo_batch_active_range, flo_edit; edit.cpp). The definition, the tile geometry and the class
// of a tile are edit_plan.hpp's.
//
// One workgroup per tile of the flat (output clip, tile) list; it finds its clip by binary search over the per-clip prefix,
// as the sample-rate conversion and the normalisation do. The segment is read through scalar loads (its index is uniform),
// and so is the tile's class, computed from it by the plan's own function: a wave-uniform branch.
//
// Interior tiles (no pad, no fade, wholly inside the source) store 16 bytes per lane. Output clips start 16-byte aligned and
// F * Cout is a multiple of 4 floats, so every tile's first output is aligned; the source address is clip_off + start * Cin
// floats, only 4-byte aligned in general. The copy form reads it with 16-byte loads at the 4-byte aligned address itself
// (one global_load_dwordx4 per lane; DESIGN 4.15 has the four alignment classes measured). 2 -> 1 reads 32 bytes per lane at
// an 8-byte aligned address, 1 -> 2 reads 8 bytes per lane at a 4-byte aligned one. A tile that lies wholly in a pad or
// wholly past the source's end stores zeros, 16 bytes per lane. Every other tile, and the generic form, goes frame by frame.
//
// All forms share ed_mix and ed_weight, so the order of operations is the definition's in every form.
// Compiled with -ffp-contract=off; the FMAs are explicit, the products single multiplications, the divisions IEEE.
#include "clip_tiles.hpp"
#include "edit_kernels.hpp"

namespace flo {

typedef float ed_v4f __attribute__((ext_vector_type(4)));
typedef float ed_v2f __attribute__((ext_vector_type(2)));
typedef unsigned int ed_v4u __attribute__((ext_vector_type(4)));

// y[j] of one frame: a = fl32(m[j][0] * x[0]), then a = fmaf(m[j][i], x[i], a) for i = 1 .. cin - 1
template <unsigned MAXC>
__device__ __forceinline__ float ed_mix(const float *row, const float (&x)[MAXC], unsigned cin) {
    float a = row[0] * x[0];
#pragma unroll
    for (unsigned i = 1; i < MAXC; i++)
        if (i < cin) a = __builtin_fmaf(row[i], x[i], a);
    return a;
}

// the fade weight of frame u of the cut: false when neither fade applies
__device__ __forceinline__ bool ed_weight(unsigned long long u, const EditSeg &s, float &w) {
    const unsigned long long v = s.frames - 1 - u;
    const bool in = u < s.fade_in, out = v < s.fade_out;
    if (!in && !out) return false;
    const float w_in = in ? __fdiv_rn((float)(unsigned)u, (float)s.fade_in) : 0.f;
    const float w_out = out ? __fdiv_rn((float)(unsigned)v, (float)s.fade_out) : 0.f;
    w = in && out ? w_in * w_out : in ? w_in : w_out;
    return true;
}

template <int FORM>
struct EdShape {
    static constexpr unsigned kCin = FORM == kEditTwoToOne ? 2 : FORM == kEditOneToTwo ? 1 : 0;   // 0: the launch's
    static constexpr unsigned kCout = FORM == kEditTwoToOne ? 1 : FORM == kEditOneToTwo ? 2 : 0;
    static constexpr unsigned kMax = FORM == kEditTwoToOne || FORM == kEditOneToTwo ? 2 : kEditMaxMix;
};

// source frame and fade weight of output frame t of the segment, mixed forms: false where the frame is +0.0
template <unsigned MAXC>
__device__ __forceinline__ bool ed_source(const EditSeg &s, const float *__restrict__ src, unsigned long long avail, unsigned long long t,
                                          bool faded, unsigned cin, float (&x)[MAXC], float &w, bool &weighted) {
    weighted = false;
#pragma unroll
    for (unsigned i = 0; i < MAXC; i++) x[i] = 0.f;
    if (t < s.pad_head) return false;
    const unsigned long long u = t - s.pad_head;
    if (u >= avail) return false;
    const float *__restrict__ p = src + (s.start + u) * cin;
#pragma unroll
    for (unsigned i = 0; i < MAXC; i++)
        if (i < cin) x[i] = p[i];
    weighted = faded && ed_weight(u, s, w);
    return true;
}

// the frames [f0, f1) of the tile one by one (every class). The generic form walks the matrix row by row: eight
// coefficients are live in scalar registers, not sixty-four.
template <int FORM>
__device__ __forceinline__ void ed_frames(const EditArgs &A, const EditSeg &s, const float *__restrict__ src, float *__restrict__ dst,
                                          unsigned long long t0, unsigned f0, unsigned f1, bool faded, unsigned cin, unsigned cout, unsigned tid) {
    constexpr unsigned MAXC = EdShape<FORM>::kMax;
    const unsigned long long avail = edit_avail(s);
    for (unsigned f = f0 + tid; f < f1; f += kEditThreads) {
        float x[MAXC], w = 1.f;
        bool weighted;
        const bool live = ed_source<MAXC>(s, src, avail, t0 + f, faded, cin, x, w, weighted);
        float *__restrict__ q = dst + (t0 + f) * cout;
        if constexpr (FORM == kEditGeneric) {
#pragma unroll 1
            for (unsigned j = 0; j < cout; j++) {
                float v = 0.f;
                if (live) {
                    const float a = ed_mix<MAXC>(A.m + j * kEditMaxMix, x, cin);
                    v = weighted ? a * w : a;
                }
                q[j] = v;
            }
        } else {
#pragma unroll
            for (unsigned j = 0; j < EdShape<FORM>::kCout; j++) {
                float v = 0.f;
                if (live) {
                    const float a = ed_mix<MAXC>(A.m + j * kEditMaxMix, x, cin);
                    v = weighted ? a * w : a;
                }
                q[j] = v;
            }
        }
    }
}

// the copy form's tile, every class: n floats from output frame t0 on, one by one
__device__ __forceinline__ void ed_copy_floats(const EditSeg &s, const float *__restrict__ src, float *__restrict__ dst, unsigned long long t0,
                                               unsigned n, bool faded, unsigned ch, unsigned tid) {
    const unsigned long long avail = edit_avail(s);
    for (unsigned i = tid; i < n; i += kEditThreads) {
        const unsigned f = i / ch, c = i - f * ch;
        const unsigned long long t = t0 + f;
        float v = 0.f;
        if (t >= s.pad_head && t - s.pad_head < avail) {
            const unsigned long long u = t - s.pad_head;
            v = src[(s.start + u) * ch + c];
            float w;
            if (faded && ed_weight(u, s, w)) v = v * w;
        }
        dst[t0 * ch + i] = v;
    }
}

// an interior tile of the copy form: n floats from sp (4-byte aligned) to dp (16-byte aligned), bit for bit
__device__ __forceinline__ void ed_copy_interior(const float *__restrict__ sp, float *__restrict__ dp, unsigned n, unsigned tid) {
    const unsigned n4 = n >> 2;
    ed_v4u *__restrict__ d4 = reinterpret_cast<ed_v4u *>(dp);
    for (unsigned i = tid; i < n4; i += kEditThreads) {
        ed_v4u v;
        __builtin_memcpy(&v, sp + 4 * (size_t)i, 16);   // one 16-byte load at a 4-byte aligned address
        d4[i] = v;
    }
    const unsigned *__restrict__ s1 = reinterpret_cast<const unsigned *>(sp);
    unsigned *__restrict__ d1 = reinterpret_cast<unsigned *>(dp);
    for (unsigned i = 4 * n4 + tid; i < n; i += kEditThreads) d1[i] = s1[i];
}

// a tile without a source frame: n floats of +0.0 at dp (16-byte aligned)
__device__ __forceinline__ void ed_zero_tile(float *__restrict__ dp, unsigned n, unsigned tid) {
    const unsigned n4 = n >> 2;
    ed_v4f *__restrict__ d4 = reinterpret_cast<ed_v4f *>(dp);
    for (unsigned i = tid; i < n4; i += kEditThreads) d4[i] = ed_v4f{0.f, 0.f, 0.f, 0.f};
    for (unsigned i = 4 * n4 + tid; i < n; i += kEditThreads) dp[i] = 0.f;
}

template <int FORM>
__global__ __launch_bounds__(kEditThreads) void edit_kernel(const EditArgs A) {
    const unsigned tid = threadIdx.x;
    const unsigned k = tile_clip(A.pre, A.n_segs, blockIdx.x);
    const unsigned tile = blockIdx.x - A.pre[k];
    const EditSeg *__restrict__ segs = A.segs;
    const EditSeg s = segs[k];
    const unsigned cin = EdShape<FORM>::kCin ? EdShape<FORM>::kCin : A.cin, cout = EdShape<FORM>::kCout ? EdShape<FORM>::kCout : A.cout;
    const unsigned F = edit_tile_frames(cout);
    const unsigned long long T = edit_out_frames(s), t0 = (unsigned long long)tile * F;
    const unsigned nf = T - t0 < F ? (unsigned)(T - t0) : F;
    const unsigned cls = edit_tile_class(s, tile, F);
    const bool faded = (cls & kEditFaded) != 0;
    const float *__restrict__ src = A.src + s.src_off;
    float *__restrict__ dst = A.dst + s.dst_off;
    if (t0 + nf <= s.pad_head || t0 >= s.pad_head + edit_avail(s)) {   // wholly in the head pad, or behind the last source frame
        ed_zero_tile(dst + t0 * cout, nf * cout, tid);
        return;
    }
    if constexpr (FORM == kEditCopy) {
        if (cls == kEditInterior) ed_copy_interior(src + (s.start + (t0 - s.pad_head)) * cin, dst + t0 * cin, nf * cin, tid);
        else ed_copy_floats(s, src, dst, t0, nf * cin, faded, cin, tid);
    } else {
    unsigned done = 0;   // frames of the tile the vector path has made
    if (FORM == kEditTwoToOne && cls == kEditInterior) {
        // four output frames per lane: 32 bytes in (8-byte aligned: the clip's offset and 2 * start are even), 16 out
        const float *__restrict__ sp = src + (s.start + (t0 - s.pad_head)) * 2;
        ed_v4f *__restrict__ d4 = reinterpret_cast<ed_v4f *>(dst + t0);
        const unsigned n4 = nf >> 2;
        for (unsigned i = tid; i < n4; i += kEditThreads) {
            ed_v2f p[4];
            __builtin_memcpy(p, __builtin_assume_aligned(sp + 8 * (size_t)i, 8), 32);
            ed_v4f v;
#pragma unroll
            for (unsigned e = 0; e < 4; e++) {
                const float x[2] = {p[e].x, p[e].y};
                v[e] = ed_mix<2>(A.m, x, 2);
            }
            d4[i] = v;
        }
        done = 4 * n4;
    }
    if (FORM == kEditOneToTwo && cls == kEditInterior) {
        // two output frames per lane: 8 bytes in (4-byte aligned), 16 out
        const float *__restrict__ sp = src + (s.start + (t0 - s.pad_head));
        ed_v4f *__restrict__ d4 = reinterpret_cast<ed_v4f *>(dst + t0 * 2);
        const unsigned n4 = nf >> 1;
        for (unsigned i = tid; i < n4; i += kEditThreads) {
            ed_v2f p;
            __builtin_memcpy(&p, sp + 2 * (size_t)i, 8);
            const float x0[2] = {p.x, 0.f}, x1[2] = {p.y, 0.f};
            ed_v4f v;
            v.x = ed_mix<2>(A.m, x0, 1);
            v.y = ed_mix<2>(A.m + kEditMaxMix, x0, 1);
            v.z = ed_mix<2>(A.m, x1, 1);
            v.w = ed_mix<2>(A.m + kEditMaxMix, x1, 1);
            d4[i] = v;
        }
        done = 2 * n4;
    }
    ed_frames<FORM>(A, s, src, dst, t0, done, nf, faded, cin, cout, tid);
    }
}

// the smallest and the largest active frame of every clip: per tile the extremes of the flat sample index by wave
// reductions (a sample's frame is its index div the channel count, which keeps the order), then one atomicMin and one
// atomicMax per tile that found something
__global__ __launch_bounds__(kEditThreads) void edit_active_kernel(const EditActiveArgs A) {
    __shared__ unsigned red_lo[kEditThreads / 64], red_hi[kEditThreads / 64];
    const unsigned tid = threadIdx.x;
    const unsigned clip = tile_clip(A.pre, A.n_clips, blockIdx.x);
    const unsigned tile = blockIdx.x - A.pre[clip];
    const unsigned long long *__restrict__ frames = A.frames, *__restrict__ src_off = A.src_off;
    const unsigned long long n = frames[clip];
    const unsigned ch = A.channels, F = edit_tile_frames(ch);
    const unsigned long long t0 = (unsigned long long)tile * F;
    const unsigned nf = n - t0 < F ? (unsigned)(n - t0) : F, cnt = nf * ch, n4 = cnt >> 2;
    const float *__restrict__ p = A.src + src_off[clip] + t0 * ch;   // 16-byte aligned: the clip is, and so are F * ch floats
    const ed_v4f *__restrict__ p4 = reinterpret_cast<const ed_v4f *>(p);
    const float thr = A.threshold;
    unsigned lo = 0xFFFFFFFFu, hi = 0;   // the smallest active index, the largest plus one
    for (unsigned i = tid; i < n4; i += kEditThreads) {
        const ed_v4f v = p4[i];
#pragma unroll
        for (unsigned e = 0; e < 4; e++)
            if (!(__builtin_fabsf(v[e]) <= thr)) {
                const unsigned j = 4 * i + e;
                lo = j < lo ? j : lo;
                hi = j + 1 > hi ? j + 1 : hi;
            }
    }
    for (unsigned j = 4 * n4 + tid; j < cnt; j += kEditThreads)
        if (!(__builtin_fabsf(p[j]) <= thr)) {
            lo = j < lo ? j : lo;
            hi = j + 1 > hi ? j + 1 : hi;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned l2 = (unsigned)__shfl_xor((int)lo, o), h2 = (unsigned)__shfl_xor((int)hi, o);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((tid & 63u) == 0) {
        red_lo[tid >> 6] = lo;
        red_hi[tid >> 6] = hi;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (unsigned w = 1; w < kEditThreads / 64; w++) {
            lo = red_lo[w] < lo ? red_lo[w] : lo;
            hi = red_hi[w] > hi ? red_hi[w] : hi;
        }
        if (hi) {
            atomicMin(A.first + clip, t0 + lo / ch);
            atomicMax(A.end + clip, t0 + (hi - 1) / ch + 1);
        }
    }
}

int launch_edit(const EditArgs &a, EditForm form, unsigned int n_tiles, hipStream_t stream) {
    if (!n_tiles) return 0;
    const dim3 grid(n_tiles), block(kEditThreads);
    switch (form) {
    case kEditCopy: edit_kernel<kEditCopy><<<grid, block, 0, stream>>>(a); break;
    case kEditTwoToOne: edit_kernel<kEditTwoToOne><<<grid, block, 0, stream>>>(a); break;
    case kEditOneToTwo: edit_kernel<kEditOneToTwo><<<grid, block, 0, stream>>>(a); break;
    case kEditGeneric: edit_kernel<kEditGeneric><<<grid, block, 0, stream>>>(a); break;
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

int launch_edit_active(const EditActiveArgs &a, unsigned int n_tiles, hipStream_t stream) {
    if (!n_tiles) return 0;
    edit_active_kernel<<<dim3(n_tiles), dim3(kEditThreads), 0, stream>>>(a);
    return (int)hipGetLastError();
}

}  // namespace flo
