// ladder_kernels.hip — the kernel of the quality ladder (flo_batch_encode_ladder, ladder.cpp). A translation unit of its own:
// lossy_kernels.hip, whose kernels are the yardstick every form is compared against, compiles to the bytes it compiled to
// before this file existed (a kernel added there moved the register allocation of its single-channel neighbours). The
// device functions are the shared ones of lossy_device.hpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lossy_device.hpp"
#include "lossy_kernels.hpp"

namespace flo {

// The frames of one transform at every rung of a quality ladder (flo_batch_encode_ladder, ladder.cpp): what
// lossy_curve_kernel prices, packed. One wavefront per frame; the channels go in the outer loop with the single-channel
// device functions (as lossy_frame_n_kernel walks them), the rungs in the inner one. Per channel, once: transform, band
// statistics, temporal masking from pass 1 and the scan, scale factors and their words, the unmasked integers round(c * sf)
// and |c|. Per rung: the keep bits exactly as lossy_curve_kernel forms them (threshold table in LDS over the dead
// transposition buffer, the rung's own ath_lin rows, the uniform branch to quantise<1, true>'s re-decision), q = keep ? q0 : 0,
// then sparse_plan_m and sparse_emit_n into ONE staged channel section (length word + sparse bytes), which is copied to the
// rung's running position in the rung's slot of this frame. Lane j carries rung j's position (12 + 50 nch + the sections of
// the earlier channels); the 25 scale words are stored per channel and rung, the frame header when the last channel is
// done. LDS does not depend on the number of rungs. Slots: [rung][frame][slot_bytes]; frame_size: [rung][frame];
// sizes[rung * n_clips + clip] += the frame's bytes (u64 integer atomics: the host sizes the files from them).
constexpr int kLadderStage = 4 + 2064 + 128 + 12;   // length word, the largest sparse blob, two trash bytes per lane; 16-byte multiple
static_assert(kLadderStage % 16 == 0, "the staged section keeps 16-byte alignment");
#ifndef FLO_LADDER_WAVES_PER_SIMD
#define FLO_LADDER_WAVES_PER_SIMD 3
#endif
__global__ __launch_bounds__(64, FLO_LADDER_WAVES_PER_SIMD) void lossy_ladder_kernel(CurveArgs C, const float *__restrict__ pcm_all, const float *__restrict__ a_t,
                                                          const float *__restrict__ s_prev, unsigned long long *__restrict__ sizes) {
    __shared__ WaveLds<1> lds;
    __shared__ __attribute__((aligned(16))) uint8_t stage[kLadderStage];
    static_assert(kMaxCurveCandidates * 32 <= kXchFloats, "the threshold table fits the exchange buffer");
    static_assert(kMaxCurveCandidates <= 64, "one lane per rung");
    const LossyArgs &A = C.A;
    const LossyDevTables &T = A.T;
    const int lane0 = lane_id();
    const int nch = A.nch;
    const unsigned long long gframe = blockIdx.x;
    if (gframe >= A.total_frames) return;
    int lo = 0, hi = A.n_clips - 1;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (A.clip_frame0[mid] <= gframe) lo = mid; else hi = mid - 1;
    }
    const unsigned clip = (unsigned)lo;
    const unsigned h = (unsigned)(gframe - A.clip_frame0[clip]);
    const float *pcm = pcm_all + A.clip_off[clip];
    const long long n_sf = (long long)A.clip_nsf[clip];
    const int n_q = C.n_q;
    const unsigned long long rung_stride = A.total_frames * (unsigned long long)A.slot_bytes;
    uint8_t *const slot0 = A.slots + gframe * (unsigned long long)A.slot_bytes;   // rung 0's slot of this frame

    LaneConst L;
    load_lane_const(lane0, L, T);
    if (lane0 == 0) lds.slots[0][kZeroSlot] = make_float2(0.f, 0.f);
    uint32_t pos = 12u + 50u * (uint32_t)nch;   // lane j: where rung j's next channel section starts
    for (int ch = 0; ch < nch; ch++) {
        // (the lane behind an optimisation barrier: what is derived from it is recomputed per channel, not hoisted out of the
        // loop into dozens of registers that live across the transform)
        const int lane = lane_id_opaque();
        float c[1][16];
        {
            float ae[1][8], ao[1][8], be[1][8], bo2[1][8];
            load_half<1>(lane, pcm, n_sf, nch, ch, (long long)h * 1024 - 1024, ae, ao);
            load_half<1>(lane, pcm, n_sf, nch, ch, (long long)h * 1024, be, bo2);
            float zr[1][8], zi[1][8];   // (mdct_frame<1> of lossy_kernels.hip)
            fold<1>(lane, ae, ao, be, bo2, zr, zi, T);
            fft512<1>(lane, zr, zi, lds.u.xch, T);
            post_rotate_transpose<1>(lane, zr, zi, lds.u.coef, c, T);
        }
        float energy[1], bmax[1];
        band_stats<1>(lane, c, lds.slots, T, energy, bmax);
        // temporal masking and scale factor as analyse_frame (lanes 0..24 = bands)
        const unsigned long long fi = (gframe * (unsigned)nch + (unsigned)ch) * 32 + (unsigned)(lane < 25 ? lane : 0);
        const float a = a_t[fi], prev = s_prev[fi];
        const float s = max_raw(a, prev * 0.7f);
        const float sf = bmax[0] > 1e-10f ? __fdiv_rn(30000.0f, bmax[0]) : 1.0f;
        const uint32_t sfw = sf_word(sf);
        float *thr_tab = lds.u.xch[0];   // [n_q][32] amplitude thresholds (the transposition buffer is dead)
        if (lane < 25) {
            lds.bandv[0][lane] = make_float2(0.f, sf);
            lds.band_s[0][lane] = s;
            for (int j = 0; j < n_q; j++) thr_tab[32 * j + lane] = masking_amplitude(s, C.smr_thr[j]);
        }
        wave_sync();
        // the quantised integers (quality-independent) and |c|
        uint32_t bo[16];
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const float4 bo4 = T.pack[(kRowBo + g) * 64 + lane];
            bo[4 * g + 0] = __float_as_uint(bo4.x), bo[4 * g + 1] = __float_as_uint(bo4.y);
            bo[4 * g + 2] = __float_as_uint(bo4.z), bo[4 * g + 3] = __float_as_uint(bo4.w);
        }
        int q0[16];
        float ax[16];
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const float sfe = reinterpret_cast<const float2 *>(reinterpret_cast<const char *>(lds.bandv[0]) + bo[e])->y;
            const float x = c[0][e];
            const float xs = x * sfe;
            const float half = __uint_as_float((__float_as_uint(xs) & 0x80000000u) | 0x3EFFFFFFu);
            q0[e] = cvt_rz(xs + half);
            ax[e] = fabsf(x);
        }
        for (int j = 0; j < n_q; j++) {
            float al[16], tb[16];
            const float4 *ap = C.ath[j] + lane;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const float4 al4 = ap[64 * g];
                al[4 * g + 0] = al4.x, al[4 * g + 1] = al4.y, al[4 * g + 2] = al4.z, al[4 * g + 3] = al4.w;
            }
            const char *tj = reinterpret_cast<const char *>(thr_tab + 32 * j);
#pragma unroll
            for (int e = 0; e < 16; e++) tb[e] = *reinterpret_cast<const float *>(tj + (bo[e] >> 1));
            uint32_t keep = 0;
            if ((C.exact_mask >> j) & 1u) {   // uniform: quantise<1, true>'s decision
                const bool qt = (C.qtrans_mask >> j) & 1u;
                const float smr = C.smr_thr[j];
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const float thr = max_raw(tb[e], al[e]);
                    bool k = ax[e] > thr;
                    const bool near = fabsf(ax[e] - thr) <= 1e-5f * thr || (qt && !(ax[e] > 1e-10f));
                    if (near) {
                        float signal_db = ax[e] > 1e-10f ? 20.0f * log10f(ax[e]) : -100.0f;
                        float sdb = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(lds.band_s[0]) + (bo[e] >> 1));
                        float t = fmaxf(sdb, T.ath_db[16 * lane + e]) - 10.0f;
                        k = (signal_db - t) > smr;
                    }
                    keep |= (k ? 1u : 0u) << e;
                }
            } else {   // quantise<1, false>'s mask: the sign of thr - |c| (see lossy_curve_kernel)
#pragma unroll
                for (int e = 15; e >= 0; e--)
                    keep = __builtin_amdgcn_alignbit(keep, __float_as_uint(max_raw(tb[e], al[e]) - ax[e]), 31);
            }
            int q[1][16];
            uint32_t m = 0;
#pragma unroll
            for (int e = 0; e < 16; e++) {
                q[0][e] = ((keep >> e) & 1u) ? q0[e] : 0;
                m |= (q[0][e] != 0 ? 1u : 0u) << e;
            }
            SparsePlan P[1];
            sparse_plan_m(lane, m, P[0]);
            const uint32_t total = P[0].total;
            if (lane == 32) *reinterpret_cast<uint32_t *>(stage) = total;   // (little-endian length word)
            uint8_t *const dsts[1] = {stage + 4};
            const uint32_t trash[1] = {total + 2u * (uint32_t)lane};
            sparse_emit_n<1>(lane, q, P, dsts, trash);
            wave_sync();
            // the section goes to the rung's running position in the rung's slot: any alignment, dword by dword
            const uint32_t pj = (uint32_t)__builtin_amdgcn_readlane((int)pos, j);
            uint8_t *const slot = slot0 + (unsigned long long)j * rung_stride;
            uint8_t *const dst = slot + pj;
            const uint32_t n = 4u + total, n4 = n >> 2;
            for (uint32_t i = (uint32_t)lane; i < n4; i += 64u) {
                const uint32_t v = reinterpret_cast<const uint32_t *>(stage)[i];
                __builtin_memcpy(dst + 4u * i, &v, 4);
            }
            if ((uint32_t)lane < (n & 3u)) dst[4u * n4 + (uint32_t)lane] = stage[4u * n4 + (uint32_t)lane];
            if (lane < 25) *reinterpret_cast<unsigned short *>(slot + 12 + 50 * ch + 2 * lane) = (unsigned short)sfw;
            if (lane == j) pos += n;
            wave_sync();   // the stage is free again
        }
    }
    if (lane0 < n_q) {   // lane j closes rung j's frame: header (writer.rs:236-254), size, and the clip's DATA bytes
        uint32_t *f = reinterpret_cast<uint32_t *>(slot0 + (unsigned long long)lane0 * rung_stride);
        const uint32_t blob_len = pos - 10u;
        f[0] = 253u | (0x0400u << 8);                              // frame type, frame_samples = 1024
        f[1] = (blob_len & 0xFFFFu) << 16;                         // flags 0 | blob length, low half
        f[2] = (blob_len >> 16) | ((uint32_t)nch << 24);           // ... high half | BlockSize::Long | channels
        A.frame_size[(unsigned long long)lane0 * A.total_frames + gframe] = pos;
        atomicAdd(&sizes[(unsigned long long)lane0 * (unsigned)A.n_clips + clip], (unsigned long long)pos);
    }
}

// The quality level of every file's header (writer.rs:64-68: the high byte of the flags, file byte 7) behind ONE
// launch_finish_files over all rungs of a group, which writes the same flags into every header: file v = rung * count + clip
// gets level[rung]. The header carries no checksum of its own (data_crc32 covers the DATA chunk). One thread per file.
__global__ void ladder_header_levels_kernel(uint8_t *out, const unsigned long long *data_off, const unsigned int *clip_frames,
                                            unsigned int count, unsigned int n_files, LadderLevels lv) {
    const unsigned v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_files) return;
    out[data_off[v] - (74ull + 20ull * clip_frames[v]) + 7] = lv.level[v / count];
}

#define FLO_LAUNCH_CHECK()                     \
    do {                                       \
        hipError_t e_ = hipGetLastError();     \
        if (e_ != hipSuccess) return (int)e_;  \
    } while (0)

int launch_lossy_ladder(const CurveArgs &C, const float *a_t, const float *s_prev, unsigned long long *sizes, hipStream_t s) {
    if (C.n_q < 1 || C.n_q > kMaxCurveCandidates || C.A.nch < 1 || C.A.nch > kMaxLossyChannels) return -1;
    if (C.A.slot_bytes < lossy_slot_bytes(C.A.nch) || !C.A.slots || !C.A.frame_size || !sizes) return -1;
    if (!C.A.total_frames) return 0;
    if (C.A.total_frames * (unsigned long long)C.n_q > 0x7FFFFFFFull) return -1;   // (the compaction's grid covers every rung's frames)
    hipLaunchKernelGGL(lossy_ladder_kernel, dim3((unsigned)C.A.total_frames), dim3(64), 0, s, C, C.A.pcm, a_t, s_prev, sizes);
    FLO_LAUNCH_CHECK();
    return 0;
}

int launch_ladder_header_levels(uint8_t *out, const unsigned long long *data_off, const unsigned int *clip_frames, unsigned int count,
                                unsigned int n_files, const LadderLevels &lv, hipStream_t s) {
    if (!n_files || !count) return 0;
    hipLaunchKernelGGL(ladder_header_levels_kernel, dim3((n_files + 255u) / 256u), dim3(256), 0, s, out, data_off, clip_frames, count, n_files, lv);
    FLO_LAUNCH_CHECK();
    return 0;
}

}  // namespace flo
