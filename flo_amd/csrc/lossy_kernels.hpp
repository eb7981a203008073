// lossy_kernels.hpp — kernel argument block and launchers of the lossy path (see lossy_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "encode_plan.hpp"
#include "lossy_device.hpp"

namespace flo {

struct LossyArgs {
    LossyDevTables T;
    // input
    const float *pcm;                        // all clips, interleaved f32
    const unsigned long long *clip_off;      // [n_clips] float offset of the clip (multiple of 4)
    const unsigned long long *clip_nsf;      // [n_clips] sample-frames per clip
    const unsigned int *clip_hops;           // [n_clips] frames per clip: ceil((nsf + 1024) / 1024)
    const unsigned long long *clip_frame0;   // [n_clips] index of the clip's first frame among all frames
    int nch;
    int n_clips;
    unsigned long long total_frames;
    unsigned int max_hops;                   // longest clip, in frames
    // output
    uint8_t *out;                            // DATA chunks
    const unsigned long long *out_off;       // [n_clips] byte offset of the clip's DATA chunk (16-byte aligned)
    unsigned int *frame_size;                // [total_frames]
    unsigned long long *clip_bytes;          // [n_clips] DATA chunk size
    // frame-parallel form
    float *a_t;                              // [total_frames][nch][32] masking level before temporal masking
    float *bmax_t;                           // [total_frames][nch][32] band maxima (frame-parallel stereo form: pass 1 leaves them for pass 2)
    float4 *coef_t;                          // nullable [total_frames][8][64]: the stereo coefficients as pass 1's lanes hold them (few frames only:
                                             // 8 KB per frame; pass 2 reads them back instead of transforming again)
    float *s_prev_out;                       // [total_frames][nch][32] scan output
    const float *s_prev;                     // same buffer, read by pass 2
    uint8_t *slots;                          // [total_frames][slot_bytes]
    unsigned int slot_bytes;                 // kFrameCap for 1-2 channels, lossy_slot_bytes(nch) beyond
    unsigned long long *frame_off;           // [total_frames] offset of the frame inside its clip's DATA chunk
    // analysis / stage tests (may be null)
    float *dbg_coeffs;                       // [total_frames][nch][1024]
    short *dbg_q;                            // [total_frames][nch][1024]
    unsigned short *dbg_sfw;                 // [total_frames][nch][25]
    const float *in_coeffs;                  // when set: skip the transform, quantise these spectra
    unsigned long long *dbg_stamps;          // diagnostic builds (FLO_STAMPS): per-wave phase cycle sums [wave][16]
    int exact;                               // the exact-threshold instantiations run (lossy_exact): near-threshold coefficients
                                             // and |c| <= 1e-10 are decided with the reference's dB expression
    unsigned int *next_clip;                 // lock-step stereo form: batch-wide counter of claimed clips (zero at launch), then
                                             // the done queue's tail and head counters (next_clip[1], [2]; zero at launch)
    // lock-step stereo form, CRC in the launch's idle tail (crc_ready null: none): a packer wave that finds the batch
    // exhausted computes the CRC slice registers (FinishArgs::part_reg layout) of its last clip and of finished clips
    // it takes from the done queue, and marks them crc_ready[clip] = epoch
    unsigned int *clear_next;                // zeroed at launch: the counters of the launch after this one (other parity)
    union {
        unsigned long long *done_q;          // [n_clips] queue entries: epoch << 32 | clip
        // frame-parallel form (which has no done queue; the union keeps the argument layout of every kernel what it was):
        // the first frame at which a band's level before temporal masking is +inf, per (clip, channel, band):
        // [n_clips][nch][32] words inf_tag << 32 | ~frame, raised by pass 1 with an atomic maximum. A word of another tag
        // is "none": the buffer is zeroed once and every launch sequence brings a tag of its own. Null: no marks are kept.
        unsigned long long *inf_mark;
    };
    unsigned int *crc_ready;                 // [n_clips]
    unsigned int *part_reg;                  // [n_clips * parts]
    unsigned int parts;                      // slices per clip (finish_parts)
    union {
        unsigned int epoch;                  // of this launch, never 0
        unsigned int inf_tag;                // frame-parallel form: of this launch sequence, never 0
    };
    const unsigned int *crc_tab;             // crc_device_tables()
    int n_cus;                               // compute units of the device (persistent workgroups)
    unsigned int chain2q_pturns;             // lock-step stereo form, set by its launcher (launches of one round): packers that share
                                             // a SIMD go first in turn, frame by frame (0: the older one always wins issue)
};

// Whether a launch runs the exact-threshold instantiations (quantise<., EXACT = true>): when the caller asks for the
// yardstick, and always at quality >= 0.99. There the reference keeps a coefficient of |c| <= 1e-10 wherever its threshold is
// below 0 dB (its level is pinned at -100 dB, the keep threshold's own value) and quantises it with 30000 / band_max: a
// non-zero integer on fade and reverb tails whose band maximum is just above 1e-10. The amplitude-domain test
// |c| > max(T_band, T_ath) of the shipped instantiations cannot express that (it is not monotone in |c|), and the flag is
// uniform per launch: the choice is made here, on the host, and the kernels of every other quality stay as they are.
inline bool lossy_exact(bool asked, const LossyDevTables &T) { return asked || T.q_transparent != 0; }

// the launchers launch the kernels the plan names (encode_plan.hpp); they choose only the launch geometry
int launch_lossy_chain(const LossyArgs &A, const LossyPlan &P, hipStream_t s);
// stereo only: one lock-step transform wave + one quantiser-and-packer wave per clip. masks: the band table's lane masks
// in device memory (LossyTablesHost::masks of the table set A.T comes from)
int launch_lossy_chain2q(const LossyArgs &A, const LossyPlan &P, const StatMasks *masks, hipStream_t s);
int launch_lossy_frames_pass(const LossyArgs &A, FrameKernel k, hipStream_t s);
// bytes reserved per frame in the frame-parallel form: header + scale words + every channel's largest sparse blob
inline unsigned int lossy_slot_bytes(int nch) {
    unsigned int need = 12u + 50u * (unsigned)nch + (unsigned)nch * (4u + 2064u) + 16u;
    need = (need + 15u) & ~15u;
    return need < (unsigned)kFrameCap ? (unsigned)kFrameCap : need;
}
constexpr int kMaxLossyChannels = 8;      // more channels than two take the generic frame-parallel kernel
int launch_lossy_scan(const LossyArgs &A, hipStream_t s);
int launch_lossy_compact(const LossyArgs &A, CompactKernel k, hipStream_t s);
// Stream step (flo_stream_encode_ready, lstream.cpp): the frame-parallel passes over streams' windows are the instantiations
// of the frame kernels with PASS | kStreamStep (lossy_frame_kernel<1, .>, lossy_frame2x_kernel, lossy_frame_n_kernel by
// A.nch); the temporal scan is seeded from the streams' carried levels and leaves their new ones.
constexpr int kStreamStep = 4;
int launch_lossy_stream_pass(const LossyArgs &A, int pass, hipStream_t s);
int launch_lossy_stream_scan(const LossyArgs &A, const float *seed, float *level_out, hipStream_t s);
// stream step (flo_stream_encode_ready, lstream.cpp): pass 1 or 2 of the frame-parallel form over streams' windows (the
// kernel by A.nch: 1, 2, 3..8 channels), and the temporal scan seeded from the streams' carried levels
int launch_lossy_stream_pass(const LossyArgs &A, int pass, hipStream_t s);
int launch_lossy_stream_scan(const LossyArgs &A, const float *seed, float *level_out, hipStream_t s);
// Size curve (flo_batch_size_curve, rate.cpp): behind pass 1 and the temporal scan of the frame-parallel form, whose levels
// do not depend on quality, lossy_curve_kernel prices every candidate quality from one transform of each frame. The
// per-candidate constants are the host's, exactly as an encode at that quality gets them (build_lossy_tables).
constexpr int kMaxCurveCandidates = 32;
struct CurveArgs {
    LossyArgs A;                                  // T (of any quality), the clip tables, nch, n_clips, total_frames
    int n_q;                                      // candidates, 1 .. kMaxCurveCandidates
    unsigned int exact_mask;                      // bit j: candidate j runs the exact-threshold branch (lossy_exact)
    unsigned int qtrans_mask;                     // bit j: LossyDevTables::q_transparent of candidate j
    float smr_thr[kMaxCurveCandidates];           // LossyDevTables::smr_thr of candidate j
    const float4 *ath[kMaxCurveCandidates];       // rows kRowAth .. kRowAth + 3 of candidate j's pack: ath_lin, [4][64] float4
};
// sizes[clip * n_q + j] += the sparse bytes of every (frame, channel) of the clip at candidate j (integer atomics)
int launch_lossy_curve(const CurveArgs &C, const float *a_t, const float *s_prev, unsigned long long *sizes, hipStream_t s);
// Quality ladder (flo_batch_encode_ladder, ladder.cpp; ladder_kernels.hip): behind the same pass 1 and scan, lossy_ladder_kernel packs every
// frame at every rung (C's candidates) from one transform. C.A.slots: [n_q][total_frames][slot_bytes], C.A.frame_size:
// [n_q][total_frames], C.A.slot_bytes >= lossy_slot_bytes(nch); sizes[rung * n_clips + clip] += the clip's DATA bytes at
// that rung (zeroed by the caller). n_q * total_frames stays below 2^31.
int launch_lossy_ladder(const CurveArgs &C, const float *a_t, const float *s_prev, unsigned long long *sizes, hipStream_t s);
// ... and behind one launch_finish_files over all rungs of a group (files rung-major, `count` per rung), the header byte
// that differs from rung to rung: the quality level (the flags' high byte) of file v is level[v / count]
struct LadderLevels {
    unsigned char level[kMaxCurveCandidates];
};
int launch_ladder_header_levels(uint8_t *out, const unsigned long long *data_off, const unsigned int *clip_frames, unsigned int count,
                                unsigned int n_files, const LadderLevels &lv, hipStream_t s);
int launch_mdct_only(const LossyDevTables &T, const float *frames, unsigned long long n, float *out, hipStream_t s);
int launch_quantise_smr(const LossyDevTables &T, const float *coeffs, const float *smr, unsigned long long n, short *q, float *sf,
                        hipStream_t s);
int launch_sparse_only(const short *q, unsigned long long n, uint8_t *slots, uint32_t *sizes, int form, hipStream_t s);
int launch_pack_streams(const uint8_t *src, const unsigned long long *src_off, const unsigned long long *dst_off,
                        const unsigned long long *sizes, int n_clips, uint8_t *dst, hipStream_t s);
int launch_synth_fill(float *pcm, const unsigned long long *clip_off, const unsigned long long *clip_nsf, int n_clips,
                      int nch, uint32_t seed, unsigned long long clip_id0, hipStream_t s);

}  // namespace flo
