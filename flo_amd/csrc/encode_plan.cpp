// encode_plan.cpp — see encode_plan.hpp.
#include "encode_plan.hpp"

namespace flo {

// which (0 = the forced form, then the analysis default 1 or auto) -> the form that runs
static LossyForm lossy_form(const LossyPlanInput &in) {
    if (in.ch > 2) return LossyForm::Frames;   // more than two channels: the generic frame-parallel kernels
    int w = in.which ? in.which : in.force_path;
    // the analysis entry points default to form 1; auto: the chain forms once the batch fills the chip, else frame-parallel
    if (!w) w = in.debug ? 1 : in.n_clips * in.ch >= 512 ? (in.ch == 2 ? 5 : 1) : 2;
    if (w == 3 || w == 4) w = 5;   // (earlier rounds' stereo chain forms: retired, the numbers stay valid)
    if (w == 5 && (in.exact || in.ch != 2)) w = 1;   // the exact-threshold yardstick and mono live in the one-wave-per-channel form
    return (LossyForm)w;
}

LossyPlan plan_lossy(const LossyPlanInput &in) {
    LossyPlan p;
    p.form = lossy_form(in);
    const bool ex = in.exact;
    switch (p.form) {
    case LossyForm::Chain2q:
        if (in.in_coeffs) p.chain2q = Chain2qKernel::InCoeffs;
        else if (in.debug) p.chain2q = Chain2qKernel::Debug;
        else p.chain2q = (in.dirty | 0x8000u) == kDirty44k ? Chain2qKernel::Dirty44k : Chain2qKernel::Generic;
        p.chain2q_clips = in.chain2q_clips;
        p.crc_ready = in.n_clips >= kFewClips;
        p.tail_crc = p.crc_ready && in.tail_crc;
        break;
    case LossyForm::Chain:
        if (in.ch == 1) p.chain = ex ? ChainKernel::MonoExact : ChainKernel::Mono;
        else p.chain = ex ? ChainKernel::StereoExact : ChainKernel::Stereo;
        break;
    case LossyForm::Frames:
        // one 3-minute clip: 63 MB that never leave the memory-side cache; a batch of thousands of clips forced into this
        // form transforms twice instead
        p.coef_handover = in.ch == 2 && in.total_frames * 8192 <= kCoefHandoverBytes;
        if (in.ch == 1) {
            p.pass1 = FrameKernel::Mono1;
            p.pass2 = ex ? FrameKernel::Mono2Exact : FrameKernel::Mono2;
        } else if (in.ch == 2 && !ex && !in.in_coeffs) {
            p.pass1 = FrameKernel::Pair1;
            p.pass2 = p.coef_handover ? FrameKernel::Pair2FromCoef : FrameKernel::Pair2;
        } else if (in.ch == 2) {
            p.pass1 = FrameKernel::Stereo1;
            p.pass2 = ex ? FrameKernel::Stereo2Exact : FrameKernel::Stereo2;
        } else {
            p.pass1 = FrameKernel::Multi1;
            p.pass2 = ex ? FrameKernel::Multi2Exact : FrameKernel::Multi2;
        }
        if (in.n_clips <= kFusedCompactClips) p.compact = CompactKernel::Fused;
        else p.compact = in.n_clips < kFewClips ? CompactKernel::Offsets1024 : CompactKernel::Offsets256;
        break;
    }
    return p;
}

unsigned finish_parts(size_t n_clips) {
    if (n_clips >= 1024) return 1;
    const size_t p = (2048 + n_clips - 1) / (n_clips ? n_clips : 1);
    const size_t cap = n_clips < kFewClips ? 512 : 128;
    return (unsigned)(p > cap ? cap : p);
}

FinishPlan plan_finish(size_t n_clips, unsigned max_frames, bool crc_ready) {
    FinishPlan f;
    const bool few = n_clips < kFewClips;
    f.fused = few && max_frames;
    // (with ready words, finish_files_kernel<256> computes the CRCs the encode's tail did not)
    f.crc_slices = !f.fused && (few || !crc_ready);
    f.threads = few ? 1024 : 256;
    f.parts = finish_parts(n_clips);
    return f;
}

}  // namespace flo
