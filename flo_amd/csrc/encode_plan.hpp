// encode_plan.hpp — which kernels an encode launches, decided once on the host from what the host knows (channels,
// clips, frames, the requested form and the analysis options) and handed to the launchers as plain data. The lossy
// plan covers flo_batch_encode's lossy forms; the finish plan covers finish_files (lossy and lossless batches). The
// launchers in lossy_kernels.hip and container_kernels.hip keep only the launch geometry (clips per workgroup, grids,
// LDS). Plain C++: no HIP headers, so a host test builds it with g++ alone.
#pragma once
#include <cstddef>
#include <cstdint>

namespace flo {

// "Few clips": below this, the bookkeeping kernels run 1024 threads per clip and finish_files fuses the CRC slices with
// the TOC; from it, the stereo chain encode computes the files' CRCs in its idle tail and finish_files<256> takes the rest.
constexpr size_t kFewClips = 64;
// up to this many clips, the frame-parallel form fuses frame offsets and compaction into one launch
constexpr size_t kFusedCompactClips = 16;
// the frame-parallel stereo form hands pass 1's coefficients (8 KB per frame) to pass 2 up to this size
constexpr size_t kCoefHandoverBytes = (size_t)256 << 20;
// DIRTY (template parameter of the lock-step chain kernel): the element positions (bit e of 16) at which some lane of the band
// table closes a segment; the other positions skip the slot store and the restart multiplication of band_stats_2. 0xFFFF
// serves every table; the plan picks the instantiation made for 44.1 kHz when the table agrees.
constexpr uint32_t kDirty44k = 0xBDBEu;

enum class LossyForm : uint8_t {
    Chain2q = 5,   // stereo: lock-step transform wave + quantiser-and-packer wave per clip (forms 3 and 4 mean it too)
    Chain = 1,     // one wave per (clip, channel)
    Frames = 2,    // frame-parallel: pass 1, scan, pass 2, compaction
};
enum class Chain2qKernel : uint8_t {   // lossy_chain2q_kernel<COEFFS, DIRTY, DBG>
    None,
    InCoeffs,   // <true, 0xFFFF, true>
    Debug,      // <false, 0xFFFF, true>
    Dirty44k,   // <false, kDirty44k, false>
    Generic,    // <false, 0xFFFF, false>
};
enum class ChainKernel : uint8_t {   // lossy_chain_kernel<NW, EXACT>
    None,
    Mono,          // <1, false>
    MonoExact,     // <1, true>
    Stereo,        // <2, false>
    StereoExact,   // <2, true>
};
enum class FrameKernel : uint8_t {
    None,
    Mono1, Mono2, Mono2Exact,             // lossy_frame_kernel<1, PASS, EXACT>
    Stereo1, Stereo2, Stereo2Exact,       // lossy_frame_kernel<2, PASS, EXACT>
    Pair1, Pair2,                         // lossy_frame2x_kernel<PASS>: both channels in lock-step
    Pair2FromCoef,                        // lossy_frame2x_kernel<2, true>: pass 1's coefficients, walks the temporal chain itself
    Multi1, Multi2, Multi2Exact,          // lossy_frame_n_kernel<PASS, EXACT>
};
enum class CompactKernel : uint8_t {
    None,
    Fused,         // lossy_offsets_compact_kernel
    Offsets1024,   // lossy_frame_offsets_kernel<1024> + lossy_compact_kernel
    Offsets256,    // lossy_frame_offsets_kernel<256> + lossy_compact_kernel
};

struct LossyPlanInput {
    int which = 0;        // flo_batch_encode's form: 0 = the context's forced form, else the analysis default or auto
    int force_path = 0;   // flo_ctx_force_path
    unsigned ch = 0;
    size_t n_clips = 0;
    uint64_t total_frames = 0;
    bool exact = false, in_coeffs = false;
    bool debug = false;   // analysis buffers (coefficients, q, scale words) requested: the analysis entry points
    uint32_t dirty = 0;   // the band table's LossyDevTables::dirty
    bool tail_crc = true;      // FLO_TAIL_CRC unset or not "0"
    int chain2q_clips = 0;     // FLO_CHAIN2X_CLIPS (diagnostic: clips per workgroup; 0 = by batch size)
};

struct LossyPlan {
    LossyForm form = LossyForm::Chain;
    Chain2qKernel chain2q = Chain2qKernel::None;
    int chain2q_clips = 0;
    ChainKernel chain = ChainKernel::None;
    FrameKernel pass1 = FrameKernel::None, pass2 = FrameKernel::None;
    bool coef_handover = false;   // the frame scratch includes the coefficient hand-over buffer
    CompactKernel compact = CompactKernel::None;
    bool crc_ready = false;       // many stereo clips: ready words per clip, the finished sizes come back behind finish_files
    bool tail_crc = false;        // ... and the launch's tail computes CRC slice registers
    // pass 2 from handed-over coefficients walks the temporal chain itself: the scan runs in the other frame-parallel cases
    bool scan() const { return form == LossyForm::Frames && pass2 != FrameKernel::Pair2FromCoef; }
};
LossyPlan plan_lossy(const LossyPlanInput &in);

// CRC slices per clip so that about two thousand workgroups run; at most 128, or 512 for few clips, whose finish runs
// 1024 threads (one per slice register)
unsigned finish_parts(size_t n_clips);

struct FinishPlan {
    bool fused = false;        // crc_and_toc_kernel, then finish_files_kernel<1024> writes CRC + header
    bool crc_slices = false;   // crc_slices_kernel runs before finish_files
    unsigned threads = 0;      // finish_files_kernel<1024> or <256>
    unsigned parts = 0;        // finish_parts
};
// crc_ready: the encode left per-clip ready words (LossyPlan::crc_ready); max_frames 0 = unknown
FinishPlan plan_finish(size_t n_clips, unsigned max_frames, bool crc_ready);

}  // namespace flo
